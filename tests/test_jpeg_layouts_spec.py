"""Pins the oracle's JPEG front end against libjpeg on files NO ENCODER AT HAND WRITES: tests/jpeg_writer.py makes them from
quantised coefficients, in the sampling layouts, table ids, header orders and Huffman tables that Pillow's libjpeg never
emits (tests/test_oracle_jpeg.py covers what it does emit).  Where libjpeg decodes, the oracle returns 0 and the same
pixels; where libjpeg raises, the oracle returns JPG_NEEDS_HOST; two classes libjpeg decodes are refused BY DESIGN (no luma
component to take; luma coded below the MCU's resolution).

The corpora built here are the ones tests/test_jpeg_layouts_gpu.py runs on the device; which decoder path a file takes is
COMPUTED from the writer's facts and the rules of ucfp_amd/csrc/jpeg.hip restated below, never assumed."""
import functools
from collections import namedtuple

import numpy as np
import pytest

pytest.importorskip("PIL.Image")

from jpeg_writer import comb_table, rand_coefs, scan_geometry, write_jpeg   # noqa: E402
from test_oracle_jpeg import libjpeg_luma                     # noqa: E402

# ---- the rules of jpeg.hip that decide a file's path (quoted; a change there shows up as a coverage assertion here) ----
SPEC_MAX_BLOCKS = 6          # kSpecMaxB: blocks per MCU the speculative kernel takes
SPEC_MIN_BYTES = 512         # jpeg_takes_spec: unstuffed bytes below which the serial lane decodes the one segment
WAVE_LANES = 64              # jpeg_huff_kernel: restart intervals decoded per round
MAX_BLOCKS_PER_MCU = 10      # T.81 B.2.3


def takes_spec(f):
    """jpeg_takes_spec: one segment, no DRI, >= 512 unstuffed bytes, <= 6 blocks per MCU."""
    return f.n_seg == 1 and f.restart == 0 and f.clean_len >= SPEC_MIN_BYTES and f.blocks_per_mcu <= SPEC_MAX_BLOCKS


def spec_waves(files):
    """launch_jpeg_decode: waves per file of the speculative kernel, from the batch's count and mean size -- doubled while
    the batch stays within 2048 wave slots and a subsequence keeps >= 256 bits."""
    n = len(files)
    mean_bits = sum(len(f.data) for f in files) // n * 8
    nw = 1
    while nw < 8 and n * nw * 2 <= 2048 and mean_bits // (64 * nw * 2) >= 256:
        nw *= 2
    return nw


def max_seg(w, h):
    """jpeg_plane_geometry: the restart intervals a file's segment table holds."""
    return min(-(-w // 8) * -(-h // 8), 1 << 20)


# expect: "decode" (libjpeg, oracle and device: status 0, the same pixels), "refused" (libjpeg raises: NEEDS_HOST) or
# "design" (libjpeg decodes; NEEDS_HOST by design)
Case = namedtuple("Case", "name f expect samp")

Y411 = ((4, 1), (1, 1), (1, 1))
Y440 = ((1, 2), (1, 1), (1, 1))
Y311 = ((3, 1), (1, 1), (1, 1))
Y420 = ((2, 2), (1, 1), (1, 1))
B7 = ((2, 2), (2, 1), (1, 1))
B8 = ((2, 2), (1, 2), (1, 2))
B10 = ((4, 2), (1, 1), (1, 1))
ALL21 = ((2, 1), (2, 1), (2, 1))
GREY22 = ((2, 2),)
GREY11 = ((1, 1),)
LAYOUTS = (Y411, Y440, Y311, B7, B8, B10, ALL21, GREY22, GREY11)
GEOMETRIES = ((1, 1), (37, 29), (96, 80), (160, 128))
OVER_TEN = (((4, 4), (1, 1), (1, 1)), ((3, 3), (1, 1), (3, 1)), ((3, 3), (1, 1), (1, 1)))     # 18, 13, 11 blocks
LUMA_BELOW = (((1, 1), (2, 2), (2, 2)), ((1, 2), (2, 1), (1, 1)))


def _name(samp, w, h, *more):
    return "-".join(["".join("%d%d" % s for s in samp), "%dx%d" % (w, h)] + [str(m) for m in more])


def _mcus(w, h, samp):
    mx, my, _ = scan_geometry(w, h, samp)
    return mx, my


@functools.lru_cache(maxsize=None)
def corpus_layouts():
    """(a) every layout x geometry x restart interval {0, 1, 3, one MCU row, more than the MCU count}, and for the files
    whose MCU count is a multiple of 64 the interval that makes exactly 64 segments."""
    out = []
    for li, samp in enumerate(LAYOUTS):
        for gi, (w, h) in enumerate(GEOMETRIES):
            mx, my = _mcus(w, h, samp)
            restarts = [0, 1, 3, mx, mx * my + 7]                  # (a 1 x 1 file: one MCU row is one MCU)
            if (mx * my) % WAVE_LANES == 0:
                restarts.append(mx * my // WAVE_LANES)
            for r in dict.fromkeys(restarts):
                rng = np.random.default_rng(1000 * li + 10 * gi + r)
                f = write_jpeg(rand_coefs(rng, w, h, samp, 0.5, 12), w, h, samp, restart=r)
                out.append(Case(_name(samp, w, h, "r%d" % r), f, "decode", samp))
    return out


# (b) coefficient density and amplitude at 160 x 128 that put a file of the layout into the middle of the size band of 2, 4
# and 8 waves (about 6, 12 and 22 KB: the bands begin at 4, 8 and 16 KiB for batches of 8)
WAVE_LAYOUTS = (Y411, Y440, ALL21)
WAVE_DENSITY = {Y411: {2: (0.6, 12), 4: (1.6, 24), 8: (6.0, 60)},
                Y440: {2: (0.4, 10), 4: (1.0, 16), 8: (3.0, 40)},
                ALL21: {2: (0.3, 8), 4: (0.6, 12), 8: (1.6, 24)}}


@functools.lru_cache(maxsize=None)
def corpus_waves():
    """-> {(layout, waves wanted): [8 files]}"""
    out = {}
    for li, samp in enumerate(WAVE_LAYOUTS):
        for nw, (density, amp) in WAVE_DENSITY[samp].items():
            w, h = 160, 128
            files = []
            for i in range(8):
                rng = np.random.default_rng(7000 + 100 * li + 10 * nw + i)
                f = write_jpeg(rand_coefs(rng, w, h, samp, density, amp), w, h, samp, quant={0: np.ones(64, int), 1: np.full(64, 2)})
                files.append(Case(_name(samp, w, h, "w%d" % nw, i), f, "decode", samp))
            out[(samp, nw)] = files
    return out


@functools.lru_cache(maxsize=None)
def corpus_headers():
    """(c) one file per header variant at 37 x 29 and 96 x 80."""
    items = [
        ("sof1", Y420, dict(sof=0xC1), "decode"),
        ("tq322", Y420, dict(tq=[3, 2, 2]), "decode"),
        ("huff100", Y420, dict(td=[1, 0, 0], ta=[1, 0, 0]), "decode"),
        ("huff322", Y420, dict(td=[3, 2, 2], ta=[3, 2, 2], sof=0xC1), "decode"),
        ("huff322-sof0", Y420, dict(td=[3, 2, 2], ta=[3, 2, 2]), "decode"),
        ("one-segment-tables", Y420, dict(one_dht=True, one_dqt=True), "decode"),
        ("segment-per-table", Y420, dict(one_dht=False, one_dqt=False), "decode"),
        ("fills", Y420, dict(fills=True, restart=2), "decode"),
        ("dri-first", Y420, dict(dri_first=True, restart=2), "decode"),
        ("com-before-sof", Y420, dict(com=(("pre_sof", 0xFE, 65533),)), "decode"),
        ("app5-before-sos", Y420, dict(com=(("pre_sos", 0xE5, 65533),)), "decode"),
        ("ids012", Y420, dict(cids=(0, 1, 2), jfif=False), "decode"),
        ("ids102030", Y420, dict(cids=(10, 20, 30), jfif=False), "decode"),
        ("idsYCc", Y420, dict(cids=("Y", "C", "c"), jfif=False), "decode"),
        ("adobe1", Y420, dict(adobe=1, jfif=False), "decode"),
        ("idsRGB", GREY11 * 3, dict(cids=("R", "G", "B"), jfif=False), "design"),
        ("adobe0", GREY11 * 3, dict(adobe=0, jfif=False), "design"),
        ("luma-below-a", LUMA_BELOW[0], {}, "design"),
        ("luma-below-b", LUMA_BELOW[1], {}, "design"),
        ("blocks18", OVER_TEN[0], {}, "refused"),
        ("blocks13", OVER_TEN[1], {}, "refused"),
        ("blocks11", OVER_TEN[2], {}, "refused"),
        ("blocks10", B10, {}, "decode"),
    ]
    out = []
    for gi, (w, h) in enumerate(((37, 29), (96, 80))):
        for ii, (name, samp, kw, expect) in enumerate(items):
            rng = np.random.default_rng(3000 + 100 * gi + ii)
            f = write_jpeg(rand_coefs(rng, w, h, samp, 0.5, 12), w, h, samp, **kw)
            out.append(Case(_name(samp, w, h, name), f, expect, samp))
    return out


def comb_tables(cls, tid, freq):
    """Explicit "comb" tables for write_jpeg(huff=...): the file's most frequent symbols get 16-bit codes.  DC tables list all
    twelve size categories (used or not) and keep a code of 10 bits; AC tables list the symbols the file uses."""
    if cls == 0:
        return comb_table(sorted(range(12), key=lambda s: (-freq[s], s)), (10, 12))
    used = [s for s in sorted(range(256), key=lambda s: (-freq[s], s)) if freq[s]]
    return comb_table(used, (11, 12, 13, 14, 15))


@functools.lru_cache(maxsize=None)
def corpus_long_codes():
    """(d) comb tables on a file of the speculative path, a restart file and a one-component file."""
    out = []
    for i, (samp, w, h, r) in enumerate(((Y411, 96, 80, 0), (Y420, 96, 80, 3), (GREY11, 96, 80, 0), (Y440, 37, 29, 1))):
        rng = np.random.default_rng(4000 + i)
        f = write_jpeg(rand_coefs(rng, w, h, samp, 1.0, 7), w, h, samp, restart=r, huff=comb_tables)
        out.append(Case(_name(samp, w, h, "comb", "r%d" % r), f, "decode", samp))
    return out


# (e) what the 64-byte steps of jpeg_scan_kernel can cut: offsets are from the first scan byte, as the kernel's steps are
def ff_straddles_step(f):
    return bool(np.any(f.stuffed_ff % 64 == 63))


def rst_straddles_step(f):
    return bool(np.any(f.rst % 64 == 63))


def rst_after_stuffed_pair_straddles_step(f):
    """FF 00 | FF at the end of a step, the marker's Dn opening the next"""
    r = f.rst[f.rst % 64 == 63]
    return bool(np.isin(r - 2, f.stuffed_ff).any())


def eoi_opens_step(f):
    return f.scan_len % 64 == 0


def _search(pred, samp, w, h, restart, first_seed):
    for seed in range(first_seed, first_seed + 400):
        rng = np.random.default_rng(seed)
        f = write_jpeg(rand_coefs(rng, w, h, samp, 1.0, 60), w, h, samp, restart=restart,
                       quant={0: np.ones(64, int), 1: np.ones(64, int)})
        if pred(f):
            return Case(_name(samp, w, h, pred.__name__, "seed%d" % seed), f, "decode", samp)
    raise AssertionError("no file with %s among 400 seeds" % pred.__name__)


@functools.lru_cache(maxsize=None)
def corpus_unstuffer():
    """-> {fact: Case}: dense high-amplitude coefficients (many FF bytes), seeds searched until the writer's offsets show
    the boundary case."""
    return {
        "ff": _search(ff_straddles_step, Y420, 96, 80, 0, 0),
        "ff-1comp": _search(ff_straddles_step, GREY11, 37, 29, 0, 0),
        "rst": _search(rst_straddles_step, Y420, 96, 80, 1, 0),
        "rst-pair": _search(rst_after_stuffed_pair_straddles_step, GREY11, 160, 128, 1, 0),
        "eoi": _search(eoi_opens_step, Y420, 37, 29, 0, 0),
        "eoi-rst": _search(eoi_opens_step, GREY11, 37, 29, 2, 0),
    }


def all_cases():
    out = list(corpus_layouts()) + list(corpus_headers()) + list(corpus_long_codes()) + list(corpus_unstuffer().values())
    for files in corpus_waves().values():
        out += files
    return out


# ---- the judges: libjpeg and the oracle, once per file and session ----
_judged = {}


def libjpeg_or_none(data):
    try:
        return libjpeg_luma(data)
    except (OSError, SyntaxError, ValueError):
        return None


def judged(oracle, case):
    """-> (oracle status, oracle pixels, libjpeg pixels or None where it raises)"""
    got = _judged.get(case.name)
    if got is None:
        rc, px = oracle.jpeg_decode_luma(case.f.data)
        got = _judged[case.name] = (rc, px, libjpeg_or_none(case.f.data))
    return got


def check_against_libjpeg(oracle, case):
    """The oracle's verdict on one file against libjpeg's; -> 1 if the file decoded."""
    rc, px, lj = judged(oracle, case)
    f = case.f
    if case.expect == "decode":
        # (the precondition of the device tests: libjpeg takes the file and no J4 range guard trips)
        assert lj is not None, "libjpeg refuses " + case.name
        assert rc == 0, "the oracle hands %s to the host: status %d" % (case.name, rc)
        assert oracle.jpeg_probe(f.data) == (0, f.w, f.h), case.name
        assert px.shape == lj.shape == (f.h, f.w) and np.array_equal(px, lj), case.name
        return 1
    if case.expect == "refused":
        assert lj is None, "libjpeg decodes " + case.name
    else:
        assert lj is not None, "libjpeg refuses " + case.name
    assert rc == oracle.JPG_NEEDS_HOST, "%s: status %d" % (case.name, rc)
    return 0


def test_corpus_names_are_unique():
    names = [c.name for c in all_cases()]
    assert len(set(names)) == len(names)


def test_layouts_equal_libjpeg(oracle):
    cases = corpus_layouts()
    for samp in LAYOUTS:
        for w, h in GEOMETRIES:
            fs = [c.f for c in cases if c.samp == samp and (c.f.w, c.f.h) == (w, h)]
            assert {0, 1, 3} <= {f.restart for f in fs} and any(f.restart > f.n_mcu for f in fs), (samp, w, h)
            assert any(f.restart * _mcus(w, h, samp)[1] == f.n_mcu for f in fs), (samp, w, h)       # one MCU row
    assert sum(check_against_libjpeg(oracle, c) for c in cases) == len(cases)


def test_layout_corpus_covers_every_decoder_path():
    """Computed from the writer's facts and the rules quoted at the top: if a threshold moves, the assertion that fails
    names what the corpus no longer reaches."""
    files = [c.f for c in corpus_layouts()]
    small = [s for s in LAYOUTS if sum(h * v for h, v in s) <= SPEC_MAX_BLOCKS or len(s) == 1]
    for samp in small:
        assert any(takes_spec(c.f) for c in corpus_layouts() if c.samp == samp), \
            "no speculative-path file of layout %s" % (samp,)
    assert any(takes_spec(f) and f.blocks_per_mcu == SPEC_MAX_BLOCKS and f.ncomp == 3 for f in files), "no 6-block speculative file"
    one_seg = [f for f in files if f.n_seg == 1 and not takes_spec(f)]
    assert any(f.blocks_per_mcu > SPEC_MAX_BLOCKS for f in one_seg), "no single-segment serial file of more than 6 blocks"
    assert any(f.blocks_per_mcu <= SPEC_MAX_BLOCKS and f.restart == 0 and f.clean_len < SPEC_MIN_BYTES for f in one_seg), \
        "no single-segment serial file below 512 bytes"
    assert any(f.blocks_per_mcu <= SPEC_MAX_BLOCKS and f.restart > 0 for f in one_seg), "no single-segment file with a DRI"
    assert any(f.n_seg > WAVE_LANES for f in files), "no file of more than 64 segments"
    assert any(f.n_seg == WAVE_LANES for f in files), "no file of exactly 64 segments"
    assert any(1 < f.n_seg < WAVE_LANES for f in files)
    assert any(f.ncomp == 1 and f.restart == 1 and f.n_seg == max_seg(f.w, f.h) and f.n_seg > 1 for f in files), \
        "no one-component file whose segment count is max_seg"
    assert {f.blocks_per_mcu for f in files} == {1, 4, 5, 6, 7, 8, 10}


def test_wave_batches_equal_libjpeg_and_hit_2_4_8_waves(oracle):
    n = 0
    for (samp, nw), cases in corpus_waves().items():
        files = [c.f for c in cases]
        assert len(files) == 8 and all(takes_spec(f) for f in files), (samp, nw)
        assert spec_waves(files) == nw, (samp, nw, spec_waves(files), sum(len(f.data) for f in files) // 8)
        n += sum(check_against_libjpeg(oracle, c) for c in cases)
    assert n == 8 * len(WAVE_LAYOUTS) * 3
    assert {nw for _, nw in corpus_waves()} == {2, 4, 8}


def test_header_variants(oracle):
    cases = corpus_headers()
    want = sum(c.expect == "decode" for c in cases)
    assert want == 2 * 16 and len(cases) - want == 2 * 7
    assert sum(check_against_libjpeg(oracle, c) for c in cases) == want
    big = [c.f for c in cases if "com-before-sof" in c.name or "app5-before-sos" in c.name]
    assert len(big) == 4 and all(len(f.data) > 65533 for f in big)


@pytest.mark.parametrize("samp", OVER_TEN + (B10,), ids=lambda s: "".join("%d%d" % x for x in s))
def test_more_than_ten_blocks_per_mcu_go_to_the_host(oracle, samp):
    """T.81 B.2.3: an interleaved MCU holds at most 10 blocks.  libjpeg refuses a frame that declares more, so the oracle (and
    the device) hand it to the host; exactly 10 blocks decode."""
    w, h = 96, 80
    blocks = sum(hh * v for hh, v in samp)
    for r in (0, 2):
        f = write_jpeg(rand_coefs(np.random.default_rng(blocks + r), w, h, samp, 0.5, 12), w, h, samp, restart=r)
        assert f.blocks_per_mcu == blocks
        rc, px = oracle.jpeg_decode_luma(f.data)
        lj = libjpeg_or_none(f.data)
        if blocks > MAX_BLOCKS_PER_MCU:
            assert lj is None and rc == oracle.JPG_NEEDS_HOST, (samp, rc)
        else:
            assert rc == 0 and np.array_equal(px, lj)


def test_long_codes(oracle):
    cases = corpus_long_codes()
    assert sum(check_against_libjpeg(oracle, c) for c in cases) == len(cases)
    files = [c.f for c in cases]
    for f in files:
        hist = f.code_len_hist
        assert 2 * hist[10:].sum() >= hist.sum(), hist          # at least half of the coded symbols: more than 9 bits
        assert hist[16] > 0 and hist[1:10].sum() > 0, hist
    assert any(takes_spec(f) for f in files), "no comb-table file on the speculative path"
    assert any(f.n_seg > 1 for f in files) and any(f.ncomp == 1 for f in files)
    assert {l for f in files for l in np.nonzero(f.code_len_hist)[0]} >= {10, 11, 12, 16}


def test_unstuffer_boundaries(oracle):
    cases = corpus_unstuffer()
    assert sum(check_against_libjpeg(oracle, c) for c in cases.values()) == len(cases)
    assert ff_straddles_step(cases["ff"].f) and ff_straddles_step(cases["ff-1comp"].f)
    assert rst_straddles_step(cases["rst"].f)
    f = cases["rst-pair"].f
    assert rst_after_stuffed_pair_straddles_step(f)
    r = int(f.rst[(f.rst % 64 == 63) & np.isin(f.rst - 2, f.stuffed_ff)][0])
    scan = f.data[f.scan_off:]
    assert scan[r - 2:r + 1] == b"\xff\x00\xff" and 0xD0 <= scan[r + 1] <= 0xD7 and (r + 1) % 64 == 0
    for k in ("eoi", "eoi-rst"):
        f = cases[k].f
        assert eoi_opens_step(f) and f.data[f.scan_off + f.scan_len:] == b"\xff\xd9"
    assert cases["eoi-rst"].f.n_seg > 1


def test_writer_facts_describe_the_file():
    """The facts the path assertions rest on, recomputed from the bytes by a plain scan."""
    for c in all_cases():
        f = c.f
        scan = f.data[f.scan_off:-2]
        assert len(scan) == f.scan_len and f.data[-2:] == b"\xff\xd9"
        ffs, rsts, clean, i = [], [], 0, 0
        while i < len(scan):
            if scan[i] == 0xFF:
                if scan[i + 1] == 0:
                    ffs.append(i)
                    clean += 1
                else:
                    assert scan[i + 1] == 0xD0 + len(rsts) % 8, c.name
                    rsts.append(i)
                i += 2
            else:
                clean += 1
                i += 1
        assert ffs == list(f.stuffed_ff) and rsts == list(f.rst) and clean == f.clean_len, c.name
        assert f.n_seg == len(rsts) + 1 == (-(-f.n_mcu // f.restart) if f.restart else 1), c.name
