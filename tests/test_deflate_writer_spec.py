"""The deflate / PNG corpus of tests/deflate_writer.py, checked without a GPU: every valid stream inflates in zlib and in the
oracle to the bytes the writer says and opens in Pillow to the writer's pixels; every invalid one is refused; and the coverage
each family claims (which codes are long, which bit phases are met, which token words sit on a seam) is computed from the
writer's report and asserted, so that an edit to a generator cannot quietly empty a case."""
import io
import zlib

import numpy as np
import pytest

PIL = pytest.importorskip("PIL.Image")

import deflate_writer as dw   # noqa: E402


def _fam(f):
    return [c for c in dw.corpus() if c.family == f]


def _named(name):
    return next(c for c in dw.corpus() if c.name == name)


def _pillow(c):
    im = PIL.open(io.BytesIO(c.png))
    im.load()
    if im.mode == "P":
        im = im.convert("RGB")
    elif im.mode == "LA":
        im = im.getchannel("L")
    return np.asarray(im)


# Pillow stops reading when the last row is complete: it opens these four, whose streams go on (or stop) behind the image's last
# byte.  zlib is their judge: three inflate to another length than the image's, one ends without a final block.
PILLOW_LENIENT = {"f4_inflates_to_raw_n_plus_1", "f4_inflates_to_raw_n_plus_257", "f4_inflates_to_3_raw_n", "f4_ends_after_non_final_block"}


def test_valid_streams_inflate_everywhere_to_the_writers_bytes(oracle):
    n = 0
    for c in dw.corpus():
        if c.status != dw.OK:
            continue
        n += 1
        assert zlib.decompress(c.z) == c.raw, c.name
        assert oracle.inflate(c.z, len(c.raw)) == (0, c.raw), c.name
        assert np.array_equal(_pillow(c), c.pixels), c.name
        rc, px = oracle.png_decode(c.png)
        assert rc == oracle.PNG_OK and np.array_equal(px, c.pixels), c.name
    assert n >= 150


def test_invalid_streams_are_refused_everywhere(oracle):
    seen = set()
    for c in dw.corpus():
        if c.status == dw.OK:
            continue
        seen.add(c.name)
        if c.family == "F4" and c.why == "length":
            assert len(zlib.decompress(c.z)) != dw.RAW_N, c.name          # a sound stream of the wrong length
        elif c.family == "F5":
            assert zlib.decompress(c.z) == c.raw                           # the stream is sound: a row's filter type is not
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(c.z)
        if c.name in PILLOW_LENIENT:
            assert _pillow(c).shape == (256, 255), c.name
        else:
            with pytest.raises((OSError, SyntaxError, ValueError)):
                _pillow(c)
        rc, _ = oracle.png_decode(c.png)
        if c.family == "F5":
            assert rc == oracle.PNG_CORRUPT, c.name
        else:
            assert rc == (oracle.PNG_NEEDS_HOST if c.status == dw.NEEDS_HOST else oracle.PNG_CORRUPT), (c.name, rc)
            rc, _ = oracle.inflate(c.z, 4 * dw.RAW_N)
            if c.why != "length":
                assert rc == (oracle.PNG_NEEDS_HOST if c.status == dw.NEEDS_HOST else oracle.PNG_CORRUPT), (c.name, rc)
    assert PILLOW_LENIENT <= seen
    want = ["btype3", "len_nlen", "stored_len_beyond_input", "hlit_field_30", "hlit_field_31", "hdist_31", "hdist_32", "cl_incomplete",
            "cl_over", "cl_first16", "cl_overrun", "no_eob_code", "ll_over_subscribed", "ll_incomplete_two_codes", "dist_over_subscribed",
            "dist_incomplete_two_codes", "unassigned_code_lone_dist", "unassigned_code_lone_ll", "match_without_dist_codes",
            "fixed_sym286", "fixed_sym287", "fixed_dist30", "fixed_dist31", "dist_beyond_start_first", "dist_beyond_start_after5",
            "inflates_to_raw_n_plus_1", "inflates_to_raw_n_plus_257", "inflates_to_3_raw_n", "inflates_to_raw_n_minus_1",
            "ends_mid_symbol", "ends_after_non_final_block", "lone_ll_code_2_bit", "lone_ll_code_15_bit", "lone_dist_code_2_bit",
            "lone_dist_code_15_bit", "dist_beyond_start_then_lone_code"]
    assert {"f4_" + w for w in want} <= seen


def test_lone_codes_go_to_the_host_and_their_one_bit_twins_decode(oracle):
    """zlib takes an incomplete code of one symbol only when that code is one bit long (inftrees.c); inflaters that follow RFC 1951's
    wording take any length.  Decoders disagree, so the verdict is the host decoder's (DESIGN P5): PNG_NEEDS_HOST, neither pixels
    nor a rejection."""
    for kind in ("ll", "dist"):
        twin = _named(f"f4_lone_{kind}_code_1_bit")
        assert twin.status == dw.OK and zlib.decompress(twin.z) == twin.raw and oracle.png_decode(twin.png)[0] == oracle.PNG_OK
        for bits in (2, 15):
            c = _named(f"f4_lone_{kind}_code_{bits}_bit")
            with pytest.raises(zlib.error, match="invalid literal/lengths set" if kind == "ll" else "invalid distances set"):
                zlib.decompress(c.z)
            assert oracle.png_decode(c.png)[0] == oracle.PNG_NEEDS_HOST
            assert oracle.inflate(c.z, dw.RAW_N)[0] == oracle.PNG_NEEDS_HOST
            blk = next(b for b in c.stream.blocks if b["kind"] == "dynamic")
            code = blk["ll"] if kind == "ll" else blk["dd"]
            assert sorted(l for l in code if l) == [bits]


def test_f1_long_codes_fall_on_every_kind_of_symbol():
    ladders = [c for c in _fam("F1") if "ladder" in c.name]
    assert len(ladders) >= 4
    long_ll, long_d = set(), set()
    for c in ladders:
        (blk,) = c.stream.blocks
        ll, dd = c.info["ll"], c.info["dd"]
        assert sorted(ll.values()) == sorted(dd.values()) == list(range(1, 16)) + [15]
        used_ll = {t[2] for t in blk["tokens"]} | {256}
        used_d = {t[3] for t in blk["tokens"] if t[3] is not None}
        assert used_ll == set(ll) and used_d == set(dd), c.name            # every coded symbol occurs
        long_ll |= {s for s in ll if ll[s] >= 11}
        long_d |= {s for s in dd if dd[s] >= 11}
    assert {0, 1, 2, 3, 128, 255, 257, 264, 265, 284, 285} <= long_ll      # plain literals; lengths without, with 1 and with 5 extra bits
    assert {0, 3, 4, 28, 29} <= long_d                                     # no, 1 and 13 extra bits
    for c in [x for x in ladders if x.geom is dw.GRAY] + [_named("f1_wide")]:
        toks = [t for b in c.stream.blocks for t in b["tokens"]]
        assert any(t[2] == 284 and t[5] == 258 for t in toks), c.name      # 258 as 284 + 31 ...
        assert any(t[2] == 285 and t[5] == 258 for t in toks) or c.name == "f1_wide", c.name      # ... and as 285
        assert any(t[6] == 32768 for t in toks), c.name


def test_f1_wide_block_is_wide_at_every_bit_phase():
    c = _named("f1_wide")
    st, blk = c.stream.blocks
    assert st["kind"] == "stored" and st["end_bit"] - st["sym_bit"] >= 24577 * 8
    nbits = blk["end_bit"] - blk["sym_bit"]
    assert nbits >= 524288                                                 # four rounds of the widest shape: 4 waves x 64 x 512 bits
    wide = [t for t in blk["tokens"] if t[1] >= 40]
    assert all(43 <= t[1] <= 48 for t in wide) and {t[1] for t in wide} == {43, 48}
    widest = [t for t in wide if t[1] == 48]                               # 15 + 5 + 15 + 13: nothing in deflate is wider
    assert len(widest) >= 17 and len({t[0] % 32 for t in widest}) >= 16    # ... at 16 evenly spaced bit phases
    assert sum(t[1] for t in wide) * 4 >= nbits * 3
    assert {t[0] % 32 for t in wide} == set(range(32))
    assert all(16385 <= t[6] <= 32768 for t in wide)
    assert any(t[1] == 1 and t[2] < 256 for t in blk["tokens"])            # the one-bit literals between them


def test_f2_blocks_begin_at_every_bit_phase_and_come_in_every_kind():
    seams = [c for c in _fam("F2") if "seams" in c.name]
    phases = {"stored": set(), "fixed": set(), "dynamic": set()}
    for c in seams:
        blocks = c.stream.blocks
        assert len(blocks) >= (200 if c.geom is dw.GRAY else 100), (c.name, len(blocks))
        assert {b["kind"] for b in blocks} == set(phases)
        assert all(len(b["tokens"]) <= 40 for b in blocks)
        early = [len(b["tokens"]) for b in blocks if not b.get("empty_run") and b["out0"] < len(c.raw) // 4 and b["kind"] != "stored"]
        assert min(early) < 10 and max(early) > 30 and sum(1 for n in early if n < 20) >= 5, c.name       # 0 .. 40 from the start on
        for b in blocks + _named("f2_phases").stream.blocks:
            if not b.get("empty_run"):
                continue
            assert b["end_bit"] == b["sym_bit"] if b["kind"] == "stored" else not b["tokens"]
            phases[b["kind"]].add(b["bit"] % 32)
            if b["kind"] == "dynamic":
                assert [l for l in b["ll"] if l] == [1] and not any(b["dd"])       # only end-of-block, as a one-bit code
        full = next(i for i, b in enumerate(blocks) if b["out0"] == len(c.raw))
        assert len(blocks) - full >= 7 and blocks[-1]["final"] and not any(b["final"] for b in blocks[:-1])
        assert {b["kind"] for b in blocks[full:-1]} == set(phases)                 # empty blocks behind the last output byte
    for kind, got in phases.items():
        assert got == set(range(32)), (kind, sorted(set(range(32)) - got))


def test_f2_stored_sizes_and_padding():
    c = _named("f2_stored_small")
    st = [b for b in c.stream.blocks if b["kind"] == "stored"]
    assert {1, 2, 3} <= {(b["end_bit"] - b["sym_bit"]) // 8 for b in st}
    after = [b for b in st if "after_phase" in b]
    assert {b["after_phase"] for b in after} == set(range(8))
    assert sum(b["pad_ones"] for b in after) == 4
    big = _named("f2_stored_65535").stream.blocks[-1]
    assert big["kind"] == "stored" and big["end_bit"] - big["sym_bit"] == 65535 * 8


def test_f2_header_codings():
    c = _named("f2_headers")
    tag = {b["tag"]: b for b in c.stream.blocks if "tag" in b}

    def spans(b):
        out, i = [], 0
        for s, rep in b["cl_syms"]:
            n = rep if s >= 16 else 1
            out.append((s, i, i + n))
            i += n
        assert i == b["hlit"] + b["hdist"]
        return out
    b = tag["rep16_crosses"]
    assert any(s == 16 and lo < b["hlit"] < hi for s, lo, hi in spans(b))          # the repeat runs on into the distance lengths
    b = tag["rep18_138_rep17_ends"]
    sp = spans(b)
    assert (18, 138) in [(s, hi - lo) for s, lo, hi in sp] and sp[-1][0] == 17 and sp[-1][2] - sp[-1][1] == 3
    b = tag["hlit286_hdist30"]
    assert b["hlit"] == 286 and b["hdist"] == 30 and b["ll"][285] and any(t[2] == 285 for t in b["tokens"])
    assert any(t[3] == 29 for t in b["tokens"])
    b = tag["hclen19"]
    assert b["hclen"] == 19 and max(b["cl_lens"]) == 7 and all(b["cl_lens"])
    b = tag["hclen_min_no_dist"]
    assert b["hclen"] == 5 and {l for l in b["ll"] if l} == {8} and not any(b["dd"])
    assert all(t[2] < 256 for t in b["tokens"])
    b = tag["one_dist_code"]
    assert [l for l in b["dd"] if l] == [1] and any(t[3] is not None for t in b["tokens"])


def test_f3_every_path_meets_every_alignment():
    c = _named("f3_geometry")
    placed = c.info["placed"]
    have = {(n, d) for n, d, _ in placed}
    for n in dw.F3_LENS:
        for d in dw.F3_SMALL + [n - 1, n, n + 1] + list(range(2040, 2057)) + list(range(8184, 8201)) + [32767, 32768]:
            assert (n, d) in have, (n, d)
    for path in ("coop", "window", "far"):
        mine = [(n, d, p) for n, d, p in placed if dw.match_path(n, d) == path]
        assert {p % 4 for _, _, p in mine} == {0, 1, 2, 3}, path
        assert {(p - d) % 4 for _, d, p in mine} == {0, 1, 2, 3}, path
    toks = [t for b in c.stream.blocks for t in b["tokens"]]
    assert sum(1 for t in toks if t[6] and t[6] == t[4] - t[5]) >= 4               # distance = the bytes produced so far
    # sources that straddle the window base: the base lies 2048 .. 2051 bytes below a round's first byte, wherever rounds fall;
    # distances 2040 .. 2056 at every length put sources on both sides of it and across it
    assert sum(1 for n, d, _ in placed if 2040 <= d <= 2056 and n >= 9) >= 5 * 17


def test_f3_match_words_fall_on_every_seam_position():
    runs = [c for c in _fam("F3") if "runs" in c.name]
    assert len(runs) == 34
    lane_pos, all_heads = set(), set()
    for c in runs:
        heads = dw.token_words(c.stream)
        lane_pos |= {h % dw.kLaneWords for h in heads}
        all_heads |= set(heads)
        toks = [t for b in c.stream.blocks for t in b["tokens"] if t[2] > 256]
        # the first round takes all 2048 words (its output stays below 8192 bytes), so the round seam is where the count says
        first = [t for t, h in zip(toks, heads) if h < dw.kRoundWords]
        assert first[-1][4] <= dw.kRoundBytes
        dists = [t[6] for t in toks]
        lens = [t[5] for t in toks]
        assert lens[:40] == [258] * 40 and dists[:40] == [256, 512] * 20          # alternating: 16 to a lane, never merged
        got = set()
        i = 40
        while i < len(toks) and len(got) < 12:
            j = i
            while j < len(toks) and (lens[j], dists[j]) == (lens[i], dists[i]) and (j == i or toks[j][0] == toks[j - 1][0] + toks[j - 1][1]):
                j += 1
            got.add((j - i, lens[i], dists[i]))
            i = j
        assert {(r, n, d) for r in (2, 16, 17, 100) for n, d in ((3, 3), (258, 1), (4, 256))} <= got
    assert lane_pos == set(range(32))                      # 31: the head in a lane's last word, its distance in the next lane's first
    assert {2046, 2047, 2048} <= all_heads                 # ... and the same at the round seam
    two = _named("f3_two_bit")
    assert sum(1 for t in two.stream.blocks[0]["tokens"] if t[1] == 2 and t[5] == 258) == 254 and not any(two.raw)


def test_f5_rows_sizes_and_layouts():
    f5 = _fam("F5")
    for lname, *_ in dw.F5_LAYOUTS:
        mine = [c for c in f5 if c.layout == lname and c.status == dw.OK]
        assert {c.h for c in mine} >= set(dw.F5_SIZES) and {c.w for c in mine} >= set(dw.F5_SIZES)
        for t in range(5):
            assert any(c.h == 129 and all(c.ftypes[r] == t for r in (0, 63, 64, 65, 127, 128)) and len(set(c.ftypes)) > 1 for c in mine)
            assert any(set(c.ftypes) == {t} for c in mine)
    bad = [c for c in f5 if c.status != dw.OK]
    assert {(int(c.ftypes[r]), r) for c in bad for r in range(129) if c.ftypes[r] > 4} == {(b, r) for b in (5, 255) for r in (0, 1, 70, 128)}


def test_batches_put_every_refused_file_between_two_valid_ones():
    for key, order in dw.batches([c.light() for c in dw.corpus()]).items():
        for i, c in enumerate(order):
            if c["status"] != dw.OK:
                a, b = order[i - 1], order[i + 1]
                assert i > 0 and a["status"] == b["status"] == dw.OK and not np.array_equal(a["pixels"], b["pixels"]), c["name"]
