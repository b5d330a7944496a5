"""GPU parity of the JPEG front end (ucfp_amd/csrc/jpeg.hip) on the files of tests/test_jpeg_layouts_spec.py -- sampling
layouts, table ids, header orders and Huffman tables that no encoder at hand writes (tests/jpeg_writer.py makes them from
coefficients).  For every file: the device's status is the oracle's; where that is 0 the plane is bit-equal to the oracle's
AND to libjpeg's; the probe reads the frame header.  Every batch goes through `decode_jpegs` (one announced geometry), the
mixed-geometry corpora also through `decode_uploads` (the ragged path).  Which kernel a file takes -- speculative, serial
lane, lane per restart interval; 1, 2, 4 or 8 waves -- is computed from the writer's facts by the rules restated in the spec
module, and test_jpeg_layouts_spec.py asserts that the corpora reach every one of them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
pytest.importorskip("PIL.Image")

from test_jpeg_layouts_spec import (check_against_libjpeg, corpus_headers, corpus_layouts, corpus_long_codes,   # noqa: E402
                                    corpus_unstuffer, corpus_waves, eoi_opens_step, ff_straddles_step, judged,
                                    rst_after_stuffed_pair_straddles_step, rst_straddles_step, spec_waves, takes_spec,
                                    SPEC_MAX_BLOCKS, SPEC_MIN_BYTES, WAVE_LANES, max_seg)


def _check(oracle, cases, frames, status):
    """Device results of `cases` against the oracle's and libjpeg's; -> files decoded."""
    from ucfp_amd import image
    n = 0
    for c, fr, st in zip(cases, frames, status):
        check_against_libjpeg(oracle, c)                      # (cached: the CPU test's verdict, the class the file is in)
        rc, px, lj = judged(oracle, c)
        assert int(st) == rc, "%s: device status %d, oracle %d" % (c.name, st, rc)
        assert image.jpeg_probe(c.f.data) == (0, c.f.w, c.f.h), c.name
        if rc == 0:
            assert fr is not None and fr.shape == px.shape, c.name
            assert np.array_equal(fr, px), "%s: %d pixels differ from the oracle's" % (c.name, int((fr != px).sum()))
            assert np.array_equal(fr, lj), c.name
            n += 1
    return n


def decode_uniform(gpu_ctx, oracle, cases):
    """One `decode_jpegs` batch per geometry; -> files decoded."""
    from ucfp_amd import image
    groups = {}
    for c in cases:
        groups.setdefault((c.f.w, c.f.h), []).append(c)
    n = 0
    for (w, h), group in groups.items():
        frames, status = image.decode_jpegs([c.f.data for c in group], w, h, ctx=gpu_ctx)
        assert len(status) == len(group)
        n += _check(oracle, group, frames, status)
    return n


def decode_ragged(gpu_ctx, oracle, cases):
    """All of `cases`, whatever their geometries, in one `decode_uploads` batch; -> files decoded."""
    from ucfp_amd import image
    frames, status = image.decode_uploads([c.f.data for c in cases], ctx=gpu_ctx)
    assert len(frames) == len(status) == len(cases)
    return _check(oracle, cases, frames, status)


def test_sampling_layouts_on_every_decoder_path(gpu_ctx, oracle):
    """4:1:1, 4:4:0, 3x1, 7-, 8- and 10-block MCUs, every component 2x1, one component declared 2x2 and 1x1; 1 x 1 to
    160 x 128; restart intervals 0, 1, 3, one MCU row, more than the MCU count, and the one that gives 64 segments."""
    cases = corpus_layouts()
    files = [c.f for c in cases]
    # the paths (the spec module's coverage test has the full list)
    assert any(takes_spec(f) and f.blocks_per_mcu == SPEC_MAX_BLOCKS for f in files)
    assert any(f.n_seg == 1 and f.blocks_per_mcu > SPEC_MAX_BLOCKS for f in files)
    assert any(f.n_seg == 1 and f.restart == 0 and f.clean_len < SPEC_MIN_BYTES for f in files)
    assert any(f.n_seg > WAVE_LANES for f in files) and any(f.n_seg == WAVE_LANES for f in files)
    assert any(f.ncomp == 1 and f.restart == 1 and f.n_seg == max_seg(f.w, f.h) > 1 for f in files)
    assert decode_uniform(gpu_ctx, oracle, cases) == len(cases)
    assert decode_ragged(gpu_ctx, oracle, cases) == len(cases)


@pytest.mark.parametrize("nw", [2, 4, 8])
def test_new_layouts_on_several_waves(gpu_ctx, oracle, nw):
    """Batches of 8 files of 4:1:1, 4:4:0 and all-2x1 sampling whose mean size makes launch_jpeg_decode run the speculative
    kernel with 2, 4 and 8 waves per file: block scans and the chain walk cross waves."""
    seen = 0
    for (samp, want), cases in corpus_waves().items():
        if want != nw:
            continue
        files = [c.f for c in cases]
        assert all(takes_spec(f) for f in files) and spec_waves(files) == nw, (samp, spec_waves(files))
        assert decode_uniform(gpu_ctx, oracle, cases) == len(cases) == 8
        seen += 1
    assert seen == 3


def test_header_variants(gpu_ctx, oracle):
    """SOF1, table ids up to 3, tables in one segment or one each, fill bytes, DRI in front of SOF, 65 533-byte COM / APPn
    segments, component ids without JFIF, Adobe; RGB-coded, luma below the MCU and more than 10 blocks per MCU: the host."""
    cases = corpus_headers()
    want = sum(c.expect == "decode" for c in cases)
    assert 0 < want < len(cases)
    assert decode_uniform(gpu_ctx, oracle, cases) == want
    assert decode_ragged(gpu_ctx, oracle, cases) == want


def test_codes_of_10_to_16_bits(gpu_ctx, oracle):
    """Comb tables: most coded symbols are longer than the 9-bit look-ahead table and take the maxcode / valoff search."""
    cases = corpus_long_codes()
    for c in cases:
        hist = c.f.code_len_hist
        assert 2 * hist[10:].sum() >= hist.sum() and hist[16] > 0, (c.name, hist)
    assert any(takes_spec(c.f) for c in cases) and any(c.f.n_seg > 1 for c in cases) and any(c.f.ncomp == 1 for c in cases)
    assert decode_uniform(gpu_ctx, oracle, cases) == len(cases)
    assert decode_ragged(gpu_ctx, oracle, cases) == len(cases)


def test_unstuffer_step_boundaries(gpu_ctx, oracle):
    """jpeg_scan_kernel's 64-byte steps: a stuffed FF 00 and an RSTn marker cut by a step, a marker cut right behind a
    stuffed pair, EOI opening a step."""
    cases = corpus_unstuffer()
    assert ff_straddles_step(cases["ff"].f) and ff_straddles_step(cases["ff-1comp"].f)
    assert rst_straddles_step(cases["rst"].f) and rst_after_stuffed_pair_straddles_step(cases["rst-pair"].f)
    assert eoi_opens_step(cases["eoi"].f) and eoi_opens_step(cases["eoi-rst"].f)
    assert decode_uniform(gpu_ctx, oracle, list(cases.values())) == len(cases)
    assert decode_ragged(gpu_ctx, oracle, list(cases.values())) == len(cases)
