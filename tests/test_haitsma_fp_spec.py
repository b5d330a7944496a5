"""The C oracle's Haitsma sub-fingerprints (steps A7 and A8 of audio.hip) against the float64 restatement in tests/haitsma_fp_ref.py.

The oracle is what every GPU test compares the HIP kernels with bit for bit, and its band edges, band sums and bit rule
are restated line by line in the HIP code: this module is the statement of them that shares no line with either."""
import numpy as np
import pytest

import haitsma_fp_ref as hr

CONFIGS = [(300.0, 2000.0), (1.0, 2500.0), (1.0, 40.0), (60.0, 2500.0), (2400.0, 2500.0)]
ON_BINS = (5000.0 / 2048.0 * 100.0, 5000.0 / 2048.0 * 133.0)      # both exact in float32: bins 100 and 133 exactly
MARGIN = 1e-5       # float32 band sums of <= 1024 terms and two differences: the error of dd stays far below 1e-5 * scale


def _signal(kind):
    rng = np.random.default_rng(77)
    n = 8 * 5000
    if kind == "noise":
        return (0.2 * rng.standard_normal(n)).astype(np.float32)
    t = np.arange(n) / 5000.0
    x = 0.3 * np.sin(2 * np.pi * (100.0 * t + 0.5 * (2300.0 / 8.0) * t * t)) + 0.02 * rng.standard_normal(n)
    return x.astype(np.float32)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]:g}-{c[1]:g}")
@pytest.mark.parametrize("kind", ["noise", "chirp"])
def test_bits_follow_the_float64_restatement(oracle, kind, cfg):
    """Every bit of oracle.haitsma: 0 where both bands are empty (scale == 0); equal to dd > 0 where |dd| > 1e-5 * scale;
    left out otherwise, and at most 1 % of the bits with a non-zero scale may be left out.

    Shares left out at 1e-5, in % of the bits with a non-zero scale (no checked bit disagreed):

        fmin, fmax      noise    chirp
        300, 2000       0.0316   0.0421
        1, 2500         0.0464   0.0987
        1, 40           0.0000   0.0000
        60, 2500        0.0473   0.0421
        2400, 2500      0.0210   0.0316
    """
    x = _signal(kind)
    got = hr.unpack_bits(oracle.haitsma(x, 5000, *cfg))
    dd, scale = hr.haitsma_bits64(x, *cfg)
    assert got.shape == dd.shape == (1 + (x.size - 2048) // 64, 32)
    live = scale > 0
    assert not got[~live].any()
    sure = live & (np.abs(dd) > MARGIN * scale)
    left_out = 1.0 - sure.sum() / live.sum()
    print(f"{kind} {cfg}: {live.sum()} bits with scale > 0, left out {100 * left_out:.4f} %, "
          f"wrong {(got[sure] != (dd[sure] > 0)).sum()}")
    assert np.array_equal(got[sure], dd[sure] > 0)
    assert left_out <= 0.01
    if cfg == (1.0, 40.0):
        assert (~live).sum() > 0            # this configuration has neighbouring empty bands


@pytest.mark.parametrize("cfg,first,last", [((300.0, 2000.0), 123, 820), ((1.0, 2500.0), 1, 1024), ((1.0, 40.0), None, None),
                                            ((60.0, 2500.0), None, None), ((2400.0, 2500.0), 984, 1024),
                                            (ON_BINS, 100, 133)])
def test_edges(oracle, cfg, first, last):
    e = hr.edges64(*cfg)
    assert np.array_equal(oracle.haitsma_edges(*cfg).astype(np.int64), e)
    assert (np.diff(e) >= 0).all() and e[-1] <= 1024
    if first is not None:
        assert (e[0], e[-1]) == (first, last)        # ON_BINS: ceil of an exact integer does not move up


def test_edge_configurations_cover_the_corners():
    """What the configurations are chosen for: empty bands, a band longer than 8 * 26 bins, the clamp at bin 1024."""
    assert (np.diff(hr.edges64(1.0, 40.0)) == 0).sum() >= 10
    assert np.diff(hr.edges64(1.0, 2500.0)).max() == 216
    assert hr.edges64(60.0, 2500.0)[-1] == 1024 and hr.edges64(2400.0, 2500.0)[-1] == 1024
    assert (hr.edges64(1.0, 2.0) == 1).all() and (hr.edges64(2499.0, 2500.0) == 1024).all()


def test_prefix_property(oracle):
    """Frame t depends on the samples of frames t - 1 and t alone: the frames of a prefix are a prefix of the frames."""
    x = _signal("noise")
    full = oracle.haitsma(x, 5000)
    for F in (1, 2, 7, 8, 9, 100, full.size - 1, full.size):
        assert np.array_equal(oracle.haitsma(x[:2048 + 64 * (F - 1)], 5000), full[:F]), F
    assert oracle.haitsma(x[:2047], 5000).size == 0


def test_frame_counts(oracle):
    """ucfp_audio_haitsma_frames (a host function of the library) against the count from the definitions: floor(n * 5000 /
    sr) samples at 5 kHz, one frame per 64 of them from 2048 on."""
    from ucfp_amd import _lib
    lib = _lib.load()

    def frames(n, sr):
        n5 = n if sr == 5000 else n * 5000 // sr
        return 1 + (n5 - 2048) // 64 if n5 >= 2048 else 0

    x = np.zeros(2200, np.float32)
    for n in (0, 1, 2047, 2048, 2049, 2111, 2112, 2113, 2175, 2176):
        assert lib.ucfp_audio_haitsma_frames(n, 5000) == oracle.haitsma(x[:n], 5000).size == frames(n, 5000), n
    assert [frames(n, 5000) for n in (2047, 2048, 2111, 2112)] == [0, 1, 1, 2]
    for sr in (1000, 4999, 5001, 44100, 384000):
        one = -(-2048 * sr // 5000)                 # the shortest input with a frame
        two = -(-2112 * sr // 5000)
        assert frames(one - 1, sr) == 0 and frames(one, sr) == 1 and frames(two - 1, sr) == 1 and frames(two, sr) == 2
        z = np.zeros(two + 1, np.float32)
        for n in (0, 1, one - 1, one, one + 1, two - 1, two, two + 1):
            assert lib.ucfp_audio_haitsma_frames(n, sr) == oracle.haitsma(z[:n], sr).size == frames(n, sr), (sr, n)
