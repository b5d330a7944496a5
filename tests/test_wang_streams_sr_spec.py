"""Wang / Panako streams at any sample rate on the CPU: S(n) restated in Python against
ucfp_wang_stream_samples, the prefix soundness the contract stands on against the oracle, the carried-input bound by a
stateful restatement (tests/wang_stream_sr_ref.py), and the host-side argument checks of the _sr entries."""
import ctypes as C

import numpy as np
import pytest

import wang_stream_sr_ref as sr_ref
from ucfp_amd import _lib
from wang_stream_sr_ref import RATES, final_samples

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4


def _wcfg(zone_t=63, pps=30, fan_out=10, zone_f=64, db=-50.0):
    return _lib.WangConfig(fan_out, zone_t, zone_f, pps, db)


def _pcfg(zone_t=96, pps=30, fan_out=5, zone_f=96, db=-50.0):
    return _lib.PanakoConfig(fan_out, zone_t, zone_f, pps, db)


def _first_n_with(sr, s8):
    """The least n with S(n) >= s8 (S is monotone)."""
    lo, hi = 0, (s8 + 2) * sr // 8000 + 4
    while lo < hi:
        mid = (lo + hi) // 2
        if final_samples(mid, sr) >= s8:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _feed(sr, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    x = 0.1 * rng.standard_normal(n)
    for f in (310.0, 941.0, 2210.0):
        x += 0.2 * np.sin(2 * np.pi * f * t * (1 + 0.1 * t / seconds))
    return x.astype(np.float32)


def test_samples_match_the_rule():
    lib = _lib.load()
    for sr in RATES:
        ns = set(range(200))
        for j in (0, 1, 7, 55, 63, 500):                # bands around the n at which frame j completes
            b = _first_n_with(sr, 1024 + 128 * j)
            ns |= set(range(max(0, b - 3 - sr // 8000), b + 4 + sr // 8000))
        prev = 0
        for n in sorted(ns):
            s, sf = lib.ucfp_wang_stream_samples(n, sr, 0), lib.ucfp_wang_stream_samples(n, sr, 1)
            assert s == final_samples(n, sr) and sf == final_samples(n, sr, True), (sr, n)
            assert prev <= s <= sf, (sr, n)             # monotone; the non-final value never exceeds the final one
            assert sf == n * 8000 // sr
            prev = s
        # monotone sample by sample, and a sample later the offline length of now is final
        vals = [lib.ucfp_wang_stream_samples(n, sr, 0) for n in range(0, 3 * (sr // 8000 + 2) + 400)]
        assert all(a <= b for a, b in zip(vals, vals[1:]))
    for sr in (0, 999, 384001):
        for fin in (0, 1):
            assert lib.ucfp_wang_stream_samples(5 * sr + 12345, sr, fin) == 0
    assert lib.ucfp_wang_stream_samples(12345, 8000, 0) == 12345 == lib.ucfp_wang_stream_samples(12345, 8000, 1)


def test_the_cap_matters():
    """A18's cap example transposed: where ceil((n - 1) 8000 / sr) exceeds floor(n 8000 / sr), the offline length wins."""
    lib = _lib.load()
    found = None
    for sr in RATES:
        for n in range(1, 200):
            if sr != 8000 and -(-(n - 1) * 8000 // sr) > n * 8000 // sr:
                found = found or (sr, n)
    assert found == (11025, 4)
    assert -(-3 * 8000 // 11025) == 3 and 4 * 8000 // 11025 == 2
    assert lib.ucfp_wang_stream_samples(4, 11025, 0) == 2 == lib.ucfp_wang_stream_samples(4, 11025, 1)
    assert lib.ucfp_wang_stream_samples(2, 44100, 0) == 0       # ceil(0.18) = 1 > floor(0.36) = 0


@pytest.mark.parametrize("sr", RATES)
def test_prefix_soundness_against_the_oracle(oracle, sr):
    """The first S(n) samples of the resampled prefix x[:n] are those of the resampled feed, bit for bit, and so are
    the hashes below frontier(S(n)): what a stream holds after n input samples is final."""
    lib = _lib.load()
    x = _feed(sr, 3.2, sr)
    n_all = x.size
    full = oracle.resample_linear(x, sr, 8000)
    assert full.size == n_all * 8000 // sr
    hashes = oracle.wang(full)
    cuts = {0, 1, 2, n_all - 1, n_all, int(2.3 * sr), int(2.3 * sr) + 1, int(3.1 * sr)}
    for j in (0, 1, 7):
        b = _first_n_with(sr, 1024 + 128 * j)
        cuts |= set(range(b - 2, b + 3))
    moved = 0
    for n in sorted(cuts):
        s = lib.ucfp_wang_stream_samples(n, sr, 0)
        pre = oracle.resample_linear(x[:n], sr, 8000) if n else np.zeros(0, np.float32)
        assert s <= pre.size
        assert np.array_equal(pre[:s].view(np.uint32), full[:s].view(np.uint32)), (sr, n)
        F = lib.ucfp_wang_stream_frontier(s, None)
        a = oracle.wang(pre[:s]) if s else np.zeros((0, 2), np.uint32)
        assert np.array_equal(a[a[:, 1] < F], hashes[hashes[:, 1] < F]), (sr, n)
        moved += F > 0
    assert moved >= 2 and hashes.shape[0] > 50
    # the final count is the offline length
    assert lib.ucfp_wang_stream_samples(n_all, sr, 1) == full.size


def _cuttings(rng, n, sr):
    k = -(-sr // 8000)
    sizes = (0, 1, 2, 7, k - 1, k, k + 1, 997, sr // 2, sr)
    out, a = [], 0
    while a < n:
        c = int(rng.choice(sizes)) if rng.random() < 0.85 else int(rng.integers(0, 3 * sr))
        out.append(min(max(c, 0), n - a))
        a += out[-1]
    return out


@pytest.mark.parametrize("sr", RATES)
def test_carried_inputs_are_enough(oracle, sr):
    """A stream that keeps only ceil(sr / 8000) + 1 inputs between chunks assembles oracle.resample_linear of the whole
    feed, whatever the cutting (the restatement asserts the bound after every push)."""
    rng = np.random.default_rng(sr + 1)
    x = _feed(sr, 1.4, sr + 7)
    full = oracle.resample_linear(x, sr, 8000) if sr != 8000 else x
    ones = [1] * min(x.size, 3 * (sr // 8000 + 2) + 40)
    for case in range(6):
        chunks = _cuttings(rng, x.size, sr) if case else ones + [0, 0, x.size - len(ones)]
        for final_carries in (False, True):
            got = sr_ref.run_stream(x, sr, chunks, final_carries)
            assert np.array_equal(got.view(np.uint32), full.view(np.uint32)), (sr, case, final_carries)
    for m in (0, 1, 2):                                 # feeds too short for an output
        assert sr_ref.run_stream(x[:m], sr, [1] * m).size == m * 8000 // sr


def test_create_checks_need_no_gpu():
    lib = _lib.load()
    h = C.c_void_p()
    # the old entries still take 8 kHz only
    for sr in (16000, 44100):
        assert lib.ucfp_wang_streams_create(None, sr, None, 4, C.byref(h)) == UCFP_E_MODALITY
        assert b"resample upstream" in lib.ucfp_last_error()
        assert lib.ucfp_wang_streams_create_ex(None, sr, None, 4, 63, C.byref(h)) == UCFP_E_MODALITY
        assert lib.ucfp_panako_streams_create(None, sr, None, 4, 63, C.byref(h)) == UCFP_E_MODALITY
        assert b"resample upstream" in lib.ucfp_last_error()
    for create, cfg in ((lib.ucfp_wang_streams_create_sr, _wcfg), (lib.ucfp_panako_streams_create_sr, _pcfg)):
        for sr in (0, 999, 384001, 1 << 31):
            assert create(None, sr, None, 4, 0, C.byref(h)) == UCFP_E_MODALITY
            assert b"sample rate" in lib.ucfp_last_error()
        for sr in (1000, 8000, 44100, 384000):
            for bad in (cfg(zone_t=0), cfg(zone_t=513), cfg(pps=0), cfg(pps=257), cfg(fan_out=65), cfg(zone_f=1025)):
                assert create(None, sr, C.byref(bad), 4, 0, C.byref(h)) == UCFP_E_MODALITY
            # the rate and the config are in range: a NULL context is the next complaint, then the sizes
            assert create(None, sr, None, 4, 0, C.byref(h)) == UCFP_E_INVALID
            assert b"ctx" in lib.ucfp_last_error()
            assert create(None, sr, None, 4, 8193, C.byref(h)) == UCFP_E_INVALID
    assert not h.value


def test_window_above_the_maximum_and_null_sets():
    lib = _lib.load()
    ctx = C.c_void_p(1)                      # never dereferenced: the window is judged before the device is asked for
    h = C.c_void_p()
    for create in (lib.ucfp_wang_streams_create_sr, lib.ucfp_panako_streams_create_sr):
        assert create(ctx, 44100, None, 4, 8193, C.byref(h)) == UCFP_E_INVALID
        assert b"window_frames" in lib.ucfp_last_error() and not h.value
        assert create(ctx, 44100, None, 0, 63, C.byref(h)) == UCFP_E_INVALID
        assert b"max_streams" in lib.ucfp_last_error() and not h.value
        assert create(ctx, 44100, None, 4, 63, None) == UCFP_E_INVALID
    # a NULL set: status codes, no crash, as for the sets of the 8 kHz entries
    slot, n = C.c_uint32(0), C.c_size_t(0)
    for abi in ("wang", "panako"):
        fn = lambda name: getattr(lib, f"ucfp_{abi}_streams_{name}")
        assert fn("open")(None, C.byref(slot)) == UCFP_E_INVALID
        assert fn("close")(None, 0) == UCFP_E_INVALID
        assert fn("max_hashes")(None, None, None, None, 0) == 0
        assert fn("push")(None, 0, None, 0, 1, None, 0, C.byref(n)) == UCFP_E_INVALID
        assert fn("push_dev")(None, None, None, None, 0, None, None, 0, None, None) == UCFP_E_INVALID
        assert fn("windows_dev")(None, None, 0, None, 0, None, None, None) == UCFP_E_INVALID
        fn("destroy")(None)


def test_state_bytes_follow_the_formula():
    lib = _lib.load()
    for W in (0, 63, 8192):
        for wc, pc in ((None, None), (C.byref(_wcfg(zone_t=512, pps=256)), C.byref(_pcfg(zone_t=512, pps=256)))):
            w8, p8 = lib.ucfp_wang_streams_state_bytes_ex(wc, W), lib.ucfp_panako_streams_state_bytes(pc, W)
            assert w8 > 0 and p8 > 0
            assert lib.ucfp_wang_streams_state_bytes_sr(wc, W, 8000) == w8
            assert lib.ucfp_panako_streams_state_bytes_sr(pc, W, 8000) == p8
            for sr in RATES + (1001, 8000 * 3, 8000 * 3 + 1):
                extra = 0 if sr == 8000 else 4 * (-(-sr // 8000) + 1)
                assert lib.ucfp_wang_streams_state_bytes_sr(wc, W, sr) == w8 + extra, (W, sr)
                assert lib.ucfp_panako_streams_state_bytes_sr(pc, W, sr) == p8 + extra, (W, sr)
    assert 4 * (-(-44100 // 8000) + 1) == 28 and 4 * (-(-384000 // 8000) + 1) == 196      # 7 and 49 floats
    assert lib.ucfp_wang_streams_state_bytes_sr(None, 0, 8000) == lib.ucfp_wang_streams_state_bytes(None)
    for sr in (0, 999, 384001):
        assert lib.ucfp_wang_streams_state_bytes_sr(None, 0, sr) == 0
        assert lib.ucfp_panako_streams_state_bytes_sr(None, 0, sr) == 0
    assert lib.ucfp_wang_streams_state_bytes_sr(None, 8193, 44100) == 0
    assert lib.ucfp_wang_streams_state_bytes_sr(C.byref(_wcfg(pps=0)), 0, 44100) == 0
    assert lib.ucfp_panako_streams_state_bytes_sr(C.byref(_pcfg(pps=0)), 0, 44100) == 0
