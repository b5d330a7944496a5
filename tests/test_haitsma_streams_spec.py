"""Streaming Haitsma on the CPU: the stateful restatement (haitsma_stream_ref) against the oracle's
offline record for any cutting, ucfp_haitsma_stream_frames against the rule, the rule's prefix soundness against the
oracle, and the stream set's host-side argument checks (no device needed)."""
import ctypes as C

import numpy as np
import pytest

import haitsma_stream_ref as ref
from ucfp_amd import _lib

UCFP_E_MODALITY, UCFP_E_INDEX, UCFP_E_INVALID = -1, -3, -4
RATES = (1000, 4000, 4999, 5000, 5001, 8000, 11025, 22050, 44100, 48000, 384000)
SECONDS = 0.75          # 3750 samples at 5 kHz: 27 frames


def _noise(rng, n):
    return (0.3 * rng.standard_normal(n)).astype(np.float32)


def _random_cuts(rng, n):
    out, a = [], 0
    while a < n:
        c = 0 if rng.random() < 0.15 else int(rng.integers(0, 3001))
        out.append(min(c, n - a))
        a += out[-1]
    return out


@pytest.mark.parametrize("sr", RATES)
def test_chunked_ref_equals_the_offline_record(oracle, sr):
    rng = np.random.default_rng(sr)
    n = int(SECONDS * sr)
    x = _noise(rng, n)
    full = oracle.haitsma(x, sr)
    assert full.size >= 20
    for final_carries in (False, True):
        got = ref.run_stream(oracle, x, sr, _random_cuts(rng, n), final_carries)
        assert np.array_equal(got, full), (sr, final_carries)
    for c in (0, 1, 2, n - 1, n):
        for final_carries in (False, True):
            got = ref.run_stream(oracle, x, sr, [c, n - c], final_carries)
            assert np.array_equal(got, full), (sr, c, final_carries)
    # non-default band edges travel with the stream
    full = oracle.haitsma(x, sr, 150.0, 2400.0)
    assert np.array_equal(ref.run_stream(oracle, x, sr, _random_cuts(rng, n), fmin=150.0, fmax=2400.0), full)


def test_stream_frames_matches_the_rule():
    lib = _lib.load()
    for sr in RATES:
        ns = set(range(0, 200))
        for j in list(range(0, 40)) + [1000, 50000]:              # around every S = 2048 + 64 j
            centre = (2048 + 64 * j) * sr // 5000
            w = 3 * (sr // 5000 + 2)
            ns |= set(range(max(0, centre - w), centre + w))
        prev = 0
        for n in sorted(ns):
            fr = lib.ucfp_haitsma_stream_frames(n, sr, 0)
            assert fr == ref.stream_frames(n, sr), (sr, n)
            assert lib.ucfp_haitsma_stream_frames(n, sr, 1) == ref.stream_frames(n, sr, True), (sr, n)   # final, 0 new samples
            assert prev <= fr <= lib.ucfp_haitsma_stream_frames(n, sr, 1), (sr, n)                     # monotone in n
            prev = fr
    assert [lib.ucfp_haitsma_stream_frames(n, 5000, 0) for n in (2047, 2048, 2111, 2112)] == [0, 1, 1, 2]
    # the cap of the rule: at 8 kHz the 8299th sample must not release 5 kHz sample 5186
    assert ref.final_samples(8299, 8000) == 5186 and -(-8298 * 5000 // 8000) == 5187
    for sr in (0, 999, 384001):
        assert lib.ucfp_haitsma_stream_frames(10 ** 6, sr, 0) == 0


@pytest.mark.parametrize("sr", RATES)
def test_prefix_soundness_against_the_oracle(oracle, sr):
    """The first Fr(n) frames of oracle.haitsma(x[:n]) equal those of oracle.haitsma(x): what a stream has emitted after
    n samples is final."""
    lib = _lib.load()
    rng = np.random.default_rng(1000 + sr)
    n_all = int(SECONDS * sr)
    x = _noise(rng, n_all)
    full = oracle.haitsma(x, sr)
    step = max(1, sr // 5000)
    cuts = {0, 1, 2, n_all - 1, n_all} | set(int(v) for v in rng.integers(0, n_all + 1, 12))
    for j in (0, 1, 7):                                           # where frame j completes, sample by sample
        centre = (2048 + 64 * j) * sr // 5000
        cuts |= set(range(centre - 2 * step - 2, centre + 2 * step + 3))
    seen = set()
    for n in sorted(cuts):
        fr = lib.ucfp_haitsma_stream_frames(n, sr, 0)
        seen.add(fr)
        pre = oracle.haitsma(x[:n], sr)
        assert fr <= pre.size and np.array_equal(pre[:fr], full[:fr]), (sr, n)
    assert {0, 1, 2} <= seen


def test_stream_set_checks_need_no_gpu():
    import torch
    lib = _lib.load()
    h = C.c_void_p()
    for sr in (0, 999, 384001):
        assert lib.ucfp_haitsma_streams_create(None, sr, None, 4, 256, C.byref(h)) == UCFP_E_MODALITY
        assert b"sample rate" in lib.ucfp_last_error()
    for fmin, fmax in ((0.5, 2000.0), (300.0, 300.0), (2000.0, 300.0), (300.0, 2500.5), (float("nan"), 2000.0)):
        cfg = _lib.HaitsmaConfig(fmin, fmax)
        assert lib.ucfp_haitsma_streams_create(None, 8000, C.byref(cfg), 4, 256, C.byref(h)) == UCFP_E_MODALITY
        assert b"band edges" in lib.ucfp_last_error()
    assert lib.ucfp_haitsma_streams_create(None, 8000, None, 4, 4097, C.byref(h)) == UCFP_E_INVALID
    assert b"block_frames" in lib.ucfp_last_error()
    rc = lib.ucfp_haitsma_streams_create(None, 8000, None, 4, 256, C.byref(h))
    # no context can exist without a device: there the answer is "no device", with one it is the NULL context
    assert rc == (UCFP_E_INVALID if torch.cuda.is_available() else UCFP_E_INDEX), lib.ucfp_last_error()
    assert not h.value
    # a NULL set: status codes, no crash
    slot = C.c_uint32(0)
    n = C.c_size_t(0)
    assert lib.ucfp_haitsma_streams_open(None, C.byref(slot)) == UCFP_E_INVALID
    assert lib.ucfp_haitsma_streams_close(None, 0) == UCFP_E_INVALID
    assert lib.ucfp_haitsma_streams_max_frames(None, None, None, None, 0) == 0
    assert lib.ucfp_haitsma_streams_push(None, 0, None, 0, 1, None, 0, C.byref(n)) == UCFP_E_INVALID
    assert lib.ucfp_haitsma_streams_push_dev(None, None, None, None, 0, None, None, 0, None, None) == UCFP_E_INVALID
    assert lib.ucfp_haitsma_streams_blocks_dev(None, None, 0, None, 0, None, None) == UCFP_E_INVALID
    lib.ucfp_haitsma_streams_destroy(None)


def test_state_bytes_follow_the_formula():
    lib = _lib.load()
    for sr in RATES:
        for block in (0, 1, 256, 4096):
            want = 4 * (2048 + (-(-sr // 5000) + 1) + 33 + block)
            assert lib.ucfp_haitsma_streams_state_bytes(sr, block) == want, (sr, block)
    assert lib.ucfp_haitsma_streams_state_bytes(44100, 256) < 10 * 1024
    assert lib.ucfp_haitsma_streams_state_bytes(384000, 0) - lib.ucfp_haitsma_streams_state_bytes(5000, 0) == 4 * 76
    assert lib.ucfp_haitsma_streams_state_bytes(999, 0) == 0 and lib.ucfp_haitsma_streams_state_bytes(8000, 4097) == 0
