"""Streaming Wang on the CPU: the emission frontier F(n) restated in Python against
ucfp_wang_stream_frontier, the rule's prefix soundness against the oracle, and the stream set's host-side
argument checks (no device needed)."""
import ctypes as C

import numpy as np

from ucfp_amd import _lib

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4


def _frontier(n, zone_t):
    """A9 word for word: frames, J, S = the first second not yet closed, C = f0(S), F = max(0, C - zone_t)."""
    frames = 0 if n < 1024 else (n - 1024) // 128 + 1
    J = max(0, frames - 7)

    def f0(s):                       # first frame t of second s: floor(128 t / 8000) = s
        return -(-125 * s // 2)

    s = 0
    while f0(s + 1) <= J:
        s += 1
    return max(0, f0(s) - zone_t)


def _cfg(zone_t=63, pps=30, fan_out=10, zone_f=64, db=-50.0):
    return _lib.WangConfig(fan_out, zone_t, zone_f, pps, db)


def test_frontier_matches_the_rule():
    lib = _lib.load()
    ns = set(range(0, 3000)) | {10 ** 7, 10 ** 7 - 1, 8000 * 3600}
    for k in range(0, 1300):                       # every frame boundary 1024 + 128 k and its neighbours
        b = 1024 + 128 * k
        ns |= {b - 1, b, b + 1}
    for s in range(0, 160):                        # samples at which J reaches f0(s) (frames = f0(s) + 7)
        f = -(-125 * s // 2) + 7
        b = 1024 + 128 * (f - 1)
        ns |= {b - 1, b, b + 1}
    rng = np.random.default_rng(5)
    ns |= set(int(v) for v in rng.integers(0, 10 ** 7, 2000))
    for zone_t in (1, 2, 62, 63, 64, 125, 200, 512):
        cfg = _cfg(zone_t=zone_t)
        for n in sorted(ns):
            assert lib.ucfp_wang_stream_frontier(n, C.byref(cfg)) == _frontier(n, zone_t), (n, zone_t)
    assert lib.ucfp_wang_stream_frontier(8000 * 60, None) == _frontier(8000 * 60, 63)   # NULL = defaults


def test_frontier_is_monotone_and_lags_at_most_132_frames():
    lib = _lib.load()
    prev = 0
    for n in range(0, 8000 * 20, 37):
        f = lib.ucfp_wang_stream_frontier(n, None)
        frames = 0 if n < 1024 else (n - 1024) // 128 + 1
        assert prev <= f and (frames == 0 or frames - f <= 7 + 62 + 63)
        prev = f


def test_prefix_soundness_against_the_oracle(oracle):
    """oracle.wang(x[:m]) restricted to t_anchor < F(m) equals the same restriction of oracle.wang(x), and that
    restriction is a prefix of oracle.wang(x): what a stream emits after m samples is final."""
    lib = _lib.load()
    rng = np.random.default_rng(11)
    for case in range(40):
        sec = 2 + 10 * rng.random()
        n = int(sec * 8000)
        t = np.arange(n) / 8000.0
        x = 0.15 * rng.standard_normal(n)
        for _ in range(3):
            f = 100 + 3000 * rng.random()
            x += 0.2 * np.sin(2 * np.pi * f * t * (1 + 0.2 * rng.random() * t / sec))
        if case % 3 == 0:
            a = rng.integers(0, n)
            x[a:a + rng.integers(0, 16000)] = 0.0      # a silence gap
        x = x.astype(np.float32)
        cfg = oracle.WangCfg(int(rng.integers(1, 65)), int(rng.choice([1, 7, 63, 100, 300, 512])),
                             int(rng.choice([1, 16, 64, 512, 1024])), int(rng.choice([1, 5, 30, 100, 256])), -50.0)
        full = oracle.wang(x, cfg)
        for m in rng.integers(0, n + 1, 4):
            F = lib.ucfp_wang_stream_frontier(int(m), C.byref(_cfg(cfg.target_zone_t, cfg.peaks_per_sec,
                                                                      cfg.fan_out, cfg.target_zone_f)))
            pre = oracle.wang(x[:m], cfg)
            a = pre[pre[:, 1] < F]
            b = full[full[:, 1] < F]
            assert np.array_equal(a, b), (case, m)
            assert np.array_equal(b, full[:b.shape[0]]), (case, m)


def test_stream_set_checks_need_no_gpu():
    """Rate and config are rejected with UCFP_E_MODALITY before any device call; a NULL context with UCFP_E_INVALID."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ucfp_wang_streams_create(None, 8000, None, 4, C.byref(h)) == UCFP_E_INVALID
    assert b"ctx" in lib.ucfp_last_error()
    assert lib.ucfp_wang_streams_create(None, 44100, None, 4, C.byref(h)) == UCFP_E_MODALITY
    assert lib.ucfp_wang_streams_create(None, 16000, _cfg(), 4, C.byref(h)) == UCFP_E_MODALITY
    for bad in (_cfg(zone_t=0), _cfg(zone_t=513), _cfg(pps=0), _cfg(pps=257), _cfg(fan_out=65), _cfg(zone_f=1025)):
        assert lib.ucfp_wang_streams_create(None, 8000, C.byref(bad), 4, C.byref(h)) == UCFP_E_MODALITY
    assert not h.value
    # a NULL set: status codes, no crash
    slot = C.c_uint32(0)
    assert lib.ucfp_wang_streams_open(None, C.byref(slot)) == UCFP_E_INVALID
    assert lib.ucfp_wang_streams_close(None, 0) == UCFP_E_INVALID
    assert lib.ucfp_wang_streams_max_hashes(None, None, None, None, 0) == 0
    n = C.c_size_t(0)
    assert lib.ucfp_wang_streams_push(None, 0, None, 0, 1, None, 0, C.byref(n)) == UCFP_E_INVALID
    assert lib.ucfp_wang_streams_push_dev(None, None, None, None, 0, None, None, 0, None, None) == UCFP_E_INVALID
    # device bytes per stream: fixed by the config, ~16.5 KiB with the defaults
    assert 16000 < lib.ucfp_wang_streams_state_bytes(None) < 17500
    assert lib.ucfp_wang_streams_state_bytes(C.byref(_cfg(zone_t=512, pps=256))) < 64 * 1024
    assert lib.ucfp_wang_streams_state_bytes(C.byref(_cfg(pps=0))) == 0
