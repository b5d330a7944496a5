"""Streaming Panako on the CPU: the emission frontier restated in Python against
ucfp_panako_stream_frontier, the rule's prefix soundness and the window bound against the numpy restatement of the
Panako spec over the oracle's peaks, and the stream set's host-side argument checks (no device needed)."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr
from ucfp_amd import _lib

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4
MAX_W = 8192
WINDOWS = (1, 63, 625, 8192)


def _f0(s):                          # first frame t of second s: floor(128 t / 8000) = s
    return -(-125 * s // 2)


def _frontier(n, zone_t):
    """A9 word for word with Panako's zone: frames, J, S = the second holding frame J, C = f0(S), F = max(0, C - zone_t)."""
    frames = 0 if n < 1024 else (n - 1024) // 128 + 1
    J = max(0, frames - 7)
    s = (J * 128) // 8000
    assert _f0(s) <= J < _f0(s + 1)      # S is the second whose frames hold J
    return max(0, _f0(s) - zone_t)


def _cfg(zone_t=96, pps=30, fan_out=5, zone_f=96, db=-50.0):
    return _lib.PanakoConfig(fan_out, zone_t, zone_f, pps, db)


def _window_cap(cfg, w):
    return (-(-2 * w // 125) + 1) * cfg.peaks_per_sec * cfg.fan_out if w else 0


def test_frontier_matches_the_rule():
    lib = _lib.load()
    ns = set(range(0, 3000)) | {10 ** 7, 10 ** 7 - 1, 8000 * 3600}
    for k in range(0, 1300):                       # every frame boundary 1024 + 128 k and its neighbours
        b = 1024 + 128 * k
        ns |= {b - 1, b, b + 1}
    for s in range(0, 160):                        # samples at which J reaches f0(s) (frames = f0(s) + 7): second edges
        for zone_t in (0, 1, 96, 512):             # ... and where F = f0(s) - zone_t leaves zero: zone edges
            b = 1024 + 128 * (_f0(s) + 7 + zone_t - 1)
            ns |= {b - 1, b, b + 1}
    rng = np.random.default_rng(5)
    ns |= set(int(v) for v in rng.integers(0, 10 ** 7, 20000))
    for zone_t in (1, 96, 512):
        cfg = _cfg(zone_t=zone_t)
        for n in sorted(ns):
            assert lib.ucfp_panako_stream_frontier(n, C.byref(cfg)) == _frontier(n, zone_t), (n, zone_t)
    assert lib.ucfp_panako_stream_frontier(8000 * 60, None) == _frontier(8000 * 60, 96)   # NULL = defaults


def test_frontier_is_monotone_and_lags_at_most_a_second_and_a_zone():
    lib = _lib.load()
    for zone_t in (1, 96, 512):
        cfg = _cfg(zone_t=zone_t)
        prev = 0
        for n in range(0, 8000 * 20, 37):
            f = lib.ucfp_panako_stream_frontier(n, C.byref(cfg))
            frames = 0 if n < 1024 else (n - 1024) // 128 + 1
            assert prev <= f and (frames == 0 or frames - f <= 7 + 62 + zone_t)
            prev = f


@pytest.fixture(scope="module")
def offline(oracle):
    """40 random signals of 2-12 s with random configs over the whole range: (x, cfg, offline records), computed once."""
    rng = np.random.default_rng(19)
    out = []
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
        cfg = pr.Cfg(int(rng.integers(1, 65)), int(rng.choice([1, 7, 96, 100, 300, 512])),
                     int(rng.choice([1, 16, 96, 512, 1024])), int(rng.choice([1, 5, 30, 100, 256])), -50.0)
        out.append((x, cfg, pr.panako_ref(oracle, x, cfg)))
    return out


def test_prefix_soundness_against_the_oracle(oracle, offline):
    """panako_ref(x[:m]) restricted to t_a < F(m) equals the same restriction of panako_ref(x), and that restriction is
    a prefix of panako_ref(x): what a stream emits after m samples is final."""
    lib = _lib.load()
    rng = np.random.default_rng(23)
    total = 0
    for case, (x, cfg, full) in enumerate(offline):
        for m in rng.integers(0, x.size + 1, 4):
            F = lib.ucfp_panako_stream_frontier(int(m), C.byref(_cfg(cfg.target_zone_t, cfg.peaks_per_sec, cfg.fan_out,
                                                                      cfg.target_zone_f)))
            pre = pr.panako_ref(oracle, x[:m], cfg)
            a = pre[pre[:, 1] < F]
            b = full[full[:, 1] < F]
            assert np.array_equal(a, b), (case, m)
            assert np.array_equal(b, full[:b.shape[0]]), (case, m)
            total += b.shape[0]
    assert total > 10000


def test_window_cap_is_the_formula_and_bounds_every_window(offline):
    lib = _lib.load()
    for cfg in (_cfg(), _cfg(pps=256, fan_out=64), _cfg(pps=1, fan_out=1), _cfg(zone_t=512, fan_out=7, pps=11)):
        for w in (0, 1, 62, 63, 125, 126, 625, 2000, 8191, 8192):
            assert lib.ucfp_panako_streams_window_cap(C.byref(cfg), w) == _window_cap(cfg, w), w
        assert lib.ucfp_panako_streams_window_cap(C.byref(cfg), MAX_W + 1) == 0
    assert lib.ucfp_panako_streams_window_cap(None, 625) == 11 * 30 * 5
    assert lib.ucfp_panako_streams_window_cap(C.byref(_cfg(pps=0)), 625) == 0
    # every F a stream of that length can report, every W: the offline records with w0 <= t_a < F fit
    for case, (x, cfg, full) in enumerate(offline):
        c = _cfg(cfg.target_zone_t, cfg.peaks_per_sec, cfg.fan_out, cfg.target_zone_f)
        ta = full[:, 1].astype(np.int64)
        assert np.all(np.diff(ta) >= 0)
        fs = sorted({lib.ucfp_panako_stream_frontier(n, C.byref(c)) for n in range(0, x.size + 4000, 64)})
        for w in WINDOWS:
            cap = lib.ucfp_panako_streams_window_cap(C.byref(c), w)
            for F in fs:
                held = np.searchsorted(ta, F, "left") - np.searchsorted(ta, max(0, F - w), "left")
                assert held <= cap, (case, w, F, held, cap)


def test_state_bytes():
    lib = _lib.load()
    wang = lib.ucfp_wang_streams_state_bytes
    for cfg, wcfg in ((_cfg(), _lib.WangConfig(5, 96, 96, 30, -50.0)),
                      (_cfg(zone_t=512, pps=256, fan_out=64), _lib.WangConfig(64, 512, 96, 256, -50.0))):
        base = lib.ucfp_panako_streams_state_bytes(C.byref(cfg), 0)
        assert base == wang(C.byref(wcfg)) > 0          # A9's state, sized with the Panako config
        for w in (1, 63, 625, 8192):
            ring = lib.ucfp_panako_streams_state_bytes(C.byref(cfg), w) - base
            assert ring == 16 * _window_cap(cfg, w) + 8, w      # the records, head and count
        assert lib.ucfp_panako_streams_state_bytes(C.byref(cfg), MAX_W + 1) == 0
    assert lib.ucfp_panako_streams_state_bytes(None, 0) == lib.ucfp_panako_streams_state_bytes(C.byref(_cfg()), 0)
    for bad in (_cfg(zone_t=0), _cfg(zone_t=513), _cfg(pps=0), _cfg(pps=257), _cfg(fan_out=0), _cfg(fan_out=65),
                _cfg(zone_f=0), _cfg(zone_f=1025)):
        assert lib.ucfp_panako_streams_state_bytes(C.byref(bad), 0) == 0
        assert lib.ucfp_panako_streams_state_bytes(C.byref(bad), 625) == 0


def test_stream_set_checks_need_no_gpu():
    """Rate and config are rejected with UCFP_E_MODALITY before any device call; a NULL context with UCFP_E_INVALID."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ucfp_panako_streams_create(None, 8000, None, 4, 0, C.byref(h)) == UCFP_E_INVALID
    assert b"ctx" in lib.ucfp_last_error()
    assert lib.ucfp_panako_streams_create(None, 8000, None, 4, MAX_W + 1, C.byref(h)) == UCFP_E_INVALID
    assert lib.ucfp_panako_streams_create(None, 44100, None, 4, 625, C.byref(h)) == UCFP_E_MODALITY
    assert lib.ucfp_panako_streams_create(None, 16000, _cfg(), 4, 0, C.byref(h)) == UCFP_E_MODALITY
    for bad in (_cfg(zone_t=0), _cfg(zone_t=513), _cfg(pps=0), _cfg(pps=257), _cfg(fan_out=65), _cfg(zone_f=1025)):
        assert lib.ucfp_panako_streams_create(None, 8000, C.byref(bad), 4, 0, C.byref(h)) == UCFP_E_MODALITY
    assert not h.value
    # a NULL set: status codes, no crash
    slot = C.c_uint32(0)
    assert lib.ucfp_panako_streams_open(None, C.byref(slot)) == UCFP_E_INVALID
    assert lib.ucfp_panako_streams_close(None, 0) == UCFP_E_INVALID
    assert lib.ucfp_panako_streams_max_hashes(None, None, None, None, 0) == 0
    n = C.c_size_t(0)
    assert lib.ucfp_panako_streams_push(None, 0, None, 0, 1, None, 0, C.byref(n)) == UCFP_E_INVALID
    assert lib.ucfp_panako_streams_push_dev(None, None, None, None, 0, None, None, 0, None, None) == UCFP_E_INVALID
    assert lib.ucfp_panako_streams_windows_dev(None, None, 0, None, 0, None, None, None) == UCFP_E_INVALID
    lib.ucfp_panako_streams_destroy(None)
