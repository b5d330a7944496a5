"""Live Wang windows on the CPU: the two facts the ring relies on, checked against the oracle's Wang
hashes -- t_anchor never decreases in offline order, and the hashes of any window [max(0, F - W), F) number at most
window_cap -- and the host-only closed forms of the C ABI (no device needed)."""
import ctypes as C

import numpy as np

from ucfp_amd import _lib

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4
WINDOWS = (1, 63, 625, 8192)
MAX_W = 8192


def _cfg(zone_t=63, pps=30, fan_out=10, zone_f=64, db=-50.0):
    return _lib.WangConfig(fan_out, zone_t, zone_f, pps, db)


def _window_cap(W, pps, fan_out):
    """A20 word for word: (ceil(2 W / 125) + 1) seconds of at most pps anchors of at most fan_out hashes."""
    return (-(-2 * W // 125) + 1) * pps * fan_out if W else 0


def test_anchor_order_and_window_bound_against_the_oracle(oracle):
    lib = _lib.load()
    rng = np.random.default_rng(20)
    tight = 0
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
        # the corners of the /v1/algorithms ranges first, then random configs over the whole of them
        if case < 4:
            fan, zt, zf, pps = [(64, 512, 1024, 256), (1, 1, 1, 1), (64, 1, 1024, 256), (64, 512, 1024, 1)][case]
        else:
            fan, zt, zf, pps = (int(rng.integers(1, 65)), int(rng.choice([1, 7, 63, 100, 300, 512])),
                                int(rng.choice([1, 16, 64, 512, 1024])), int(rng.choice([1, 5, 30, 100, 256])))
        full = oracle.wang(x, oracle.WangCfg(fan, zt, zf, pps, -50.0))
        ta = full[:, 1].astype(np.int64)
        assert np.all(np.diff(ta) >= 0), case            # hashes leave in anchor order
        c = _cfg(zt, pps, fan, zf)
        # F moves once a second: every 1000 samples reaches every value a stream of x can be asked at
        reach = sorted({int(lib.ucfp_wang_stream_frontier(m, C.byref(c))) for m in list(range(0, n + 1, 1000)) + [n]})
        assert reach[0] == 0
        for W in WINDOWS:
            cap = lib.ucfp_wang_streams_window_cap(C.byref(c), W)
            assert cap == _window_cap(W, pps, fan)
            for F in reach:
                held = int(np.searchsorted(ta, F, "left") - np.searchsorted(ta, max(0, F - W), "left"))
                assert held <= cap, (case, W, F, held, cap)
                tight = max(tight, held * 8 // max(cap, 1))
    assert tight >= 1          # some window came within a factor of 8 of its bound: the bound is not vacuous


def test_closed_forms_need_no_gpu():
    lib = _lib.load()
    assert MAX_W == 8192
    # the defaults: 3300 hashes and 8 + 8 * 3300 = 26 408 bytes of ring at W = 625
    assert lib.ucfp_wang_streams_window_cap(None, 625) == 3300
    assert lib.ucfp_wang_streams_state_bytes_ex(None, 625) == lib.ucfp_wang_streams_state_bytes(None) + 26408
    cfgs = [None, _cfg(), _cfg(zone_t=512, pps=256, fan_out=64), _cfg(zone_t=1, pps=1, fan_out=1), _cfg(pps=100, fan_out=3)]
    for c in cfgs:
        p = C.byref(c) if c is not None else None
        pps, fan = (c.peaks_per_sec, c.fan_out) if c is not None else (30, 10)
        base = lib.ucfp_wang_streams_state_bytes(p)
        assert base > 0
        assert lib.ucfp_wang_streams_state_bytes_ex(p, 0) == base          # W = 0 is today's set
        assert lib.ucfp_wang_streams_window_cap(p, 0) == 0
        for W in (1, 62, 63, 125, 126, 625, 8191, MAX_W):
            cap = _window_cap(W, pps, fan)
            assert lib.ucfp_wang_streams_window_cap(p, W) == cap
            assert lib.ucfp_wang_streams_state_bytes_ex(p, W) == base + 8 + 8 * cap
        for W in (MAX_W + 1, 1 << 20, 0xFFFFFFFF):                         # a window above the maximum
            assert lib.ucfp_wang_streams_window_cap(p, W) == 0
            assert lib.ucfp_wang_streams_state_bytes_ex(p, W) == 0
    for bad in (_cfg(zone_t=0), _cfg(zone_t=513), _cfg(pps=0), _cfg(pps=257), _cfg(fan_out=0), _cfg(fan_out=65),
                _cfg(zone_f=0), _cfg(zone_f=1025)):
        for W in (0, 63, MAX_W):
            assert lib.ucfp_wang_streams_window_cap(C.byref(bad), W) == 0
            assert lib.ucfp_wang_streams_state_bytes_ex(C.byref(bad), W) == 0


def test_windowed_set_checks_need_no_gpu():
    """create_ex judges the rate and the config first (UCFP_E_MODALITY), as create does; NULL arguments are refused."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ucfp_wang_streams_create_ex(None, 44100, None, 4, MAX_W + 1, C.byref(h)) == UCFP_E_MODALITY
    bad = _cfg(pps=257)
    assert lib.ucfp_wang_streams_create_ex(None, 8000, C.byref(bad), 4, MAX_W + 1, C.byref(h)) == UCFP_E_MODALITY
    assert lib.ucfp_wang_streams_create_ex(None, 8000, None, 4, 63, C.byref(h)) == UCFP_E_INVALID
    assert b"ctx" in lib.ucfp_last_error()
    assert not h.value
    assert lib.ucfp_wang_streams_windows_dev(None, None, 0, None, 0, None, None, None) == UCFP_E_INVALID
