"""The oracle's Wang peaks, pairs and hashes against the numpy restatement of tests/wang_peaks_ref.py
on the clips of tests/wang_cases.py, and the property every clip exists for.  Conditions on the oracle alone: the GPU
tests of tests/test_wang_edges_gpu.py compare the kernels with this oracle on these clips, so a clip that lost its
property would leave them passing and empty."""
import numpy as np
import pytest

import wang_cases as wc
import wang_peaks_ref as wr

PPS = (1, 30, 255, 256)
CONFIGS = ((10, 63, 64, -50.0), (64, 512, 1024, -200.0), (64, 8, 16, -200.0), (1, 512, 1, -200.0))
TINY = np.finfo(np.float32).tiny


@pytest.fixture(scope="module")
def spectra(oracle):
    cache = {}

    def get(name, x):
        if name not in cache:
            cache[name] = oracle.stft_power(x, wc.N_FFT, wc.HOP)
        return cache[name]
    return get


def _stats(P):
    """Candidates per second, peaks per row and (t, k, p) before the per-second cap."""
    per = {}
    t, k, p = wr.peaks(P, 1 << 30, per)
    rows = np.bincount(t, minlength=P.shape[0])
    return per, rows, t, k, p


@pytest.mark.parametrize("name,x", list(wc.all_cases()), ids=[n for n, _ in wc.all_cases()])
def test_oracle_equals_restatement(oracle, spectra, name, x):
    P = spectra(name, x)
    assert P.shape == (wc.frames_of(x.size), wc.BINS)
    for pps in PPS:
        t, k, p = wr.peaks(P, pps)
        ot, ok, op = oracle.wang_peaks(P, pps)
        assert np.array_equal(ot, t) and np.array_equal(ok, k) and op.tobytes() == p.tobytes(), (name, pps)
        for fan_out, zt, zf, db in CONFIGS:
            o = oracle.wang(x, oracle.WangCfg(fan_out, zt, zf, pps, db), cap=pps * 3 * fan_out + 64)
            r = wr.pairs(t, k, p, fan_out, zt, zf, db)
            assert o.shape == r.shape and np.array_equal(o, r), (name, pps, fan_out, zt, zf, db)


@pytest.mark.parametrize("name", ["lattice_tied", "lattice_distinct", "lattice_partial"])
def test_lattices_fill_a_row_and_a_second(spectra, name):
    per, rows, t, k, p = _stats(spectra(name, wc.LATTICES[name]()))
    assert max(per.values()) >= 250 and rows.max() == 32          # kept[256] / kCandCap, and kPl, are reached
    sec = wr.second_of(t)
    if name == "lattice_tied":
        assert np.unique(p).size == 1                              # the rank is (t, k) alone
    elif name == "lattice_distinct":
        assert all(np.unique(p[sec == s]).size == (sec == s).sum() for s in per)   # the rank is the power alone
    else:
        counts = [np.unique(p[sec == s], return_counts=True)[1] for s in per]
        tied = sum(int(c[c > 1].sum()) for c in counts)            # peaks that share their power inside their second
        assert 0.1 * p.size < tied < 0.9 * p.size                  # both halves of the rank rule decide


def test_am_tones_fill_a_second_from_many_rows(spectra):
    per, rows, *_ = _stats(spectra("am_tones", wc.am_tones()))
    assert max(per.values()) >= 240 and rows.max() <= 8


@pytest.mark.parametrize("p", wc.PERIODS)
def test_period_clips_tie_across_the_window_edge(spectra, p):
    P = spectra(f"period{p}", wc.period(p))
    d = p // wc.HOP
    assert P.shape[0] == 120 and np.array_equal(P[:-d], P[d:])     # frames t and t + d are bit-identical
    _, _, t, _, _ = _stats(P)
    late = int((t >= wr.RT).sum())
    if d <= wr.RT:
        assert late == 0            # the twin 7 frames earlier is inside the window and wins every tie
    else:
        assert late >= 100          # the twin 8 or 9 frames away is outside it: both are peaks


def test_combs(spectra):
    per, rows, t, k, p = _stats(spectra("comb1024", wc.comb(1024)))
    assert max(per.values()) >= 250 and rows.max() == 32
    assert np.array_equal(np.unique(k[t == t[0]]), np.arange(0, 512, 16))       # neighbours exactly 16 bins apart
    per, rows, t, k, p = _stats(spectra("comb896", wc.comb(896)))
    # the strongest of the 7 distinct rows, once: every later copy loses to its twin 7 frames earlier
    assert t.size == 32 and (t == t[0]).all() and t[0] < wr.RT


@pytest.mark.parametrize("kind", list(wc.NONFINITE_KINDS))
@pytest.mark.parametrize("where", wc.NONFINITE_WHERE)
def test_nonfinite_clips_have_whole_nan_rows_and_peaks_beside_them(spectra, kind, where):
    P = spectra(f"nonfinite-{kind}-{where}", wc.nonfinite(kind, where))
    T = P.shape[0]
    want = np.zeros(T, bool)
    for i in wc.nonfinite_at(where):                               # the frames that hold sample i
        want[max(0, -(-(i - wc.N_FFT + 1) // wc.HOP)):min(T, i // wc.HOP + 1)] = True
    nan = np.isnan(P)
    assert np.array_equal(nan.all(axis=1), want) and np.array_equal(nan.any(axis=1), want)
    assert np.isfinite(P[~want]).all()
    _, rows, t, _, _ = _stats(P)
    assert not rows[want].any()                                    # a NaN cell is never a peak
    if where in ("mid", "pair15", "pair9"):
        edges = np.nonzero(want[1:] != want[:-1])[0]               # the finite row before / after each run
        beside = sorted({int(e) if want[e + 1] else int(e) + 1 for e in edges})
        assert len(beside) == (2 if where == "mid" else 3 if where == "pair9" else 4)
        for r in beside:
            assert rows[r] >= 1, (r, rows[r])                      # its 7 earlier or 7 later rows are all NaN
    if where == "pair9":
        r = wc.BAD // wc.HOP + 1                                   # the one finite row: NaN rows on both sides
        assert want[r - 7:r].all() and want[r + 1:r + 8].all() and not want[r] and rows[r] >= 2


@pytest.mark.parametrize("a", wc.SCALES)
def test_scaled_clips_reach_denormals_and_infinity(spectra, a):
    P = spectra(f"scaled{a:g}", wc.scaled(a))
    assert not np.isnan(P).any()
    _, rows, t, k, p = _stats(P)
    if a < 1:
        assert ((P > 0) & (P < TINY)).sum() > 1000                 # denormal powers
        assert (a > 1e-20) or (P == 0).sum() > 0                   # and, at the smallest, powers that underflow to 0
        assert t.size > 100
        assert (a > 1e-20) or (p < TINY).all()                     # ... where every peak is a denormal
    elif a == 1e17:
        assert np.isfinite(P).all() and P.max() > 1e36 and t.size > 100
    else:
        assert np.isinf(P).any(axis=1).all()                       # every row overflows
        assert a < 1e35 or np.isinf(P).all()                       # at 1e35 every cell does
        assert t.size == 1 and p[0] == np.inf                      # all ties: the first +Inf cell wins
        assert a < 1e35 or (t[0], k[0]) == (0, 0)


def test_zone_and_floor_cases_decide(oracle):
    """The configs of the GPU zone and floor tests differ where they are meant to: 7 versus 8 frames, 15 versus 16 bins,
    and a floor that splits the peaks of lattice_distinct near their median."""
    x = wc.lattice_distinct()
    n = {z: oracle.wang(x, oracle.WangCfg(*z)).shape[0] for z in wc.ZONES}
    assert n[(64, 7, 15, 256, -200.0)] == 0 < n[(64, 8, 15, 256, -200.0)] < n[(64, 8, 16, 256, -200.0)]
    assert n[(1, 512, 1, 256, -200.0)] > 600 and n[(64, 512, 1024, 256, -200.0)] > 40000
    m = {db: oracle.wang(x, oracle.WangCfg(64, 512, 1024, 256, db)).shape[0] for db in (30.0, wc.mid_floor_db(oracle), -200.0)}
    assert len(m) == 3 and m[30.0] == 0 < m[wc.mid_floor_db(oracle)] < m[-200.0]
