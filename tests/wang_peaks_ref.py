"""Plain-numpy restatement of the Wang peak rule, pairing and hash, with the config as parameters.

The spectrum is the oracle's (`P = oracle.stft_power(x, 1024, 128)`, float32 [T, 512]); everything after it is restated
here.  Comparisons are written out as array tests on float32 values, so a NaN compares false on both sides exactly as
it does in C: a NaN cell is never a peak and never blocks one, and +Inf cells tie like any other value."""
import numpy as np

SR, HOP, RT, RK = 8000, 128, 7, 15


def candidates(P) -> np.ndarray:
    """A5, first half: bool [T, K], true where P > 0 and no cell of the clamped +-7 frame x +-15 bin window is greater,
    or equal and earlier in (t, k) order.  15 x 31 shifted-array tests."""
    P = np.asarray(P, np.float32)
    T, K = P.shape
    ok = P > 0
    for dt in range(-RT, RT + 1):
        t0, t1 = max(0, -dt), min(T, T - dt)             # rows t with 0 <= t + dt < T
        if t0 >= t1:
            continue
        for dk in range(-RK, RK + 1):
            if dt == 0 and dk == 0:
                continue
            k0, k1 = max(0, -dk), min(K, K - dk)
            v = P[t0:t1, k0:k1]
            o = P[t0 + dt:t1 + dt, k0 + dk:k1 + dk]
            blocked = o > v
            if dt < 0 or (dt == 0 and dk < 0):           # the neighbour comes first in (t, k) order: it wins a tie
                blocked = blocked | (o == v)
            ok[t0:t1, k0:k1] &= ~blocked
    return ok


def second_of(t):
    return (np.asarray(t, np.int64) * HOP) // SR


def peaks(P, peaks_per_sec: int, per_second=None):
    """A5: (t, k, p) in (t, k) order: of every second floor(t * 128 / 8000) the `peaks_per_sec` first candidates in
    (p descending, t ascending, k ascending) order.  `per_second`, if a dict, receives second -> candidate count."""
    P = np.asarray(P, np.float32)
    t, k = np.nonzero(candidates(P))                     # row-major: (t, k) order
    p = P[t, k]
    sec = second_of(t)
    keep = []
    for s in np.unique(sec):
        idx = np.nonzero(sec == s)[0]
        if per_second is not None:
            per_second[int(s)] = idx.size
        # stable sort on descending power: equal powers stay in (t, k) order
        order = idx[np.argsort(-p[idx].astype(np.float64), kind="stable")]
        keep.append(np.sort(order[:peaks_per_sec]))
    keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
    return t[keep].astype(np.uint32), k[keep].astype(np.uint32), p[keep]


def floor_power(db: float) -> np.float32:
    """A6: (float)(65536 * 10^(dB / 10)), evaluated in double from the float32 config field."""
    return np.float32(65536.0 * 10.0 ** (float(np.float32(db)) / 10.0))


def pairs(t, k, p, fan_out: int, zone_t: int, zone_f: int, db: float) -> np.ndarray:
    """A6 + A7 over peaks in (t, k) order: uint32 [n, 2] of (f_a << 23 | f_b << 14 | dt, t_anchor).  An anchor needs
    p >= floor; it takes the first `fan_out` later peaks with 0 < dt <= zone_t and |df| <= zone_f."""
    t = np.asarray(t, np.int64)
    k = np.asarray(k, np.int64)
    fl = floor_power(db)
    out = []
    for i in range(t.size):
        if not p[i] >= fl:
            continue
        dt = t[i + 1:] - t[i]
        df = np.abs(k[i + 1:] - k[i])
        j = np.nonzero((dt > 0) & (dt <= zone_t) & (df <= zone_f))[0][:fan_out] + i + 1
        h = (k[i] << 23) | (k[j] << 14) | ((t[j] - t[i]) & 0x3FFF)
        out.append(np.stack([h, np.full(j.size, t[i])], axis=1))
    if not out:
        return np.zeros((0, 2), np.uint32)
    return np.concatenate(out).astype(np.uint32)


def wang(P, fan_out=10, zone_t=63, zone_f=64, peaks_per_sec=30, db=-50.0) -> np.ndarray:
    t, k, p = peaks(P, peaks_per_sec)
    return pairs(t, k, p, fan_out, zone_t, zone_f, db)
