"""CPU restatement of the Panako vote whose bins follow the scale, shared by the Panako pitch tests.

A resampled copy has its times divided by the speed and its frequencies multiplied by it, so the three 9-bit bins of a
hash (k_a << 23 | k_b << 14 | k_c << 5 | r) move.  With bins = 1 a (query triple, posting) pair supports hypothesis s iff
|k_x' - B_s(k_x)| <= f_slack for x = a, b, c, |r' - r| <= r_slack and |256 d' - s d| <= 256 slack, where
B_s(k) = (512 k + s) // (2 s); everything else is A14's (panako_match_ref).  `PanakoPitchRef` is the numpy reference,
`brute_force` reads the definition literally, in nested loops, for small cases only, and `render_resampled` plays a
score at another speed the way a resampler does."""
import numpy as np

import panako_match_ref as pm
from panako_match_ref import Invalid, Unsupported  # noqa: F401

MAX_F_SLACK = 3
SCALED_DEFAULTS = dict(scale_step=2, f_slack=1)      # the Python defaults of bins="scaled" (ucfp_amd.index)


def config(bins: int = 0, f_slack: int = 0, **match) -> dict:
    """A14's checked parameters plus bins (0 kept, 1 scaled) and f_slack (0 ... 3, 0 when the bins are kept)."""
    c = pm.config(**match)
    if bins not in (0, 1) or not 0 <= f_slack <= MAX_F_SLACK or (bins == 0 and f_slack != 0):
        raise Invalid(f"bins = {bins}, f_slack = {f_slack}")
    c["bins"], c["f_slack"] = bins, f_slack
    return c


def bin_map(s, k):
    """B_s(k) = round(256 k / s), halves up."""
    return (512 * k + s) // (2 * s)


def bin_interval(k: int, kp: int, f: int):
    """The closed form: |k' - B_s(k)| <= f  <=>  s_lo <= s <= s_hi for 64 <= s <= 1024 (s_hi None = unbounded)."""
    s_lo = (512 * k) // (2 * kp + 2 * f + 1) + 1
    s_hi = (512 * k) // (2 * (kp - f) - 1) if kp - f >= 1 else None
    return s_lo, s_hi


def bins_of(h):
    return (h >> 23) & 511, (h >> 14) & 511, (h >> 5) & 511, h & 31


class PanakoPitchRef(pm.PanakoMatchRef):
    """One tenant: {record_id: Panako records}; bins = 0 is PanakoMatchRef word for word."""

    def __init__(self, records: dict, max_postings: int = 0):
        super().__init__(records, max_postings)
        if self.h.size:
            lo = np.searchsorted(self.h, self.h, "left")
            hi = np.searchsorted(self.h, self.h, "right")
            self.stopped = (hi - lo > max_postings) if max_postings else np.zeros(self.h.size, bool)
        else:
            self.stopped = np.zeros(0, bool)

    def votes(self, q, bins: int = 0, f_slack: int = 0, **match):
        c = config(bins, f_slack, **match)
        if not bins:
            nq, o, j, dl, c0 = super().votes(q, **match)
            return nq, o, j, dl, c
        t = pm.triples(q, 1 << 28)
        scales = np.array(c["scales"], np.int64)
        z = np.zeros(0, np.int64)
        if t.shape[0] == 0 or self.h.size == 0:
            return t.shape[0], z, z, z, c
        f, smin, smax = f_slack, int(scales[0]), int(scales[-1])
        live = np.nonzero(~self.stopped)[0]
        pa, pb, pc, prr = bins_of(self.h[live])
        out_o, out_j, out_d = [z], [z], [z]
        for h, a, d in t.tolist():
            ka, kb, kc, r = bins_of(h)
            # a cheap superset first: the bins any hypothesis allows, the ratio bits
            ok = np.abs(prr - r) <= c["r_slack"]
            for k, pk in ((ka, pa), (kb, pb), (kc, pc)):
                ok &= (pk >= bin_map(smax, k) - f) & (pk <= bin_map(smin, k) + f)
            ps = live[ok]
            if ps.size == 0:
                continue
            # then the definition, per hypothesis
            sup = np.abs(256 * self.d[ps][:, None] - scales[None, :] * d) <= 256 * c["slack"]
            for k, pk in ((ka, pa[ok]), (kb, pb[ok]), (kc, pc[ok])):
                sup &= np.abs(pk[:, None] - bin_map(scales, k)[None, :]) <= f
            m, j = np.nonzero(sup)
            out_o.append(self.o[ps[m]])
            out_j.append(j)
            out_d.append(self.a[ps[m]] - ((scales[j] * a + 128) >> 8))
        return t.shape[0], np.concatenate(out_o), np.concatenate(out_j), np.concatenate(out_d), c

    # query(q, k, min_votes, bins=..., f_slack=..., **match) is PanakoMatchRef's: it hands every keyword to votes(), and
    # the vote itself (sort, window count, fold, top-k) is A14's.


def brute_force(records: dict, q, k: int, min_votes: int = 1, max_postings: int = 0, bins: int = 0, f_slack: int = 0, **match):
    """The definitions read literally (small cases only)."""
    c = config(bins, f_slack, **match)
    if not bins:
        return pm.brute_force(records, q, k, min_votes, max_postings, **match)
    sets = {rid: {tuple(int(v) for v in row) for row in pm.triples(x, 1 << 31)} for rid, x in records.items()}
    Q = {tuple(int(v) for v in row) for row in pm.triples(q, 1 << 28)}
    P = {}
    for s in sets.values():
        for h, _, _ in s:
            P[h] = P.get(h, 0) + 1
    hits = []
    for rid, s in sets.items():
        best = None                                 # (votes, -|s - 256|, -s, -offset) maximised
        for sc in c["scales"]:
            offs = []
            for h, a, d in Q:
                ka, kb, kc, r = bins_of(h)
                for hp, ap, dp in s:
                    if max_postings and P[hp] > max_postings:
                        continue
                    kap, kbp, kcp, rp = bins_of(hp)
                    if (abs(kap - bin_map(sc, ka)) <= f_slack and abs(kbp - bin_map(sc, kb)) <= f_slack
                            and abs(kcp - bin_map(sc, kc)) <= f_slack and abs(rp - r) <= c["r_slack"]
                            and abs(256 * dp - sc * d) <= 256 * c["slack"]):
                        offs.append(ap - ((sc * a + 128) >> 8))
            for o0 in set(offs):
                n = sum(1 for o in offs if o0 <= o < o0 + c["window"])
                cand = (n, -abs(sc - 256), -sc, -o0)
                if best is None or cand > best:
                    best = cand
        if best is not None and best[0] >= max(min_votes, 1):
            hits.append((rid, best[0], -best[3], -best[2], float(np.float32(best[0]) / np.float32(len(Q)))))
    hits.sort(key=lambda x: (-x[1], x[0]))
    return hits[:k] if Q and k else []


# ---- signals ---------------------------------------------------------------------------------------------------------

def render_resampled(score, t0: float, t1: float, speed: float = 1.0, sr: int = pm.SR) -> np.ndarray:
    """The excerpt [t0, t1) of the score played at `speed` through a resampler: onsets and durations divided by speed
    (pm.render) and every frequency multiplied by it.  Tones pushed past sr / 2 alias and are left in."""
    score = np.array(score, dtype=np.float64, copy=True)
    score[:, 2] *= speed
    return pm.render(score, t0, t1, speed, sr)


def resampled_excerpt(i: int, speed: float) -> np.ndarray:
    return render_resampled(pm.make_score(9300 + i), pm.EXCERPT[0], pm.EXCERPT[1], speed)


# ---- fixed corners, shared by the spec test (reference and brute force) and the GPU test (the C ABI) -----------------

def hsh(ka: int, kb: int, kc: int, r: int = 0) -> int:
    return (ka << 23) | (kb << 14) | (kc << 5) | r


def one(s: int) -> dict:
    return dict(scale_min=s, scale_max=s, scale_step=1)


def corners():
    """-> list of (name, records {id: records}, query, kwargs of query() incl. max_postings, expected hits without the
    score or None)."""
    rec = pm.rec
    scaled = dict(bins=1, slack=0)
    return [
        ("k = 0 stays 0 under every scale", {1: rec((hsh(0, 0, 0), 100, 82)), 2: rec((hsh(1, 0, 0), 100, 82))},
         rec((hsh(0, 0, 0), 0, 64)), dict(f_slack=0, **scaled, **one(328)), [(1, 1, 100, 328)]),
        ("B_512(1) sits on an exact half and rounds up to 1",
         {1: rec((hsh(1, 1, 1), 20, 20)), 2: rec((hsh(0, 0, 0), 20, 20))}, rec((hsh(1, 1, 1), 5, 10)),
         dict(f_slack=0, **scaled, **one(512)), [(1, 1, 10, 512)]),
        ("one past the half: B_513(1) = 0", {1: rec((hsh(1, 1, 1), 20, 20)), 2: rec((hsh(0, 0, 0), 20, 20))},
         rec((hsh(1, 1, 1), 5, 10)), dict(f_slack=0, slack=1, bins=1, **one(513)), [(2, 1, 10, 513)]),
        ("bins clamped at 0 with f_slack = 3: no carry into the neighbouring field",
         {1: rec((hsh(2, 0, 3), 50, 40), (hsh(0, 510, 1), 50, 40), (hsh(2, 5, 3), 50, 40))},
         rec((hsh(1, 1, 1), 10, 40)), dict(f_slack=3, **scaled, **one(256)), [(1, 1, 40, 256)]),
        ("bins clamped at 511 with f_slack = 3: no carry into the neighbouring field",
         {1: rec((hsh(508, 511, 509), 50, 40), (hsh(509, 0, 0), 50, 40), (hsh(511, 506, 511), 50, 40))},
         rec((hsh(510, 510, 510), 10, 40)), dict(f_slack=3, **scaled, **one(256)), [(1, 1, 40, 256)]),
        ("B_s(k) above 511 is out of reach", {1: rec((hsh(511, 511, 511), 50, 40))}, rec((hsh(511, 511, 511), 10, 80)),
         dict(f_slack=3, **scaled, **one(128)), []),
        ("the bin interval and the d interval do not meet",
         {1: rec((hsh(100, 200, 300), 500, 100))}, rec((hsh(125, 250, 375), 0, 100)),
         dict(f_slack=1, bins=1, slack=2, scale_min=204, scale_max=320, scale_step=2), []),
        ("the same posting once d agrees with the bins",
         {1: rec((hsh(100, 200, 300), 500, 125))}, rec((hsh(125, 250, 375), 0, 100)),
         dict(f_slack=0, bins=1, slack=0, scale_min=204, scale_max=320, scale_step=2), [(1, 1, 500, 320)]),
        ("bins = 1, f_slack = 0, s = 256 is kept mode",
         {4: rec((pm.H0, 300, 100), (pm.H0 + 64, 340, 80)), 9: rec((pm.H0, 300, 100), (pm.H0 + 1, 350, 80))},
         rec((pm.H0, 40, 100), (pm.H0 + 64, 80, 80)), dict(f_slack=0, bins=1, slack=1, r_slack=1, **one(256)),
         [(4, 2, 260, 256), (9, 1, 260, 256)]),
        ("one posting votes under two hypotheses, the preferred one wins",
         {1: rec((hsh(100, 100, 100), 300, 100))}, rec((hsh(100, 100, 100), 0, 100)),
         dict(f_slack=1, bins=1, slack=2, scale_min=254, scale_max=258, scale_step=2), [(1, 1, 300, 256)]),
        ("a stopped hash beside a live one in the same bucket",
         {1: rec(*[(hsh(100, 100, 100), 300 + i, 50) for i in range(4)], (hsh(100, 100, 101), 300, 50)),
          2: rec((hsh(100, 100, 100), 300, 50))},
         rec((hsh(100, 100, 100), 0, 50)), dict(f_slack=1, max_postings=4, **scaled, **one(256)), [(1, 1, 300, 256)]),
        ("the same without the stop", {1: rec(*[(hsh(100, 100, 100), 300 + i, 50) for i in range(4)], (hsh(100, 100, 101), 300, 50)),
                                       2: rec((hsh(100, 100, 100), 300, 50))},
         rec((hsh(100, 100, 100), 0, 50)), dict(f_slack=1, **scaled, **one(256)), [(1, 5, 300, 256), (2, 1, 300, 256)]),
    ]


INVALID_CONFIGS = [dict(bins=2), dict(bins=1, f_slack=4), dict(bins=0, f_slack=1), dict(bins=1, f_slack=1, slack=9),
                   dict(bins=1, scale_min=63)]
