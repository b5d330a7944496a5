"""CPU restatement of the Panako (scale, offset) vote, shared by the Panako match tests.

Records and queries are uint32 [n, 4] arrays of (hash, t_a, t_b, t_c) or their bytes.  `PanakoMatchRef` is the numpy
reference; `brute_force` reads the definitions literally, in nested loops, for small cases only.  `Invalid` stands for
UCFP_E_INVALID, `Unsupported` for UCFP_E_UNSUPPORTED.

The second half is a score-based signal generator: a score is a list of tone bursts (onset, duration, frequency,
amplitude); `render(score, t0, t1, speed)` synthesises the excerpt [t0, t1) with every time divided by `speed` and the
frequencies kept -- a true time stretch, with no resampler."""
import numpy as np

DEFAULTS = dict(scale_min=204, scale_max=320, scale_step=4, window=16, slack=2, r_slack=1)
MAX_HYP, MAX_D = 64, 1023


class Invalid(ValueError):
    pass


class Unsupported(ValueError):
    pass


def config(**match) -> dict:
    """The checked match parameters, with `scales` = the hypotheses."""
    c = {**DEFAULTS, **match}
    if set(c) != set(DEFAULTS):
        raise Invalid(f"unknown match parameter in {sorted(match)}")
    if not (64 <= c["scale_min"] <= c["scale_max"] <= 1024 and c["scale_step"] >= 1 and 1 <= c["window"] <= 256
            and 0 <= c["slack"] <= 8 and c["r_slack"] in (0, 1)):
        raise Invalid(f"match config out of range: {c}")
    c["scales"] = list(range(c["scale_min"], c["scale_max"] + 1, c["scale_step"]))
    if len(c["scales"]) > MAX_HYP:
        raise Invalid(f"{len(c['scales'])} hypotheses")
    return c


def as_records(x) -> np.ndarray:
    if isinstance(x, (bytes, bytearray)):
        if len(x) % 16:
            raise Invalid("bytes are not a multiple of 16")
        return np.frombuffer(bytes(x), np.uint32).reshape(-1, 4)
    return np.asarray(x, dtype=np.uint32).reshape(-1, 4)


def triples(x, max_ta: int) -> np.ndarray:
    """The distinct (h, a, d) of an item as int64 [n, 3], sorted; Invalid on d outside 1 ... 1023 or t_a >= max_ta."""
    r = as_records(x).astype(np.int64)
    d = r[:, 3] - r[:, 1]
    if r.shape[0] and (d.min() < 1 or d.max() > MAX_D):
        raise Invalid("t_c - t_a outside 1 ... 1023")
    if r.shape[0] and r[:, 1].max() >= max_ta:
        raise Invalid(f"t_a >= {max_ta}")
    t = np.stack([r[:, 0], r[:, 1], d], axis=1)
    return np.unique(t, axis=0) if t.shape[0] else t


def pref_ranks(scales) -> np.ndarray:
    """rank[j] of hypothesis j in the order (|s - 256|, s)."""
    order = sorted(range(len(scales)), key=lambda j: (abs(scales[j] - 256), scales[j]))
    rank = np.zeros(len(scales), np.int64)
    rank[order] = np.arange(len(scales))
    return rank


class PanakoMatchRef:
    """One tenant: {record_id: Panako records}."""

    def __init__(self, records: dict, max_postings: int = 0):
        self.max_postings = max_postings
        self.ids = np.array(sorted(records), np.uint64)
        hs, as_, ds, os_ = [], [], [], []
        for o, rid in enumerate(self.ids.tolist()):
            t = triples(records[rid], 1 << 31)
            hs.append(t[:, 0]); as_.append(t[:, 1]); ds.append(t[:, 2]); os_.append(np.full(t.shape[0], o, np.int64))
        cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
        h, a, d, o = cat(hs), cat(as_), cat(ds), cat(os_)
        order = np.lexsort((o, d, a, h))
        self.h, self.a, self.d, self.o = h[order], a[order], d[order], o[order]
        self.postings = int(self.h.size)

    def votes(self, q, **match):
        """-> (|Q|, ordinal, j, offset) of every expanded vote of the query, in no particular order."""
        c = config(**match)
        t = triples(q, 1 << 28)
        scales = np.array(c["scales"], np.int64)
        if t.shape[0] == 0:
            return 0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), c
        qi, pi = [], []
        for dr in range(-c["r_slack"], c["r_slack"] + 1):
            r = (t[:, 0] & 31) + dr
            ok = (r >= 0) & (r <= 31)
            hp = (t[:, 0] & ~np.int64(31)) | np.clip(r, 0, 31)
            lo = np.searchsorted(self.h, hp, "left")
            ln = np.searchsorted(self.h, hp, "right") - lo
            ln = np.where(ok, ln, 0)
            if self.max_postings:
                ln = np.where(ln > self.max_postings, 0, ln)
            tot = int(ln.sum())
            if tot:
                qi.append(np.repeat(np.arange(t.shape[0]), ln))
                pi.append(np.repeat(lo - (np.cumsum(ln) - ln), ln) + np.arange(tot))
        if not qi:
            return t.shape[0], np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), c
        qi, pi = np.concatenate(qi), np.concatenate(pi)
        out_o, out_j, out_d = [], [], []
        for lo in range(0, qi.size, 1 << 16):      # in slices: the support matrix is matches x hypotheses
            qs, ps = qi[lo:lo + (1 << 16)], pi[lo:lo + (1 << 16)]
            sup = np.abs(256 * self.d[ps][:, None] - scales[None, :] * t[qs, 2][:, None]) <= 256 * c["slack"]
            m, j = np.nonzero(sup)
            out_o.append(self.o[ps[m]])
            out_j.append(j)
            out_d.append(self.a[ps[m]] - ((scales[j] * t[qs[m], 1] + 128) >> 8))
        return t.shape[0], np.concatenate(out_o), np.concatenate(out_j), np.concatenate(out_d), c

    def votes_total(self, q, **match) -> int:
        return int(self.votes(q, **match)[1].size)

    def query(self, q, k: int, min_votes: int = 1, **match):
        """-> list of (record_id, votes, offset, scale, score)."""
        nq, o, j, dl, c = self.votes(q, **match)
        if o.size >= 1 << 32:
            raise Unsupported("2^32 expanded votes")
        if nq == 0 or k == 0 or o.size == 0:
            return []
        key = ((o * 64 + j) << 33) + (dl + (1 << 31))
        order = np.argsort(key, kind="stable")
        key, o, j, dl = key[order], o[order], j[order], dl[order]
        cnt = np.searchsorted(key, key + c["window"], "left") - np.arange(key.size)
        rank = pref_ranks(c["scales"])[j]
        best = np.lexsort((dl, rank, -cnt, o))     # per ordinal: most votes, preferred scale, smallest offset
        o, j, dl, cnt = o[best], j[best], dl[best], cnt[best]
        first = np.ones(o.size, bool)
        first[1:] = o[1:] != o[:-1]
        o, j, dl, cnt = o[first], j[first], dl[first], cnt[first]
        keep = cnt >= max(min_votes, 1)
        o, j, dl, cnt = o[keep], j[keep], dl[keep], cnt[keep]
        order = np.lexsort((self.ids[o], -cnt))[:k]
        return [(int(self.ids[o[i]]), int(cnt[i]), int(dl[i]), int(c["scales"][j[i]]),
                 float(np.float32(cnt[i]) / np.float32(nq))) for i in order]


def brute_force(records: dict, q, k: int, min_votes: int = 1, max_postings: int = 0, **match):
    """The definitions read literally (small cases only)."""
    c = config(**match)
    sets = {rid: {tuple(int(v) for v in row) for row in triples(x, 1 << 31)} for rid, x in records.items()}
    Q = {tuple(int(v) for v in row) for row in triples(q, 1 << 28)}
    P = {}
    for s in sets.values():
        for h, _, _ in s:
            P[h] = P.get(h, 0) + 1
    hits = []
    for rid, s in sets.items():
        matches = []                                # (d, a, d', a') of every pair
        for h, a, d in Q:
            r = h & 31
            for rp in range(max(0, r - c["r_slack"]), min(31, r + c["r_slack"]) + 1):
                hp = (h & ~31) | rp
                if max_postings and P.get(hp, 0) > max_postings:
                    continue
                matches += [(d, a, dp, ap) for (h2, ap, dp) in s if h2 == hp]
        best = None                                 # (votes, -|s - 256|, -s, -offset) maximised
        for sc in c["scales"]:
            offs = [ap - ((sc * a + 128) >> 8) for d, a, dp, ap in matches if abs(256 * dp - sc * d) <= 256 * c["slack"]]
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

SR = 8000
N_RECORDINGS, RECORDING_S = 8, 20.0
EXCERPT = (4.0, 12.0)                                # seconds of the recording; frame 250 at hop 128
SPEEDS = (0.85, 0.9, 0.96, 1.0, 1.03, 1.1, 1.2)


def make_score(seed: int, seconds: float = RECORDING_S, per_second: float = 9.0):
    """Tone bursts at seeded onsets: rows of (onset s, duration s, frequency Hz, amplitude)."""
    rng = np.random.default_rng(seed)
    n = int(seconds * per_second)
    onset = np.sort(rng.uniform(0.0, seconds - 0.2, n))
    dur = rng.uniform(0.10, 0.16, n)
    freq = rng.integers(40, 440, n) * (SR / 1024.0)  # on the bin centres of the 1024-point transform
    amp = rng.uniform(0.08, 0.25, n)
    return np.stack([onset, dur, freq, amp], axis=1)


def render(score, t0: float, t1: float, speed: float = 1.0, sr: int = SR) -> np.ndarray:
    """The excerpt [t0, t1) of the score played at `speed`: onsets and durations divided by speed, frequencies kept."""
    n = int(round((t1 - t0) / speed * sr))
    x = np.zeros(n)
    for onset, dur, freq, amp in np.asarray(score):
        a = int(round((onset - t0) / speed * sr))
        m = int(round(dur / speed * sr))
        lo, hi = max(a, 0), min(a + m, n)
        if hi <= lo or m < 2:
            continue
        i = np.arange(lo, hi) - a
        x[lo:hi] += amp * np.hanning(m)[i] * np.sin(2 * np.pi * freq * i / sr)
    return x.astype(np.float32)


def recording(i: int) -> np.ndarray:
    return render(make_score(9300 + i), 0.0, RECORDING_S)


def stretched_excerpt(i: int, speed: float) -> np.ndarray:
    return render(make_score(9300 + i), EXCERPT[0], EXCERPT[1], speed)


# ---- fixed corners, shared by the spec test (reference and brute force) and the GPU test (the C ABI) -----------------

def rec(*rows) -> np.ndarray:
    """Rows of (hash, t_a, d) -> Panako records with t_b = t_a and t_c = t_a + d."""
    return np.array([(h, a, a, a + d) for h, a, d in rows], np.uint32).reshape(-1, 4)


ONE = dict(scale_min=256, scale_max=256, scale_step=1)        # the hypothesis s = 256 alone
H0, H1, H2 = (5 << 5) | 7, 9 << 5, 12 << 5                       # H1 and H2 have r = 0


def corners():
    """-> list of (name, records {id: records}, query, kwargs of query(), expected hits without the score or None)."""
    return [
        ("offsets W - 1 apart share a window", {1: rec((H0, 100, 50), (H0, 115, 50))}, rec((H0, 0, 50)),
         dict(window=16, slack=0, **ONE), [(1, 2, 100, 256)]),
        ("offsets W apart do not", {1: rec((H0, 100, 50), (H0, 116, 50))}, rec((H0, 0, 50)),
         dict(window=16, slack=0, **ONE), [(1, 1, 100, 256)]),
        ("a negative offset", {1: rec((H0, 5, 50), (H0 + 64, 9, 20))}, rec((H0, 50, 50), (H0 + 64, 54, 20)),
         dict(slack=0, **ONE), [(1, 2, -45, 256)]),
        ("s a + 128 on a multiple of 256", {1: rec((H0, 10, 48), (H0 + 64, 13, 48))}, rec((H0, 2, 64), (H0 + 64, 6, 64)),
         dict(scale_min=192, scale_max=192, scale_step=1, slack=0, window=1), [(1, 2, 8, 192)]),
        ("|256 d' - s d| = 256 slack, and one more", {1: rec((H0, 10, 52)), 2: rec((H0, 10, 53))}, rec((H0, 0, 50)),
         dict(slack=2, **ONE), [(1, 1, 10, 256)]),
        ("r = 0 and r = 31 with r_slack = 1",
         {1: rec((H1 | 1, 7, 10), (H1 | 31, 7, 10), (H2 | 30, 7, 10), ((H2 | 31) + 1, 7, 10))},
         rec((H1, 0, 10), (H2 | 31, 0, 10)), dict(r_slack=1, slack=0, **ONE), [(1, 2, 7, 256)]),
        ("the same with r_slack = 0",
         {1: rec((H1 | 1, 7, 10), (H1 | 31, 7, 10), (H2 | 30, 7, 10), ((H2 | 31) + 1, 7, 10))},
         rec((H1, 0, 10), (H2 | 31, 0, 10)), dict(r_slack=0, slack=0, **ONE), []),
        ("duplicated triples in record and query", {1: rec((H0, 10, 50), (H0, 10, 50))}, rec((H0, 3, 50), (H0, 3, 50)),
         dict(slack=0, **ONE), [(1, 1, 7, 256)]),
        ("a tie between 252 and 260 resolves to 252", {1: rec((H0, 40, 64))}, rec((H0, 10, 64)),
         dict(scale_min=252, scale_max=260, scale_step=8, slack=1), [(1, 1, 30, 252)]),
        ("a tie with 256 resolves to 256", {1: rec((H0, 40, 64))}, rec((H0, 10, 64)),
         dict(scale_min=252, scale_max=260, scale_step=4, slack=1), [(1, 1, 30, 256)]),
        ("an empty record", {1: rec(), 2: rec((H0, 40, 64))}, rec((H0, 10, 64)), dict(slack=0, **ONE), [(2, 1, 30, 256)]),
        ("pairs are counted: the score exceeds 1", {1: rec((H0, 100, 50), (H0, 101, 50), (H0, 102, 50))}, rec((H0, 0, 50)),
         dict(slack=0, **ONE), [(1, 3, 100, 256)]),
        ("the defaults over two records", {4: rec((H0, 300, 100), (H0 + 64, 340, 80), (H0 + 128, 390, 60)),
                                           9: rec((H0, 300, 100), (H0 + 64, 350, 80))},
         rec((H0, 40, 80), (H0 + 64, 72, 64), (H0 + 128, 112, 48)), dict(), None),
    ]


def invalid_items():
    """-> list of (name, item, is bad as a record, is bad as a query)."""
    return [
        ("15 bytes", b"\0" * 15, True, True),
        ("d = 0", rec((H0, 5, 0)), True, True),
        ("d = 1024", rec((H0, 5, 1024)), True, True),
        ("t_c < t_a", np.array([[H0, 9, 9, 3]], np.uint32), True, True),
        ("t_a = 2^31", rec((H0, 1 << 31, 5)), True, True),
        ("t_a = 2^28", rec((H0, 1 << 28, 5)), False, True),
        ("t_a = 2^28 - 1, d = 1023", rec((H0, (1 << 28) - 1, 1023)), False, False),
        ("t_a = 2^31 - 1", rec((H0, (1 << 31) - 1, 1)), False, True),
    ]


INVALID_CONFIGS = [dict(scale_min=63), dict(scale_max=1025), dict(scale_min=300, scale_max=299), dict(scale_step=0),
                   dict(window=0), dict(window=257), dict(slack=9), dict(r_slack=2),
                   dict(scale_min=200, scale_max=265, scale_step=1)]           # 66 hypotheses
