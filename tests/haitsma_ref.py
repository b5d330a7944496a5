"""CPU restatement of the Haitsma sub-fingerprint index spec, shared by the Haitsma index tests.

Records and queries are uint32 [n] arrays of sub-fingerprints (or their little-endian bytes).  `HaitsmaRef` is the numpy
reference (sort + searchsorted + unique + popcount table); `brute_force` is the nested-loop reading of the definitions,
for small cases only.  Both return lists of (record_id, dist, offset, score)."""
import numpy as np

POP16 = np.array([bin(i).count("1") for i in range(65536)], np.int64)


def as_frames(x) -> np.ndarray:
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(bytes(x), "<u4").astype(np.uint32)
    return np.asarray(x, dtype=np.uint32).reshape(-1)


def popcount(v) -> np.ndarray:
    v = np.asarray(v, np.uint32)
    return POP16[v & np.uint32(0xFFFF)] + POP16[v >> np.uint32(16)]


def masks(flip_bits: int) -> np.ndarray:
    """The probe masks: 1, 33 or 529 of them."""
    if flip_bits not in (0, 1, 2):
        raise ValueError("flip_bits is 0, 1 or 2")
    m = [0]
    if flip_bits >= 1:
        m += [1 << b for b in range(32)]
    if flip_bits >= 2:
        m += [(1 << a) | (1 << b) for a in range(32) for b in range(a + 1, 32)]
    return np.array(m, np.uint32)


def score(dist: int, m: int) -> float:
    return float(np.float32(1) - np.float32(dist) / np.float32(32 * m))


class HaitsmaRef:
    """One tenant: {record_id: frames}."""

    def __init__(self, records: dict, max_postings: int = 0):
        self.max_postings = max_postings
        self.ids = np.array(sorted(records), np.uint64)
        fr = [as_frames(records[i]) for i in self.ids.tolist()]
        self.len = np.array([f.size for f in fr], np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.len)]).astype(np.int64)
        self.flat = np.concatenate(fr) if fr else np.zeros(0, np.uint32)
        self.pos = np.argsort(self.flat, kind="stable")
        self.val = self.flat[self.pos]

    def seeds(self, q, flip_bits: int):
        """-> (ordinals, offsets) of the admissible seeds, duplicates kept, and the number of positions looked at."""
        q = as_frames(q)
        m = q.size
        mk = masks(flip_bits)
        pr = (q[:, None] ^ mk[None, :]).ravel()
        j = np.repeat(np.arange(m), mk.size)
        lo = np.searchsorted(self.val, pr, "left")
        ln = np.searchsorted(self.val, pr, "right") - lo
        if self.max_postings:
            ln = np.where(ln > self.max_postings, 0, ln)
        tot = int(ln.sum())
        if not tot:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
        p = self.pos[np.repeat(lo - (np.cumsum(ln) - ln), ln) + np.arange(tot)]
        o = np.searchsorted(self.start, p, "right") - 1
        d = p - self.start[o] - np.repeat(j, ln)
        ok = (d >= 0) & (d + m <= self.len[o])
        return o[ok], d[ok], tot

    def candidates(self, q, flip_bits: int):
        o, d, _ = self.seeds(q, flip_bits)
        key = np.unique((o << 32) | d)
        return key >> 32, key & 0xFFFFFFFF

    def query(self, q, k: int, flip_bits: int = 2, max_ber_ppm: int = 350_000):
        q = as_frames(q)
        m = q.size
        if m == 0 or k == 0 or self.flat.size == 0:
            return []
        o, d = self.candidates(q, flip_bits)
        if not o.size:
            return []
        base, dist = self.start[o] + d, np.zeros(o.size, np.int64)
        step = max(1, (1 << 22) // m)              # candidates per pass: bounds the gathered block
        for a in range(0, o.size, step):
            idx = base[a:a + step, None] + np.arange(m)[None, :]
            dist[a:a + step] = popcount(self.flat[idx] ^ q[None, :]).sum(1)
        best = np.lexsort((d, dist, o))            # per ordinal: the smallest dist, then the smallest offset
        o, d, dist = o[best], d[best], dist[best]
        first = np.ones(o.size, bool)
        first[1:] = o[1:] != o[:-1]
        o, d, dist = o[first], d[first], dist[first]
        keep = dist * 1_000_000 <= max_ber_ppm * 32 * m
        o, d, dist = o[keep], d[keep], dist[keep]
        order = np.lexsort((self.ids[o], dist))[:k]
        return [(int(self.ids[o[i]]), int(dist[i]), int(d[i]), score(int(dist[i]), m)) for i in order]


def brute_force(records: dict, q, k: int, flip_bits: int = 2, max_ber_ppm: int = 350_000, max_postings: int = 0):
    """The definitions read literally (small cases only)."""
    recs = {int(rid): [int(x) for x in as_frames(v)] for rid, v in records.items()}
    Q = [int(x) for x in as_frames(q)]
    m = len(Q)
    P = {}
    for f in recs.values():
        for v in f:
            P[v] = P.get(v, 0) + 1
    stopped = {v for v, c in P.items() if max_postings and c > max_postings}
    pc = lambda x: bin(x).count("1")  # noqa: E731
    hits = []
    for rid, f in recs.items():
        best = None
        for d in range(0, len(f) - m + 1):
            if not any(pc(f[d + j] ^ Q[j]) <= flip_bits and f[d + j] not in stopped for j in range(m)):
                continue
            dist = sum(pc(f[d + j] ^ Q[j]) for j in range(m))
            if best is None or dist < best[0]:
                best = (dist, d)
        if best is not None and best[0] * 1_000_000 <= max_ber_ppm * 32 * m:
            hits.append((rid, best[0], best[1], score(best[0], m)))
    hits.sort(key=lambda x: (x[1], x[0]))
    return hits[:k] if m and k else []


# ---------------------------------------------------------------- shared cases

def fixed_cases():
    """[(name, records, query, max_postings)]: the corners of the spec, small enough for brute_force."""
    a, b, c, e = 0x12345678, 0x9ABCDEF0, 0x0F0F0F0F, 0xDEADBEEF
    seg = [a, b, c, e, a ^ 1, b ^ 2]
    return [
        ("exact", {7: [e, a, b, c, e], 9: [c, c, a]}, [a, b, c], 0),
        ("m=1", {7: [e, a, b], 2: [a ^ 3, a ^ 1]}, [a], 0),
        ("m=n_r", {7: [a, b, c], 8: [a, b, c ^ 7, e]}, [a, b, c], 0),
        ("m>n_r", {7: [a, b], 8: [a]}, [a, b, c], 0),
        ("empty record", {3: [], 7: [a, b, c], 9: []}, [b, c], 0),
        ("equal records", {11: seg, 5: seg, 8: seg[:3]}, seg[1:4], 0),
        ("segment twice", {4: seg + [e ^ 5] + seg, 6: seg}, seg, 0),
        ("long run", {4: [a] * 40 + [b, c], 6: [a] * 9}, [a] * 8, 0),
        ("long run stopped", {4: [a] * 40 + [b, c], 6: [a] * 9 + [b]}, [a, a, b], 10),
        ("flips", {4: [e, a ^ 3, b ^ 0x11, c ^ 0x80000001, e], 6: [a ^ 7, b ^ 7, c ^ 7]}, [a, b, c], 0),
        ("two bits on one frame only", {4: [a ^ 0x30, b ^ 0xF00, c ^ 0xF000], 6: [a ^ 0x70, b, c]}, [a, b, c], 0),
    ]


SR = 5000
CLIP = 2048 + 64 * 255      # samples of a 256-frame excerpt


def white(rng, secs=40):
    return (0.3 * rng.standard_normal(int(secs * SR))).astype(np.float32)


def tonal(rng, secs=40):
    n = int(secs * SR)
    t = np.arange(n) / SR
    x = np.zeros(n)
    seg = int(0.25 * SR)
    for s in range(0, n, seg):
        e = min(n, s + seg)
        for _ in range(4):
            f = rng.uniform(200, 2200)
            amp = rng.uniform(0.2, 1.0)
            x[s:e] += amp * np.sin(2 * np.pi * f * t[s:e] + rng.uniform(0, 6.28))
    x += 0.05 * rng.standard_normal(n)
    return (x / np.abs(x).max() * 0.8).astype(np.float32)


def corpus(gen, seed, n=24):
    """n recordings of 40 s drawn one after the other from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    return [gen(rng) for _ in range(n)]


def excerpts(xs, snr_db, seed):
    """One 256-frame excerpt per recording, cut at an arbitrary sample, with white noise at snr_db: [(s0, float32 clip)]."""
    rng = np.random.default_rng(seed)
    out = []
    for x in xs:
        s0 = int(rng.integers(0, x.size - CLIP))
        clip = x[s0:s0 + CLIP].astype(np.float64)
        clip = clip + rng.standard_normal(clip.size) * np.sqrt(np.mean(clip ** 2) / 10 ** (snr_db / 10))
        out.append((s0, clip.astype(np.float32)))
    return out


# the end-to-end inputs: (name, generator, corpus seed, excerpt seed, SNR in dB, flip_bits at which 24 of 24 must hold)
END_TO_END = (("white", white, 1000, 2000, 15, (0, 1, 2)), ("tonal", tonal, 1000, 2000, 20, (2,)))
FIRST_ID = 100


def identified(hits, rid, s0):
    """The condition on one excerpt: the source record first, its offset within one frame of s0 / 64, no other record."""
    return bool(hits) and hits[0][0] == rid and abs(hits[0][2] - s0 / 64) <= 1 and all(h[0] == rid for h in hits)
