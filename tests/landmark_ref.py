"""CPU restatement of the landmark index spec, shared by the landmark tests.

Landmarks are uint32 [n, 2] arrays of (hash, t).  `LandmarkRef` is the numpy reference; `brute_force` is the nested-loop
reading of the definitions, for small cases only."""
import numpy as np

BIAS = 1 << 31


def as_pairs(x) -> np.ndarray:
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(bytes(x), np.uint32).reshape(-1, 2)
    return np.asarray(x, dtype=np.uint32).reshape(-1, 2)


def _unique_keys(pairs) -> np.ndarray:
    p = as_pairs(pairs).astype(np.uint64)
    return np.unique((p[:, 0] << np.uint64(32)) | p[:, 1])


class LandmarkRef:
    """One tenant: {record_id: landmarks}."""

    def __init__(self, records: dict, max_postings: int = 0):
        self.max_postings = max_postings
        self.ids = np.array(sorted(records), np.uint64)
        keys, ords = [], []
        for o, rid in enumerate(self.ids.tolist()):
            k = _unique_keys(records[rid])
            keys.append(k)
            ords.append(np.full(k.size, o, np.int64))
        keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
        ords = np.concatenate(ords) if ords else np.zeros(0, np.int64)
        order = np.lexsort((ords, keys))
        self.keys, self.ords = keys[order], ords[order]
        self.hashes = (self.keys >> np.uint64(32)).astype(np.uint32)
        self.ts = (self.keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        self.postings = int(self.keys.size)

    def runs(self, q):
        """-> (|Q|, sorted unique query keys, run starts, run lengths after the stop cap)."""
        qk = _unique_keys(q)
        qh = (qk >> np.uint64(32)).astype(np.uint32)
        lo = np.searchsorted(self.hashes, qh, "left")
        hi = np.searchsorted(self.hashes, qh, "right")
        ln = hi - lo
        if self.max_postings:
            ln = np.where(ln > self.max_postings, 0, ln)
        return qk.size, qk, lo, ln

    def votes_total(self, q) -> int:
        return int(self.runs(q)[3].sum())

    def query(self, q, k: int, min_votes: int = 1):
        """-> list of (record_id, votes, offset, score)."""
        nq, qk, lo, ln = self.runs(q)
        if nq == 0 or k == 0 or ln.sum() == 0:
            return []
        tq = (qk & np.uint64(0xFFFFFFFF)).astype(np.int64)
        tot = int(ln.sum())
        start = np.repeat(lo - (np.cumsum(ln) - ln), ln) + np.arange(tot)
        which = np.repeat(np.arange(qk.size), ln)
        ords = self.ords[start]
        delta = self.ts[start] - tq[which]
        key, cnt = np.unique(ords * (1 << 33) + (delta + BIAS), return_counts=True)
        o, d = key >> 33, (key & ((1 << 33) - 1)) - BIAS
        best = np.lexsort((d, -cnt, o))           # per ordinal: max count, then the smallest offset
        o, d, cnt = o[best], d[best], cnt[best]
        first = np.ones(o.size, bool)
        first[1:] = o[1:] != o[:-1]
        o, d, cnt = o[first], d[first], cnt[first]
        keep = cnt >= max(min_votes, 1)
        o, d, cnt = o[keep], d[keep], cnt[keep]
        order = np.lexsort((self.ids[o], -cnt))[:k]
        return [(int(self.ids[o[i]]), int(cnt[i]), int(d[i]), float(np.float32(cnt[i]) / np.float32(nq))) for i in order]


def brute_force(records: dict, q, k: int, min_votes: int = 1, max_postings: int = 0):
    """The definitions read literally (small cases only)."""
    sets = {rid: {(int(h), int(t)) for h, t in as_pairs(v)} for rid, v in records.items()}
    Q = {(int(h), int(t)) for h, t in as_pairs(q)}
    P = {}
    for s in sets.values():
        for h, _ in s:
            P[h] = P.get(h, 0) + 1
    live = [(h, t) for h, t in Q if not (max_postings and P.get(h, 0) > max_postings)]
    hits = []
    for rid, s in sets.items():
        deltas = {tr - t for h, t in live for (hr, tr) in s if hr == h}
        best_v, best_d = 0, None
        for d in sorted(deltas):
            c = sum(1 for h, t in live if (h, t + d) in s)
            if c > best_v:
                best_v, best_d = c, d
        if best_v >= max(min_votes, 1):
            hits.append((rid, best_v, best_d, float(np.float32(best_v) / np.float32(len(Q)))))
    hits.sort(key=lambda x: (-x[1], x[0]))
    return hits[:k] if Q and k else []
