"""CPU restatement of the LSH de-duplication spec (DESIGN.md "LSH" L5-L7), shared by the dedup tests.

Rows are 0 .. n-1 of 1032-byte MinHash-128 records.  agree(a, c) = number of equal slots out of all 128.
  L5  per band, per maximal run of equal keys in the stably sorted table (rows r_0 < r_1 < ...): the candidate pairs
      are (r_i, r_j) with 0 < j - i <= span (span 0 = 16, SPAN_ALL = the whole run); `pairs` counts them over bands
  L6  a candidate is an edge if agree >= min_agree
  L7  clusters = connected components; label = smallest row, keep = (label == row), rep_id = ids[label]

`dedup_ref` is that text with a plain union-find.  The band keys are `oracle.lsh_band_keys` (numpy), the runs come
from a stable argsort.  Two things keep it usable on runs of thousands of rows, neither changes a result: the pairs
at distance d are taken for a whole band at once (in a sorted table key[p + d] == key[p] says p and p + d lie in one
run), and before the Python-level unions the edges whose ends already have one root are dropped (uniting them is a
no-op).  Rows with equal content (found once, by np.unique) agree in 128 slots without being compared again.
`brute_force` reads the definitions with no sort and no runs: the graph "share a band key and agree >= min_agree"
over all n^2 pairs, i.e. what an unbounded span must give."""
import numpy as np

import oracle

SPAN_ALL = 0xFFFFFFFF
DEFAULT_SPAN = 16


def slots_of(records) -> np.ndarray:
    r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, 1032)
    return np.ascontiguousarray(r[:, 8:]).view("<u8").reshape(-1, 128)


def records_of(slots) -> np.ndarray:
    """uint64 [n, 128] -> 1032-byte MinHash records (header: u16 schema = 1, six zero pad bytes)."""
    slots = np.ascontiguousarray(slots, dtype="<u8").reshape(-1, 128)
    n = slots.shape[0]
    rec = np.zeros((n, 1032), np.uint8)
    rec[:, 0] = 1
    rec[:, 8:] = slots.view(np.uint8).reshape(n, 1024)
    return rec


class UnionFind:
    def __init__(self, n: int):
        self.parent = np.arange(n, dtype=np.int64)

    def find(self, x: int) -> int:
        p = self.parent
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return int(x)

    def union(self, a: int, b: int) -> None:
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)      # the smaller row stays the root

    def roots(self) -> np.ndarray:
        """Root of every element (pointer jumping; leaves the forest flat)."""
        p = self.parent
        while True:
            q = p[p]
            if np.array_equal(q, p):
                return p
            p[:] = q


def _agree(slots, content, a, c, chunk=1 << 16) -> np.ndarray:
    out = np.full(a.shape[0], 128, np.int64)
    diff = np.flatnonzero(content[a] != content[c])       # equal content: 128 by definition
    for s in range(0, diff.size, chunk):
        d = diff[s:s + chunk]
        out[d] = (slots[a[d]] == slots[c[d]]).sum(axis=1)
    return out


def _finish(ids, labels, pairs):
    n = labels.shape[0]
    ids = np.asarray(ids, np.uint64).reshape(-1)
    keep = labels == np.arange(n)
    sizes = np.bincount(labels, minlength=max(n, 1))
    clusters = int(keep.sum())
    stats = np.array([pairs, clusters, n - clusters, int(sizes.max()) if n else 0], np.uint64)
    return labels.astype(np.uint32), ids[labels] if n else np.zeros(0, np.uint64), keep, stats


def dedup_ref(ids, records, bands: int = 16, rows: int = 8, min_agree: int = 103, span: int = DEFAULT_SPAN):
    """-> (labels uint32 [n], rep_ids uint64 [n], keep bool [n], stats uint64 [4] = pairs, clusters, duplicates, largest)."""
    assert 1 <= min_agree <= 128
    slots = slots_of(records)
    n = slots.shape[0]
    if span == 0:
        span = DEFAULT_SPAN
    if n == 0:
        return _finish(ids, np.zeros(0, np.int64), 0)
    keys = oracle.lsh_band_keys(records, bands, rows)
    content = np.unique(slots, axis=0, return_inverse=True)[1].reshape(-1)
    uf = UnionFind(n)
    pairs = 0
    for b in range(bands):
        order = np.argsort(keys[:, b], kind="stable")        # L2: rows ascend inside a run
        sk = keys[order, b]
        pos = np.arange(n - 1)                                 # positions p with key[p + d] == key[p], d = 1, 2, ...
        d = 1
        while d <= span and pos.size:
            pos = pos[pos + d < n]
            pos = pos[sk[pos + d] == sk[pos]]
            if not pos.size:
                break
            pairs += int(pos.size)
            a, c = order[pos], order[pos + d]                  # a < c
            edge = _agree(slots, content, a, c) >= min_agree
            if edge.any():
                a, c = a[edge], c[edge]
                r = uf.roots()
                new = r[a] != r[c]
                for x, y in zip(a[new].tolist(), c[new].tolist()):
                    uf.union(x, y)
            d += 1
    return _finish(ids, uf.roots().copy(), pairs)


def pairs_closed_form(records, bands: int, rows: int, span: int) -> int:
    """sum over runs of sum_i min(span, m - 1 - i)."""
    if span == 0:
        span = DEFAULT_SPAN
    keys = oracle.lsh_band_keys(records, bands, rows)
    total = 0
    for b in range(bands if keys.shape[0] else 0):
        _, counts = np.unique(keys[:, b], return_counts=True)
        for m in counts.tolist():
            total += sum(min(span, m - 1 - i) for i in range(m))
    return total


def brute_force(ids, records, bands: int, rows: int, min_agree: int):
    """All n^2 pairs, no sort, no runs: an edge joins two rows that share a band key and agree in >= min_agree slots.
    -> (labels, rep_ids, keep, stats) with stats[0] = the number of (pair, band) key matches."""
    slots = slots_of(records)
    n = slots.shape[0]
    keys = oracle.lsh_band_keys(records, bands, rows)
    uf = UnionFind(n)
    pairs = 0
    for a in range(n - 1):
        shared = (keys[a] == keys[a + 1:]).sum(axis=1)          # row a against every later row c
        agree = (slots[a] == slots[a + 1:]).sum(axis=1)
        pairs += int(shared.sum())
        for c in np.flatnonzero((shared > 0) & (agree >= min_agree)).tolist():
            uf.union(a, a + 1 + c)
    labels = np.array([uf.find(i) for i in range(n)], np.int64)
    return _finish(ids, labels, pairs)
