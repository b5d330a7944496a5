"""float64 reference of the cosine kNN contract (cosine.hip's header) and the checker the small-shard cosine tests share.

Contract: score = dot(q, v) / (|q| |v|); a row with zero norm or with any NaN / +-Inf component has no score (its norm is
Inf or NaN and its dot product +-Inf or NaN: the f32 score is always NaN, and "NaN scores are dropped"); a zero-norm query
has no hits; best k by (score descending, id ascending).  Everything here is plain numpy in float64 -- no f32 accumulation
order is restated -- so a GPU answer is compared within the project's tolerance and ids only where the reference's own
gaps decide the order.  (Rows whose f32 norm over- or underflows while the float64 one does not are outside this
reference: the tests that use it plant none.)"""
import numpy as np

INVALID_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_EXEMPT_SHARE = 0.10   # of a case's (query, rank) places, at most this share may be near-ties exempt from the id comparison


def make_case(n, dim, nq, seed):
    """Gaussian rows and queries with the plants every small-shard case carries (those the shard has room for):
      query 0 = 3 * a row; with n > 40 that row sits between a row with one NaN component and an all-+Inf row, all three in
                the same aligned 8 rows (so also the same 16-row tile and the same 32-row block)
      query 1 = a row that exists in four bit-identical copies at random positions (ids are shuffled: row order != id order)
      query 2 = 0 (no hits);   three zero rows.
    -> ids u64 [n], rows f32 [n, dim], queries f32 [nq, dim]"""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    queries = rng.standard_normal((nq, dim), dtype=np.float32)
    ids = rng.permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(5)
    if n > 40:
        p0 = 8 * int(rng.integers(0, n // 8)) + int(rng.integers(1, 7))
        taken = {p0 - 1, p0, p0 + 1}
        rows[p0 - 1, int(rng.integers(0, dim))] = np.nan
        rows[p0 + 1] = np.inf
    else:
        p0 = int(rng.integers(0, n))
        taken = {p0}
    queries[0] = rows[p0] * np.float32(3.0)
    free = [int(p) for p in rng.permutation(n) if int(p) not in taken]
    if nq >= 2 and len(free) >= 4:
        rows[free[1:4]] = rows[free[0]]
        queries[1] = rows[free[0]]
        free = free[4:]
    if len(free) >= 3:
        rows[free[:3]] = 0.0
    if nq >= 3:
        queries[2] = 0.0
    return ids, rows, queries


class CosineRef:
    """The best kmax + 1 of every query in float64, computed once; `check` compares a GPU answer for any k <= kmax over
    the first queries of the batch, `answer` is the reference's own answer in the GPU's output format."""

    def __init__(self, ids, rows, queries, kmax):
        self.ids = np.ascontiguousarray(ids, dtype=np.uint64)
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.kmax = int(kmax)
        n = self.rows.shape[0]
        finite = np.isfinite(self.rows).all(axis=1)
        r64 = np.where(finite[:, None], self.rows, np.float32(0)).astype(np.float64)
        rn = np.sqrt((r64 * r64).sum(axis=1))
        self.bad = ~finite | (rn == 0)                      # rows without a score
        self.bad_ids = self.ids[self.bad]
        self.row_of = {int(i): r for r, i in enumerate(self.ids)}
        assert len(self.row_of) == n, "ids must be unique"
        scorable = int((~self.bad).sum())
        q64 = np.asarray(queries, dtype=np.float32).astype(np.float64)
        qn = np.sqrt((q64 * q64).sum(axis=1))
        self.best = []                                      # per query: (row numbers, float64 scores) of the best kmax + 1
        for q0 in range(0, q64.shape[0], 64):
            dots = r64 @ q64[q0:q0 + 64].T
            for j in range(dots.shape[1]):
                kk = min(self.kmax + 1, scorable)
                if not (np.isfinite(qn[q0 + j]) and qn[q0 + j] > 0) or kk == 0:
                    self.best.append((np.zeros(0, np.int64), np.zeros(0, np.float64)))
                    continue
                sc = dots[:, j] / np.where(self.bad, 1.0, rn * qn[q0 + j])
                sc[self.bad] = -np.inf
                thr = np.partition(sc, n - kk)[n - kk]      # the kk-th best score: everything at or above it competes
                cand = np.nonzero(sc >= thr - 1e-12)[0]
                # Bit-identical rows have ONE score.  The matrix product above may round their dots differently (its
                # blocking depends on the row's position), which would order copies by that noise instead of by id --
                # and drop a copy an ulp under the threshold, hence the slack above.  The first copy met lends its score.
                sc_c, first = sc[cand], {}
                for t, r in enumerate(cand):
                    sc_c[t] = sc_c[first.setdefault(self.rows[r].tobytes(), t)]
                by = np.lexsort((self.ids[cand], -sc_c))[:kk]
                self.best.append((cand[by], sc_c[by]))

    def answer(self, k):
        """-> (ids [nq, k] u64, scores [nq, k] f32, counts [nq] u32): the reference's answer rounded to f32."""
        nq = len(self.best)
        g_ids = np.full((nq, k), INVALID_ID, np.uint64)
        g_sc = np.zeros((nq, k), np.float32)
        g_c = np.zeros(nq, np.uint32)
        for q, (order, sc) in enumerate(self.best):
            m = min(k, order.size)
            g_ids[q, :m], g_sc[q, :m], g_c[q] = self.ids[order[:m]], sc[:m], m
        return g_ids, g_sc, g_c

    def _same_row(self, a, b):
        return np.array_equal(self.rows[a].view(np.uint32), self.rows[b].view(np.uint32))

    def check(self, g_ids, g_sc, g_c, k, tol):
        """Asserts the answer of the first len(g_c) queries for this k; -> the largest |score - reference|.
          counts equal;  |score - ref| <= tol at every place;  no hit is a row without a score;  the scores of a query never
          rise from one place to the next, and every place beyond its count holds INVALID_ID;
          ids equal at every place whose float64 gaps to BOTH neighbours (the (k+1)-th best included: the k-th place is exempt
          only when it really is within 2 tol of the next) exceed 2 tol -- a zero gap between bit-identical copies of one row
          does not exempt: such hits must carry bit-equal scores and ascending ids, so their order is decided too;
          and, from the reference alone: at most MAX_EXEMPT_SHARE of the places are exempt (else the case proves little)."""
        assert 1 <= k <= self.kmax
        nq = len(g_c)
        assert nq <= len(self.best) and g_ids.shape == (nq, k) and g_sc.shape == (nq, k)
        places = exempt = 0
        dev = 0.0
        for q in range(nq):
            order, sc = self.best[q]
            m = min(k, order.size)
            assert g_c[q] == m, (q, int(g_c[q]), m)
            assert (g_ids[q, m:] == INVALID_ID).all(), (q, m, g_ids[q, m:])
            if m == 0:
                continue
            got_ids, got_sc = g_ids[q, :m], g_sc[q, :m]
            d = float(np.abs(got_sc.astype(np.float64) - sc[:m]).max())
            assert d <= tol, (q, d, got_sc, sc[:m])
            assert (np.diff(got_sc) <= 0).all(), (q, got_sc)
            dev = max(dev, d)
            assert not np.isin(got_ids, self.bad_ids).any(), (q, got_ids[np.isin(got_ids, self.bad_ids)])
            big = min(k + 1, order.size)
            close = (sc[:big - 1] - sc[1:big]) <= 2 * tol                 # close[j]: places j and j + 1 are a near-tie
            for j in np.nonzero(close)[0]:
                if self._same_row(order[j], order[j + 1]):
                    close[j] = False
            c = np.zeros(big + 1, bool)
            c[1:big] = close
            decided = ~(c[:m] | c[1:m + 1])
            assert np.array_equal(got_ids[decided], self.ids[order[:m]][decided]), (q, got_ids, self.ids[order[:m]], decided)
            places += m
            exempt += int((~decided).sum())
            groups = {}
            for pos in range(m):
                assert int(got_ids[pos]) in self.row_of, (q, pos, got_ids[pos])
                groups.setdefault(self.rows[self.row_of[int(got_ids[pos])]].tobytes(), []).append(pos)
            for at in groups.values():
                if len(at) > 1:
                    assert len(set(got_sc[at].view(np.uint32).tolist())) == 1, (q, at, got_sc[at])
                    assert (np.diff(got_ids[at].astype(np.int64)) > 0).all(), (q, at, got_ids[at])
        assert exempt <= MAX_EXEMPT_SHARE * places, (exempt, places)
        return dev
