"""The few-query selection of the cosine search (topk.hip chunk_min_u32 + select_pruned_u32) at every size at which it
takes another path, through DeviceIndex(COSINE_F32, 4, APPEND_ONLY) on corpora built on the device.

The sizes follow from the constants of topk.hip:
  select_pruned_chunk   chunks of 1024 keys, doubled until at most kPruneMaxChunks = 4096 of them cover the corpus;
  256 threads           thread t of select_pruned_u32 looks after chunks t, t + 256, ...: a second slot from 257 chunks on;
  kPruneBatch = 4       pieces of 1024 keys gathered per trip: a chunk of more than 4096 keys spans two trips;
  kPruneKeep = 1024     the candidate list is pruned to its best k, and the threshold tightened, beyond this many;
  (n & 3) == 0          16-byte loads of the keys, scalar loads otherwise.

Rows are copies of a few integer directions, so a dot product and a squared norm are exact in f32 and every copy of a
direction scores the same bits: the answer is decided by (score class descending, id ascending) with no rounding question,
and it is computed here in integer / float64 arithmetic.  ids are a wrapping odd-multiplier image of the row number:
pseudo-random order, half of them above 2^63."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRUNE_BASE_CHUNK = 1024       # topk.hip select_pruned_chunk
PRUNE_MAX_CHUNKS = 4096       # topk.hip kPruneMaxChunks
PRUNE_BATCH = 4               # topk.hip kPruneBatch
PRUNE_KEEP = 1024             # topk.hip kPruneKeep
PRUNE_THREADS = 256           # topk.hip select_pruned_u32: __launch_bounds__(256), mine[kPruneMaxChunks / 256]
MAX_K = 128                   # ucfp_hip.h UCFP_INDEX_MAX_K
COS_TOL = 1e-5                # the project's bound on a cosine score
INVALID_ID = 0xFFFFFFFFFFFFFFFF
ID_MUL, ID_ADD = 0x9E3779B97F4A7C15, 0x0123456789            # id = row * ID_MUL + ID_ADD mod 2^64 (ID_MUL odd: a bijection)


def chunk_of(n):
    chunk = PRUNE_BASE_CHUNK
    while -(-n // chunk) > PRUNE_MAX_CHUNKS:
        chunk *= 2
    return chunk


def nchunks_of(n):
    return -(-n // chunk_of(n))


FULL = PRUNE_BASE_CHUNK * PRUNE_MAX_CHUNKS                     # 4 194 304: the last size with chunks of 1024
SIZES = [
    (10 + 1) * PRUNE_BASE_CHUNK,                               # 11 264: k + 1 chunks at k = 10, the fewest with a threshold
    MAX_K * PRUNE_BASE_CHUNK, MAX_K * PRUNE_BASE_CHUNK + 1,     # 131 072 / 131 073: 128 and 129 chunks against k = 128
    PRUNE_THREADS * PRUNE_BASE_CHUNK, PRUNE_THREADS * PRUNE_BASE_CHUNK + 1,   # 262 144 / 262 145: 256 and 257 chunks
    FULL,                                                      # 4096 chunks of 1024
    FULL + 1,                                                  # chunk 2048, odd n (scalar loads), a last chunk of one row
    FULL + 4,                                                  # chunk 2048, 16-byte loads
    2 * FULL + 4,                                              # chunk 4096: four pieces = kPruneBatch
    4 * FULL + 1,                                              # chunk 8192: eight pieces, a chunk spans two trips
]
assert SIZES == [11_264, 131_072, 131_073, 262_144, 262_145, 4_194_304, 4_194_305, 4_194_308, 8_388_612, 16_777_217]
assert [chunk_of(n) for n in SIZES] == [1024] * 6 + [2048, 2048, 4096, 8192]
assert [nchunks_of(n) for n in SIZES] == [11, 128, 129, 256, 257, 4096, 2049, 2049, 2049, 2049]
assert chunk_of(SIZES[-2]) // PRUNE_BASE_CHUNK == PRUNE_BATCH and chunk_of(SIZES[-1]) // PRUNE_BASE_CHUNK == 2 * PRUNE_BATCH
LARGEST = SIZES[-1]

# Integer directions, components in -8 .. 8.  TABLE[0] is the background; every direction has a positive dot product with
# it, so the negated background scores below zero against every row.
TABLE = np.array([[7, 7, 7, 8], [8, 1, 0, -4], [8, 3, -6, -2], [-5, 5, 7, -1], [3, 0, -5, 4], [-3, 2, 0, 7], [1, 1, 8, 4],
                  [8, 7, 2, -4]], np.int64)
ZERO = len(TABLE)                                              # the class of zero-norm rows: never returned
NEG_BG = -1                                                    # query code: the negated background


def query_vector(code):
    return -TABLE[0] if code == NEG_BG else TABLE[code]


def class_scores(code):
    """float64 cosine of the query with every direction of the table."""
    q = query_vector(code).astype(np.float64)
    t = TABLE.astype(np.float64)
    return (t @ q) / (np.linalg.norm(t, axis=1) * np.linalg.norm(q))


def assert_table_precondition():
    """For every query, two distinct directions score more than 1e-4 apart (far above the f32 error of a score), and the
    negated background scores at most -1e-4 everywhere: the order of the classes is the same in f32 and in float64."""
    assert np.abs(TABLE).max() <= 8 and np.all(TABLE @ TABLE[0] > 0)
    for code in [NEG_BG] + list(range(len(TABLE))):
        s = np.sort(class_scores(code))
        assert np.diff(s).min() > 1e-4, code
    assert class_scores(NEG_BG).max() < -1e-4 and class_scores(NEG_BG).min() == pytest.approx(-1.0, abs=1e-12)


def test_table_precondition():
    assert_table_precondition()


class Corpus:
    """rows, ids and the classes on the device; per class the 128 smallest ids (unsigned), computed with torch."""

    def __init__(self, torch, n, kind):
        assert_table_precondition()
        self.torch, self.n, self.kind = torch, n, kind
        chunk, nchunks = chunk_of(n), nchunks_of(n)
        row = torch.arange(n, dtype=torch.int64, device="cuda")
        if kind == "sparse":
            cls = torch.zeros(n, dtype=torch.int64, device="cuda")            # the background everywhere
            cls[(row * 7919 + 13) % 100_003 == 0] = ZERO                       # zero-norm rows here and there
            zc_all, zc_one = 3, 5                                              # a chunk of zero rows; one of zero rows + one row
            cls[zc_all * chunk:(zc_all + 1) * chunk] = ZERO
            cls[zc_one * chunk:(zc_one + 1) * chunk] = ZERO
            c_lo, c_hi = 1, nchunks - 2                                        # (c_hi: the second slot of its thread from 257 chunks on)
            assert len({c_lo, c_hi, zc_all, zc_one, nchunks - 1, 0}) == 6
            plant = [0, n - 1, zc_one * chunk + chunk - 3]
            for c in (c_lo, c_hi):
                # (with chunks of 1024 the second of these is the next chunk's first row and the third equals the first)
                plant += [c * chunk + 5, c * chunk + 1023, c * chunk + 1024, c * chunk + chunk - 1]
            plant = sorted(set(plant))
            assert 8 <= len(plant) <= 11 and plant[-1] == n - 1
            self.planted = {r: 1 + i % 4 for i, r in enumerate(plant)}         # four rare classes of 2 - 3 rows each
            for r, c in self.planted.items():
                cls[r] = c
            if n % chunk == 1:
                assert (n - 1) // chunk == nchunks - 1                         # the one-row last chunk holds a planted row
        else:
            # massive ties: direction 1 in 10 rows of 16, directions 2, 3 and the background in the others, in every chunk
            r16 = ((row * 2654435761) >> 7) % 16
            cls = torch.zeros(n, dtype=torch.int64, device="cuda")
            cls[r16 < 15] = 3
            cls[r16 < 13] = 2
            cls[r16 < 10] = 1
        self.cls = cls
        table = torch.tensor(np.vstack([TABLE, np.zeros((1, 4), np.int64)]), dtype=torch.float32, device="cuda")
        self.rows = table[cls].contiguous()
        mul = ID_MUL - 2**64                                                   # the same multiplier in two's complement
        self.ids = row * mul + ID_ADD                                          # wraps
        assert not bool((self.ids == -1).any())                                # no id is 2^64 - 1
        assert bool((self.ids < 0).any()) and bool((self.ids >= 0).any())      # ids on both sides of 2^63
        self.count = torch.bincount(cls, minlength=ZERO + 1).cpu().numpy()
        flipped = self.ids ^ (-2**63)                                          # signed order of these = unsigned order of the ids
        self.best = {}
        for c in range(ZERO):
            if self.count[c] == 0:
                continue
            sel = flipped[cls == c]
            low = torch.sort(sel).values if sel.numel() <= MAX_K else torch.topk(sel, MAX_K, largest=False, sorted=True).values
            self.best[c] = (low ^ (-2**63)).cpu().numpy().view(np.uint64)
            assert np.all(self.best[c][1:] > self.best[c][:-1])
        self.live = int(n - self.count[ZERO])
        if kind == "ties":
            pad = torch.zeros(nchunks * chunk, dtype=torch.bool, device="cuda")
            pad[:n] = cls == 1
            per_chunk = pad.view(nchunks, chunk).sum(1)
            # >= 6000 copies of the best row, some in every chunk (a one-row last chunk apart): the list outgrows kPruneKeep
            assert self.count[1] >= 6000 > PRUNE_KEEP and bool((per_chunk[:-1] > 0).all())
        torch.cuda.synchronize()

    def expect(self, code, k):
        """(ids [k], float64 scores [k], count): classes by score descending, ids ascending within a class."""
        s = class_scores(code)
        ids = np.full(k, INVALID_ID, np.uint64)
        sc = np.full(k, -2.0)
        got = 0
        for c in np.argsort(-s):
            if c not in self.best or got == k:
                continue
            take = self.best[c][:k - got]
            ids[got:got + take.size] = take
            sc[got:got + take.size] = s[c]
            got += take.size
        assert got == min(k, self.live)
        return ids, sc, got


class Searcher:
    def __init__(self, torch, ctx, corpus):
        from ucfp_amd import index
        self.torch, self.corpus = torch, corpus
        self.ix = index.DeviceIndex(index.COSINE_F32, 4, index.APPEND_ONLY, ctx)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.ix.append_dev(0, corpus.ids.data_ptr(), corpus.rows.data_ptr(), corpus.n, self.stream)

    def check(self, codes, k):
        torch, nq = self.torch, len(codes)
        q = torch.tensor(np.stack([query_vector(c) for c in codes]), dtype=torch.float32, device="cuda")
        o_ids = torch.full((nq, k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        o_sc = torch.full((nq, k), 12345.0, dtype=torch.float32, device="cuda")
        o_keys = torch.full((nq, k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        o_cnt = torch.full((nq,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.ix.search_dev(0, q.data_ptr(), nq, k, o_ids.data_ptr(), o_sc.data_ptr(), o_keys.data_ptr(), o_cnt.data_ptr(),
                           self.stream)
        torch.cuda.synchronize()
        g_ids = o_ids.cpu().numpy().view(np.uint64)
        g_sc = o_sc.cpu().numpy()
        g_keys = o_keys.cpu().numpy().view(np.uint32)
        g_cnt = o_cnt.cpu().numpy().view(np.uint32)
        for j, code in enumerate(codes):
            what = (self.corpus.kind, self.corpus.n, "nq", nq, "k", k, "query", j, code)
            w_ids, w_sc, w_cnt = self.corpus.expect(code, k)
            assert int(g_cnt[j]) == w_cnt, what
            assert np.array_equal(g_ids[j], w_ids), what
            assert np.all(np.abs(g_sc[j].astype(np.float64) - w_sc) <= COS_TOL), what
            assert np.all(g_keys[j, w_cnt:] == np.uint32(0xFFFFFFFF)), what
            if code == NEG_BG:                                      # scores <= -0.0: the upper half of the key range
                assert np.all(g_keys[j, :w_cnt] >= np.uint32(0x80000000)), what

    def close(self):
        self.ix.close()


def _few_query_sets(n):
    """nq = 1 (a direction with planted / massively tied best rows, and the negated background), 2 and 4."""
    if n == LARGEST:
        return [[1], [NEG_BG]]                                      # (nq = 1 only at 16.8 M rows)
    return [[1], [NEG_BG], [NEG_BG, 2], [3, NEG_BG, 1, 4]]


@pytest.mark.parametrize("kind", ["sparse", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_cosine_few_queries_every_size(gpu_ctx, torch_cuda, n, kind):
    """1, 2 and 4 queries at k = 1, 10 and 128 over
    sparse: a huge background class, four rare classes of 2 - 3 rows planted at row 0, at row n - 1 (the one-row last chunk
            where n has one), at the 1024-key piece boundaries and the last row of two chunks, next to zero-norm rows, a
            chunk of nothing but zero rows and one of zero rows and a single planted row;
    ties:   >= 6000 copies of the best row in every chunk, so that the candidate list overflows kPruneKeep again and again
            and smaller ids keep arriving after the threshold has tightened."""
    corpus = Corpus(torch_cuda, n, kind)
    s = Searcher(torch_cuda, gpu_ctx, corpus)
    try:
        for codes in _few_query_sets(n):
            for k in (1, 10, MAX_K):
                s.check(codes, k)
    finally:
        s.close()


@pytest.mark.parametrize("kind", ["sparse", "ties"])
def test_cosine_sixteen_queries_take_the_same_selection(gpu_ctx, torch_cuda, monkeypatch, kind):
    """UCFP_COSINE_NO_PRUNE (read on every call) sends 5 .. 16 queries through the key matrix to select_pruned_u32: 16
    workgroups over chunks of 2048 keys."""
    monkeypatch.setenv("UCFP_COSINE_NO_PRUNE", "1")
    corpus = Corpus(torch_cuda, FULL + 4, kind)
    s = Searcher(torch_cuda, gpu_ctx, corpus)
    try:
        s.check([NEG_BG] + [c % len(TABLE) for c in range(1, 16)], 10)
    finally:
        s.close()


@pytest.mark.parametrize("kind", ["sparse", "ties"])
def test_cosine_seventeen_queries_odd_n_many_slices(gpu_ctx, torch_cuda, monkeypatch, kind):
    """One query more, under the same switch: select_topk_u32 over an odd n (unaligned rows of the key matrix: scalar head
    and tail around the 16-byte body) in 241 slices, merged by the tree (more than its fan-in of 64)."""
    monkeypatch.setenv("UCFP_COSINE_NO_PRUNE", "1")
    corpus = Corpus(torch_cuda, FULL + 1, kind)
    s = Searcher(torch_cuda, gpu_ctx, corpus)
    try:
        s.check([NEG_BG] + [c % len(TABLE) for c in range(1, 17)], 10)
    finally:
        s.close()
