"""Multi-tenant Hamming search (DESIGN M1 - M6): one batch in which every query names its own tenant.

The specification is one sentence: row i of a multi search is, bit for bit, what the per-tenant search of tenants[i] writes
for query i alone.  Expected answers come from the project's reference (oracle.hamming_topk) over the arrays of the host
model (tests/index_model.py), tenant by tenant; the per-tenant DeviceIndex.search(tenant, q[None], k) is a second witness.
Neither is the code under test.

Rows have few distinct bits (the AND of three random words), so that ties at the k-th distance are the rule; every
scenario is checked on the CPU to hold a query with more ties than places (eq > need) and one with rows strictly below the
k-th distance (lt > 0).  Sizes aim at the implementation's edges through ucfp_index_search_multi_limits: rows per work
item T, queries per work item Q, tie-list capacity C."""
import ctypes as C
import threading

import numpy as np
import pytest

from index_model import IndexModel

pytestmark = pytest.mark.gpu

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_DIST = np.uint32(0xFFFFFFFF)
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint32)


def low_bits(rng, n):
    """n 64-bit words with about 8 bits set: Hamming distances between them take few values."""
    w = rng.integers(0, 2**64, (3, n), dtype=np.uint64)
    return w[0] & w[1] & w[2]


def distances(rows, q):
    x = (np.ascontiguousarray(rows, np.uint64) ^ np.uint64(q)).view(np.uint8).reshape(-1, 8)
    return _POP8[x].sum(axis=1)


def tie_profile(rows, q, k):
    """-> (tau, lt, need, eq) of one query over one tenant's rows, as DESIGN M3 defines them (numpy, CPU)."""
    n = len(rows)
    cnt = min(k, n)
    if cnt == 0:
        return None
    hist = np.bincount(distances(rows, q), minlength=65)
    cum = np.cumsum(hist)
    tau = int(np.searchsorted(cum, cnt))
    lt = int(cum[tau] - hist[tau])
    return tau, lt, cnt - lt, int(hist[tau])


def assert_tie_rich(model, tenants, queries, k):
    """The scenario holds a query with more ties at tau than places for them, and one with rows below tau."""
    prof = [tie_profile(model.arrays(int(t))[1], q, k) for t, q in zip(tenants, queries)]
    prof = [p for p in prof if p]
    assert any(p[3] > p[2] for p in prof), "no query with eq > need: the scenario does not test ties"
    assert k == 1 or any(p[1] > 0 for p in prof), "no query with lt > 0"      # (lt < k: k = 1 has none by definition)


def expected(oracle, model, tenants, queries, k):
    """The reference's answer, tenant by tenant, with the padding of ucfp_index_search."""
    tenants = np.asarray(tenants, np.uint32)
    queries = np.asarray(queries, np.uint64)
    nq = len(tenants)
    ids = np.full((nq, k), INVALID, np.uint64)
    dist = np.full((nq, k), NO_DIST, np.uint32)
    counts = np.zeros(nq, np.uint32)
    for t in np.unique(tenants):
        sel = np.nonzero(tenants == t)[0]
        m_ids, m_rows = model.arrays(int(t))
        if len(m_ids) == 0:
            continue
        o_ids, o_d, o_c = oracle.hamming_topk(m_ids, m_rows, queries[sel], k)
        for j, i in enumerate(sel):
            c = int(o_c[j])
            ids[i, :c], dist[i, :c], counts[i] = o_ids[j, :c], o_d[j, :c], c
    scores = np.where(dist == NO_DIST, np.float32(-1.0), np.float32(1.0) - dist.astype(np.float32) * np.float32(1.0 / 64.0))
    return ids, scores.astype(np.float32), dist, counts


def assert_same(got, want, what=""):
    g_ids, g_sc, g_d, g_c = got
    w_ids, w_sc, w_d, w_c = want
    assert np.array_equal(g_c, w_c), f"{what}: counts differ at {np.nonzero(g_c != w_c)[0][:8]}"
    bad = np.nonzero((g_ids != w_ids).any(axis=1) | (g_d != w_d).any(axis=1))[0]
    assert bad.size == 0, f"{what}: rows {bad[:8]} differ: got {g_ids[bad[0]][:12]} / {g_d[bad[0]][:12]}, want {w_ids[bad[0]][:12]} / {w_d[bad[0]][:12]}"
    assert np.array_equal(g_sc.view(np.uint32), w_sc.view(np.uint32)), f"{what}: score bits differ"


def witness(ix, tenants, queries, k, rows=None):
    """The per-tenant search, one query per call (the second witness of M2)."""
    nq = len(tenants)
    rows = range(nq) if rows is None else rows
    out = (np.empty((len(rows), k), np.uint64), np.empty((len(rows), k), np.float32), np.empty((len(rows), k), np.uint32),
           np.empty(len(rows), np.uint32))
    for j, i in enumerate(rows):
        r = ix.search(int(tenants[i]), np.array([queries[i]], np.uint64), k)
        for o, a in zip(out, r):
            o[j] = a[0]
    return out


def check(ix, oracle, model, tenants, queries, k, what, witness_rows=None):
    got = ix.search_multi(tenants, queries, k)
    assert_same(got, expected(oracle, model, tenants, queries, k), what + " vs oracle")
    rows = list(range(len(tenants))) if witness_rows is None else list(witness_rows)
    assert_same(tuple(a[rows] for a in got), witness(ix, tenants, queries, k, rows), what + " vs per-tenant search")
    return got


def fill(ix, model, tenant, ids, rows):
    ix.upsert(tenant, ids, rows)
    model.upsert(tenant, ids, rows)


@pytest.fixture(scope="module")
def limits():
    from ucfp_amd import index
    return index.search_multi_limits()


@pytest.fixture(scope="module")
def world(gpu_ctx, limits):
    """One index: tenants of every size at the edges of a work item, ids in random order (row order carries no meaning)."""
    from ucfp_amd import index
    T, Q, _ = limits
    rng = np.random.default_rng(31)
    sizes = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 50_000]
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    tenant_of = {}
    for j, n in enumerate(sizes):
        t = 1000 + 37 * j
        tenant_of[n] = t
        fill(ix, model, t, rng.permutation(4 * n).astype(np.uint64)[:n] + np.uint64(10), low_bits(rng, n))
    tenant_of[0] = 5        # never upserted
    # 300 queries: a tenant with Q - 1, one with Q, one with Q + 1, the rest spread; shuffled
    per = {tenant_of[1]: Q - 1, tenant_of[T]: Q, tenant_of[2 * T + 3]: Q + 1, tenant_of[50_000]: 40, tenant_of[0]: 7}
    tenants = [t for t, c in per.items() for _ in range(c)]
    others = [tenant_of[n] for n in (2, 63, 64, 65, T - 1, T + 1)]
    while len(tenants) < 299:
        tenants.append(others[len(tenants) % len(others)])
    tenants = np.array(tenants, np.uint32)
    queries = low_bits(rng, len(tenants))
    for i in range(0, len(tenants), 5):        # every fifth query is a row of its tenant (distance 0 exists)
        rows = model.arrays(int(tenants[i]))[1]
        if len(rows):
            queries[i] = rows[int(rng.integers(len(rows)))]
    order = rng.permutation(len(tenants))
    tenants, queries = tenants[order], queries[order]
    tenants = np.append(tenants, tenants[17])      # a repeated (tenant, query) pair
    queries = np.append(queries, queries[17])
    yield ix, model, tenants, queries, tenant_of
    ix.close()


@pytest.mark.parametrize("k", [1, 10, 128])
def test_shapes_every_size_edge_against_both_witnesses(world, oracle, k):
    ix, model, tenants, queries, _ = world
    assert len(tenants) == 300
    assert_tie_rich(model, tenants, queries, k)
    got = check(ix, oracle, model, tenants, queries, k, f"shapes k={k}")
    assert np.array_equal(got[0][17], got[0][299]) and got[3][17] == got[3][299]
    assert (got[3] < k).any() or k == 1, "no query with k > n"


def test_answer_does_not_depend_on_the_batch(world, oracle):
    """The same queries reversed, all of one tenant, and one at a time give the same rows."""
    ix, model, tenants, queries, tenant_of = world
    k = 10
    full = ix.search_multi(tenants, queries, k)
    rev = ix.search_multi(tenants[::-1].copy(), queries[::-1].copy(), k)
    assert_same(tuple(a[::-1] for a in rev), full, "reversed batch")
    sel = np.nonzero(tenants == tenant_of[50_000])[0]
    one = ix.search_multi(tenants[sel], queries[sel], k)
    assert_same(one, tuple(a[sel] for a in full), "one tenant of the batch alone")
    single = ix.search_multi(tenants[3:4], queries[3:4], k)
    assert_same(single, tuple(a[3:4] for a in full), "one query alone")


@pytest.mark.parametrize("k", [10, 64])
def test_many_segments_4096_tenants(gpu_ctx, oracle, k):
    from ucfp_amd import index
    rng = np.random.default_rng(4096 + k)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    nt, n = 4096, 50
    for t in range(nt):
        fill(ix, model, 7 * t + 1, rng.permutation(1000).astype(np.uint64)[:n], low_bits(rng, n))
    tenants = (7 * rng.permutation(nt) + 1).astype(np.uint32)
    queries = low_bits(rng, nt)
    if k < n:       # (k = 64 takes all 50 rows of a tenant: no row at tau is left out, the padding is what it tests)
        assert_tie_rich(model, tenants[:64], queries[:64], k)
    got = check(ix, oracle, model, tenants, queries, k, f"4096 segments k={k}", witness_rows=range(0, nt, 32))
    assert (got[3] == min(k, n)).all()
    ix.close()


def test_one_segment_equals_the_batched_search(world, limits):
    """200 queries of one tenant: bit for bit the per-tenant search of the whole batch."""
    ix, model, _, _, tenant_of = world
    rng = np.random.default_rng(200)
    t = tenant_of[50_000]
    queries = low_bits(rng, 200)
    for k in (10, 128):
        got = ix.search_multi(np.full(200, t, np.uint32), queries, k)
        assert_same(got, ix.search(t, queries, k), f"one segment k={k}")


def test_a_batch_larger_than_one_plan(gpu_ctx, oracle):
    """More queries than one plan holds (16384): the batch runs in chunks, the rows stay in the caller's order."""
    from ucfp_amd import index
    rng = np.random.default_rng(77)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    for t in range(9):
        n = (0, 1, 40, 64, 65, 300, 1025, 17, 2)[t]
        if n:
            fill(ix, model, t, rng.permutation(5000).astype(np.uint64)[:n], low_bits(rng, n))
    nq = 16384 + 16384 + 37
    tenants = rng.integers(0, 9, nq).astype(np.uint32)
    queries = low_bits(rng, nq)
    check(ix, oracle, model, tenants, queries, 5, "chunked batch", witness_rows=range(0, nq, 257))
    ix.close()


# ---- ties ------------------------------------------------------------------------------------------------------------------
def test_ties_twenty_thousand_identical_codes(gpu_ctx, oracle, limits):
    """20 000 identical codes whose ids are a random permutation, 500 rows deleted first so that rows have moved: the k
    smallest ids answer, whatever the row order (the gated exact pass: far more ties than the tie list holds)."""
    from ucfp_amd import index
    _, _, cap = limits
    rng = np.random.default_rng(20000)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    code = np.uint64(0x0123456789ABCDEF)
    # distinct ids spread over all 64 bits (an odd multiplier is a bijection): every byte of an id decides somewhere
    ids = rng.permutation(1 << 20)[:20_500].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    fill(ix, model, 9, ids, np.full(20_500, code, np.uint64))
    gone = rng.permutation(ids)[:500]
    assert ix.delete(9, gone) == 500 and model.delete(9, gone) == 500
    fill(ix, model, 8, rng.permutation(900).astype(np.uint64)[:300], low_bits(rng, 300))     # an ordinary neighbour in the batch
    assert cap == 0 or 20_000 > cap
    tenants = np.array([9, 8, 9, 9, 8], np.uint32)
    queries = np.array([code, 3, code ^ np.uint64(0b111), code, 12345], np.uint64)
    left = np.sort(model.arrays(9)[0])
    for k in (10, 128):
        got = check(ix, oracle, model, tenants, queries, k, f"identical codes k={k}")
        assert np.array_equal(got[0][0], left[:k]) and (got[2][0] == 0).all()
        assert np.array_equal(got[0][2], left[:k]) and (got[2][2] == 3).all()
    ix.close()


def test_ties_at_the_tie_list_capacity(gpu_ctx, oracle, limits):
    """Tenants built around query 0: `lt` rows at distance 1, `eq` rows at distance 2, the rest far away.  eq = C - 1, C,
    C + 1 (the tie list exactly full, and one more: the gated pass); need = eq; need = 1."""
    from ucfp_amd import index
    _, _, cap = limits
    rng = np.random.default_rng(512)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    k = 10
    cases = [(3, 7), (9, 30), (0, 10), (0, 11)]                  # (lt, eq): need = eq; need = 1; no row below tau
    if cap > 0:
        cases += [(3, cap - 1), (3, cap), (3, cap + 1), (0, cap), (0, cap + 1), (9, cap + 1)]
    tenants = []
    for j, (lt, eq) in enumerate(cases):
        rows = np.concatenate([np.uint64(1) << rng.integers(0, 64, lt).astype(np.uint64),
                               np.full(eq, 0b11, np.uint64) << rng.integers(0, 63, eq).astype(np.uint64),
                               low_bits(rng, 200) | np.uint64(0xFFFF)]).astype(np.uint64)
        ids = rng.permutation(50_000)[:len(rows)].astype(np.uint64)
        order = rng.permutation(len(rows))
        fill(ix, model, 100 + j, ids[order], rows[order])
        prof = tie_profile(model.arrays(100 + j)[1], 0, k)
        assert prof == (2, lt, k - lt, eq), (lt, eq, prof)
        tenants.append(100 + j)
    tenants = np.array(tenants + tenants[::-1], np.uint32)
    check(ix, oracle, model, tenants, np.zeros(len(tenants), np.uint64), k, "tie-list capacity")
    ix.close()


# ---- index flavours and lifetime -------------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def test_append_only_index_filled_through_append_dev(gpu_ctx, torch_cuda, oracle, limits):
    from ucfp_amd import index
    torch = torch_cuda
    T, _, _ = limits
    rng = np.random.default_rng(6)
    ix = index.DeviceIndex(index.HAMMING64, flags=index.APPEND_ONLY, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    stream = torch.cuda.current_stream().cuda_stream
    for t, n in ((1, 65), (2, T + 1), (3, 3000)):
        for lo in range(0, n, 700):                       # several appends: the shard grows in between
            m = min(700, n - lo)
            ids = (rng.permutation(10_000)[:m] + 10_000 * (lo // 700)).astype(np.uint64)
            rows = low_bits(rng, m)
            d_ids, d_rows = _dev(torch, ids), _dev(torch, rows)
            ix.append_dev(t, d_ids.data_ptr(), d_rows.data_ptr(), m, stream)
            model.upsert(t, ids, rows)
    torch.cuda.synchronize()
    tenants = rng.integers(0, 5, 120).astype(np.uint32)
    queries = low_bits(rng, 120)
    assert_tie_rich(model, tenants, queries, 10)
    check(ix, oracle, model, tenants, queries, 10, "append-only index")
    ix.close()


def test_after_growth_and_deletes(gpu_ctx, oracle):
    from ucfp_amd import index
    rng = np.random.default_rng(8)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    for t in (1, 2, 3):
        fill(ix, model, t, rng.permutation(9000).astype(np.uint64)[:1000], low_bits(rng, 1000))
    tenants = rng.integers(1, 4, 90).astype(np.uint32)
    queries = low_bits(rng, 90)
    check(ix, oracle, model, tenants, queries, 10, "before growth")
    fill(ix, model, 2, np.arange(20_000, 21_500, dtype=np.uint64), low_bits(rng, 1500))     # past the shard's capacity
    gone = model.arrays(3)[0][::3]
    assert ix.delete(3, gone) == model.delete(3, gone)
    gone = model.arrays(1)[0]
    assert ix.delete(1, gone) == model.delete(1, gone)                                     # a tenant emptied
    assert_tie_rich(model, tenants, queries, 10)
    got = check(ix, oracle, model, tenants, queries, 10, "after growth and deletes")
    assert (got[3][tenants == 1] == 0).all()
    ix.close()


def test_two_streams_then_an_upsert_that_grows_a_shard(gpu_ctx, torch_cuda, oracle):
    """Two multi searches enqueued on two streams, an upsert that re-allocates a shard they read, a flush: both answer
    from the rows before the upsert; the next search sees the new rows."""
    from ucfp_amd import index
    torch = torch_cuda
    rng = np.random.default_rng(12)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = IndexModel(np.uint64)
    for t in (1, 2, 3, 4):
        fill(ix, model, t, rng.permutation(9000).astype(np.uint64)[:1000], low_bits(rng, 1000))
    k, nq = 10, 150
    batches = []
    for _ in range(2):
        tenants = rng.integers(0, 6, nq).astype(np.uint32)
        queries = low_bits(rng, nq)
        batches.append((tenants, queries, expected(oracle, model, tenants, queries, k)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    torch.cuda.synchronize()
    for (tenants, queries, _), s in zip(batches, streams):
        d_q = _dev(torch, queries)
        o = (torch.zeros(nq * k, dtype=torch.int64, device="cuda"), torch.zeros(nq * k, dtype=torch.float32, device="cuda"),
             torch.zeros(nq * k, dtype=torch.int32, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda"))
        s.wait_stream(torch.cuda.current_stream())
        ix.search_multi_dev(tenants, d_q.data_ptr(), nq, k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                            s.cuda_stream)
        outs.append((d_q, o))
    new_ids, new_rows = np.arange(30_000, 32_000, dtype=np.uint64), low_bits(rng, 2000)
    ix.upsert(2, new_ids, new_rows)          # 1000 -> 3000 rows: the shard is re-allocated
    ix.flush()
    for (tenants, queries, want), (_, o) in zip(batches, outs):
        got = (o[0].cpu().numpy().view(np.uint64).reshape(nq, k), o[1].cpu().numpy().reshape(nq, k),
               o[2].cpu().numpy().view(np.uint32).reshape(nq, k), o[3].cpu().numpy().view(np.uint32))
        assert_same(got, want, "search enqueued before the upsert")
    model.upsert(2, new_ids, new_rows)
    tenants, queries, _ = batches[0]
    check(ix, oracle, model, tenants, queries, k, "after the upsert", witness_rows=range(0, nq, 7))
    ix.close()


# ---- the device form's outputs ---------------------------------------------------------------------------------------------
def test_dev_outputs_between_sentinels_and_null_outputs(world, torch_cuda, oracle):
    ix, model, tenants, queries, _ = world
    torch = torch_cuda
    nq, k, guard = len(tenants), 10, 256
    sizes = [nq * k * 8, nq * k * 4, nq * k * 4, nq * 4]
    offs, at = [], guard
    for s in sizes:
        offs.append(at)
        at += (s + 255) // 256 * 256 + guard
    want = expected(oracle, model, tenants, queries, k)
    d_q = _dev(torch, queries)
    stream = torch.cuda.current_stream().cuda_stream

    def run(with_optional):
        buf = torch.full((at,), 0xA5, dtype=torch.uint8, device="cuda")
        p = [buf.data_ptr() + o for o in offs]
        ix.search_multi_dev(tenants, d_q.data_ptr(), nq, k, p[0], p[1] if with_optional else 0, p[2] if with_optional else 0,
                            p[3], stream)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        used = np.zeros(at, bool)
        for j, (o, s) in enumerate(zip(offs, sizes)):
            if with_optional or j in (0, 3):
                used[o:o + s] = True
        assert (h[~used] == 0xA5).all(), "bytes outside the output arrays were written"
        return [h[o:o + s] for o, s in zip(offs, sizes)]

    a = run(True)
    got = (a[0].view(np.uint64).reshape(nq, k), a[1].view(np.float32).reshape(nq, k), a[2].view(np.uint32).reshape(nq, k),
           a[3].view(np.uint32))
    assert_same(got, want, "device form")
    b = run(False)
    assert np.array_equal(b[0], a[0]) and np.array_equal(b[3], a[3]), "ids / counts change when scores and distances are NULL"


# ---- refusals and empties --------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_empties(world, gpu_ctx):
    from ucfp_amd import _lib, errors, index
    ix, _, tenants, queries, _ = world
    lib = _lib.load()
    nq, k = 8, 4
    t = np.ascontiguousarray(tenants[:nq])
    q = np.ascontiguousarray(queries[:nq])

    def fresh(kk):
        return (np.full((nq, kk), 77, np.uint64), np.full((nq, kk), 7.0, np.float32), np.full((nq, kk), 77, np.uint32),
                np.full(nq, 77, np.uint32))

    def untouched(o, counts_too=True):
        return (o[0] == 77).all() and (o[1] == 7.0).all() and (o[2] == 77).all() and (not counts_too or (o[3] == 77).all())

    def call(handle, tp, n, kk, o):
        return lib.ucfp_index_search_multi(handle, tp, q.ctypes.data, n, kk, o[0].ctypes.data, o[1].ctypes.data, o[2].ctypes.data,
                                           o[3].ctypes.data)

    o = fresh(k)
    assert call(ix.handle, None, nq, k, o) == errors.InvalidArgument.code and untouched(o)
    assert b"tenants" in lib.ucfp_last_error()
    o = fresh(index.MAX_K + 1)
    assert call(ix.handle, t.ctypes.data, nq, index.MAX_K + 1, o) == errors.InvalidArgument.code and untouched(o)
    cos = index.DeviceIndex(index.COSINE_F32, dim=16, ctx=gpu_ctx)
    o = fresh(k)
    assert call(cos.handle, t.ctypes.data, nq, k, o) == errors.UnsupportedError.code and untouched(o)
    assert b"COSINE_F32" in lib.ucfp_last_error()
    with pytest.raises(errors.UnsupportedError):
        index.MultiSearchBatcher(cos)
    cos.close()
    o = fresh(k)
    assert call(ix.handle, t.ctypes.data, 0, k, o) == 0 and untouched(o)                    # nq = 0
    assert call(ix.handle, None, 0, k, o) == 0 and untouched(o)
    assert call(ix.handle, t.ctypes.data, nq, 0, o) == 0 and untouched(o, counts_too=False) and (o[3] == 0).all()   # k = 0
    ids, sc, d, cnt = ix.search_multi(t[:0], q[:0], 5)
    assert ids.shape == (0, 5) and cnt.shape == (0,)


def test_dev_form_refusals_write_nothing(world, gpu_ctx, torch_cuda):
    """The same three refusals through ucfp_index_search_multi_dev: every output buffer keeps its sentinel bytes."""
    from ucfp_amd import _lib, errors, index
    torch = torch_cuda
    ix, _, tenants, queries, _ = world
    lib = _lib.load()
    nq, kbig = 8, index.MAX_K + 1
    t = np.ascontiguousarray(tenants[:nq])
    d_q = _dev(torch, queries[:nq])
    stream = torch.cuda.current_stream().cuda_stream
    cos = index.DeviceIndex(index.COSINE_F32, dim=16, ctx=gpu_ctx)
    for handle, tp, k, code, word in ((ix.handle, None, 4, errors.InvalidArgument.code, b"tenants"),
                                      (ix.handle, t.ctypes.data, kbig, errors.InvalidArgument.code, b"UCFP_INDEX_MAX_K"),
                                      (cos.handle, t.ctypes.data, 4, errors.UnsupportedError.code, b"COSINE_F32")):
        bufs = [torch.full((nq * kbig * w,), 0xA5, dtype=torch.uint8, device="cuda") for w in (8, 4, 4, 1)]
        rc = lib.ucfp_index_search_multi_dev(handle, tp, d_q.data_ptr(), nq, k, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                             bufs[2].data_ptr(), bufs[3].data_ptr(), stream)
        assert rc == code and word in lib.ucfp_last_error()
        torch.cuda.synchronize()
        assert all(bool((b == 0xA5).all()) for b in bufs), "a refused call wrote to an output"
    cos.close()


# ---- the micro-batcher -----------------------------------------------------------------------------------------------------
def test_multi_batcher_64_threads_200_tenants(gpu_ctx):
    from ucfp_amd import errors, index
    rng = np.random.default_rng(64)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    nt = 200
    for t in range(nt):
        n = int(rng.integers(1, 400))
        ix.upsert(t, rng.permutation(5000).astype(np.uint64)[:n], low_bits(rng, n))
    b = index.MultiSearchBatcher(ix, max_batch=256)
    per_tenant = index.SearchBatcher(ix, 3)
    with pytest.raises(errors.InvalidArgument):
        index.SearchBatcher.submit(b, 5, 3)               # a submit without a tenant on a multi batcher
    with pytest.raises(errors.InvalidArgument):
        index.MultiSearchBatcher.submit(per_tenant, 3, 5, 3)   # a submit with a tenant on a per-tenant batcher
    per_tenant.close()
    threads, per = 64, 50
    plans = [(rng.integers(0, nt + 2, per), low_bits(rng, per), int(rng.integers(1, 129))) for _ in range(threads)]
    errs = []

    def work(plan):
        ts, qs, k = plan
        try:
            for t, q in zip(ts, qs):
                g_ids, g_sc, g_d = b.submit(int(t), int(q), k)
                w_ids, w_sc, w_d, w_c = ix.search(int(t), np.array([q], np.uint64), k)
                c = int(w_c[0])
                if not (len(g_ids) == c and np.array_equal(g_ids, w_ids[0, :c]) and np.array_equal(g_d, w_d[0, :c])
                        and np.array_equal(g_sc.view(np.uint32), w_sc[0, :c].view(np.uint32))):
                    errs.append((int(t), int(q), k))
        except Exception as e:      # noqa: BLE001 -- reported below, from the main thread
            errs.append(repr(e))

    ths = [threading.Thread(target=work, args=(p,)) for p in plans]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, errs[:5]
    batches, items = b.stats()
    assert items == threads * per and batches < items
    b.close()
    index.MultiSearchBatcher(ix).close()       # create, destroy with nothing submitted
    ix.close()


# ---- GpuIndex --------------------------------------------------------------------------------------------------------------
def test_gpu_index_hamming_many_equals_hamming(gpu_ctx):
    from ucfp_amd import index
    rng = np.random.default_rng(99)
    g = index.GpuIndex(ctx=gpu_ctx)
    space = "imgfprint-phash-v1"
    hashes = {}
    for t in (1, 2, 9):
        n = 50 * t
        hashes[t] = low_bits(rng, n)
        g._hamming(space).upsert(t, rng.permutation(1000).astype(np.uint64)[:n], hashes[t])
    reqs = [(int(t), int(low_bits(rng, 1)[0])) for t in rng.integers(0, 11, 40)]      # unknown tenants included
    reqs += [(2, int(hashes[2][7])), (2, int(hashes[2][7]))]
    for k in (1, 10, 200):
        assert g.hamming_many(space, reqs, k) == [g.hamming(t, space, h, k) for t, h in reqs]
    assert g.hamming_many(space, reqs, 0) == [[] for _ in reqs]
    assert g.hamming_many("no-such-space", reqs, 5) == [[] for _ in reqs]
    assert g.hamming_many(space, [], 5) == []
