"""Filtered search on the device (DESIGN F3 - F5).  The yardstick is F4: a filtered search returns, bit for bit, what the
unfiltered entry returns on a second index of the same kind, dim and flags that holds exactly the allowed rows in the
shard's row order; Hamming answers are also checked against a numpy brute force under (distance, id)."""
import ctypes as C

import numpy as np
import pytest

import index_filter_ref as ref
from ucfp_amd import _lib, errors, index

pytestmark = pytest.mark.gpu

INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)


def same(a, b):
    """Bit-exact equality of two search answers (ids, scores, keys, counts)."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))


def dedicated(ix, ctx, ids, rows, mask):
    """The yardstick index: same kind, dim and flags, the allowed rows only, in the same relative order."""
    d = index.DeviceIndex(ix.kind, ix.dim, ix.flags, ctx)
    if mask.any():
        d.upsert(0, ids[mask], rows[mask])
    return d


def check(ix, ctx, view, ids, rows, queries, k, mask):
    """F4 for one view (`mask`: the rows it must allow) and one query batch; Hamming also against the brute force."""
    d = dedicated(ix, ctx, ids, rows, mask)
    got, want = ix.search(0, queries, k, view), d.search(0, queries, k)      # (the host entry refreshes a stale view)
    d.close()
    assert view.stats()["rows_allowed"] == int(mask.sum())
    assert same(got, want)
    view.check_guards()                                    # nothing wrote outside the view's own buffers
    if ix.kind == index.HAMMING64:
        b_ids, b_d, b_c = ref.hamming_topk(ids, rows, mask, queries, k)
        assert np.array_equal(got[0], b_ids) and np.array_equal(got[2], b_d) and np.array_equal(got[3], b_c)
    return got


def make_view(ix, data):
    return ix.filter(0, data)


def mixed_kind(rng):
    return lambda vals: ref.RUN if rng.integers(0, 3) == 0 else ref.default_kind(vals)


# ---- probe edges ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_probe_tile_edges(gpu_ctx, n):
    rng = np.random.default_rng(n)
    ids = rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(977) + np.uint64(1 << 33))   # not ascending with the row
    codes = rng.integers(0, 2**64, n, dtype=np.uint64)
    q = np.concatenate([codes[:1] ^ np.uint64(3), rng.integers(0, 2**64, 2, dtype=np.uint64)])
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    ix.upsert(0, ids, codes)
    patterns = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": np.arange(n) == 0, "last": np.arange(n) == n - 1,
                "every_other": np.arange(n) % 2 == 0}
    for name, mask in patterns.items():
        absent = [int(i) + 1 for i in ids[:5]] + [7, 2**64 - 1]          # ids the tenant does not hold are ignored
        view = make_view(ix, ref.write_ids([int(i) for i in ids[mask]] + absent, mixed_kind(rng)))
        got = check(ix, gpu_ctx, view, ids, codes, q, 5, mask)
        assert (got[3] == min(5, int(mask.sum()))).all(), name
        assert view.stats()["rows_seen"] == n
        view.close()
    ix.close()


def test_probe_every_container_type(gpu_ctx):
    """A shard that holds members and near misses of every hand-built filter; each filter must allow exactly its members."""
    rng = np.random.default_rng(5)
    cases = ref.hand_built()
    held = set()
    for _, members in cases.values():
        pick = members[:40] + members[-40:] + [members[int(j)] for j in rng.integers(0, max(len(members), 1), 40 if members else 0)]
        for m in pick:
            held.update(x for x in (m, m ^ 1, m + 1, m - 1, m + 65536, m ^ (1 << 32)) if 0 <= x < 2**64 - 1)
    ids = rng.permutation(np.array(sorted(held), dtype=np.uint64))
    codes = rng.integers(0, 2**64, ids.size, dtype=np.uint64)
    q = rng.integers(0, 2**64, 4, dtype=np.uint64)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    ix.upsert(0, ids, codes)
    for name, (data, members) in cases.items():
        view = make_view(ix, data)
        mask = np.isin(ids, np.array(members, dtype=np.uint64))
        assert name == "count_0" or mask.any(), name
        check(ix, gpu_ctx, view, ids, codes, q, 32, mask)
        view.close()
    ix.close()


@pytest.mark.parametrize("nc", [1, 2, 3, 4, 1000])
def test_probe_directory_sizes(gpu_ctx, nc):
    rng = np.random.default_rng(nc)
    keys = np.sort(rng.choice(1 << 20, nc, replace=False)).astype(np.uint64) * np.uint64(3)
    allowed = (keys << np.uint64(16)) | rng.integers(0, 65536, nc, dtype=np.uint64)
    others = np.concatenate([allowed ^ np.uint64(1 << 16), allowed ^ np.uint64(2), allowed + np.uint64(1 << 40)])
    ids = rng.permutation(np.concatenate([allowed, others]))
    codes = rng.integers(0, 2**64, ids.size, dtype=np.uint64)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    ix.upsert(0, ids, codes)
    view = make_view(ix, ref.write_ids(allowed.tolist(), mixed_kind(rng)))
    assert view.stats()["containers"] == nc
    check(ix, gpu_ctx, view, ids, codes, rng.integers(0, 2**64, 3, dtype=np.uint64), 10, np.isin(ids, allowed))
    view.close()
    ix.close()


# ---- Hamming ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ham(gpu_ctx):
    rng = np.random.default_rng(11)
    n = 20_000
    ids = rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(5) + np.uint64(9))
    codes = rng.integers(0, 2**64, n, dtype=np.uint64)
    mask = rng.random(n) < 0.15
    q = rng.integers(0, 2**64, 256, dtype=np.uint64)
    q[:64] = codes[mask][:64] ^ np.uint64(0x11)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    ix.upsert(0, ids, codes)
    data = index.filter_bytes(ids[mask], runs=True)
    view = ix.filter(0, data)
    d = dedicated(ix, gpu_ctx, ids, codes, mask)
    brute = ref.hamming_topk(ids, codes, mask, q, 32)
    yield dict(ix=ix, view=view, d=d, ids=ids, codes=codes, mask=mask, q=q, brute=brute, data=data)
    view.close()
    d.close()
    ix.close()


@pytest.mark.parametrize("nq", [1, 8, 9, 256])
@pytest.mark.parametrize("k", [1, 10, 32])
def test_hamming_view_equals_dedicated_index_and_brute_force(ham, nq, k):
    got = ham["ix"].search(0, ham["q"][:nq], k, ham["view"])
    assert same(got, ham["d"].search(0, ham["q"][:nq], k))
    b_ids, b_d, b_c = ham["brute"]
    assert np.array_equal(got[0], b_ids[:nq, :k]) and np.array_equal(got[2], b_d[:nq, :k])
    assert (got[3] == k).all() and 2500 < ham["view"].stats()["rows_allowed"] == int(ham["mask"].sum()) < 3500


def test_hamming_fewer_rows_than_k_and_ties(gpu_ctx):
    rng = np.random.default_rng(12)
    n = 3000
    ids = rng.permutation(np.arange(n, dtype=np.uint64) + np.uint64(100))
    codes = rng.choice(np.array([0, 1, 3, 2**64 - 1], dtype=np.uint64), n)          # four codes: every distance is a tie
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    ix.upsert(0, ids, codes)
    q = np.array([0, 1, 2, 2**63, 5, 6, 7, 8, 9], dtype=np.uint64)
    few = make_view(ix, ref.write_ids(ids[:7].tolist()))
    got = check(ix, gpu_ctx, few, ids, codes, q, 10, np.arange(n) < 7)
    assert (got[3] == 7).all() and (got[0][:, 7:] == INVALID).all() and (got[2][:, 7:] == 0xFFFFFFFF).all()
    ties = make_view(ix, ref.write_ids(ids[::3].tolist(), mixed_kind(rng)))
    for nq in (1, 9):
        check(ix, gpu_ctx, ties, ids, codes, q[:nq], 32, np.arange(n) % 3 == 0)
    few.close()
    ties.close()
    ix.close()


def dev_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def test_hamming_append_only_index_filtered(gpu_ctx, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(13)
    n = 50_000
    ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)                # ascending: the view keeps the order state
    codes = rng.integers(0, 2**64, n, dtype=np.uint64)
    mask = rng.random(n) < 0.3
    q = np.concatenate([codes[mask][:40] ^ np.uint64(9), rng.integers(0, 2**64, 60, dtype=np.uint64)])
    st = torch.cuda.current_stream().cuda_stream
    ix = index.DeviceIndex(index.HAMMING64, 0, index.APPEND_ONLY, gpu_ctx)
    d = index.DeviceIndex(index.HAMMING64, 0, index.APPEND_ONLY, gpu_ctx)
    d_ids, d_codes = dev_u64(torch, ids), dev_u64(torch, codes)
    m_ids, m_codes = dev_u64(torch, ids[mask]), dev_u64(torch, codes[mask])
    half = n // 2
    ix.append_dev(0, d_ids.data_ptr(), d_codes.data_ptr(), half, st)
    ix.append_dev(0, d_ids.data_ptr() + 8 * half, d_codes.data_ptr() + 8 * half, n - half, st)
    d.append_dev(0, m_ids.data_ptr(), m_codes.data_ptr(), int(mask.sum()), st)
    view = ix.filter(0, index.filter_bytes(ids[mask]))
    for nq, k in ((1, 10), (8, 32), (100, 10)):
        got = ix.search(0, q[:nq], k, view)
        assert same(got, d.search(0, q[:nq], k))
        b = ref.hamming_topk(ids, codes, mask, q[:nq], k)
        assert np.array_equal(got[0], b[0]) and np.array_equal(got[2], b[1]) and np.array_equal(got[3], b[2])
    view.close()
    d.close()
    ix.close()


# ---- cosine -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [8, 100, 768])
def test_cosine_view_equals_dedicated_index(gpu_ctx, dim):
    rng = np.random.default_rng(dim)
    n = 3000
    ids = rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(2))
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    mask = rng.random(n) < 0.4
    zero = np.flatnonzero(mask)[5]
    rows[zero] = 0.0                                                                   # a zero-norm row among the allowed rows
    rows[np.flatnonzero(mask)[6]] = rows[np.flatnonzero(mask)[9]]                      # and a tie
    q = rng.standard_normal((65, dim)).astype(np.float32)
    q[1] = rows[np.flatnonzero(mask)[9]]
    ix = index.DeviceIndex(index.COSINE_F32, dim, 0, gpu_ctx)
    ix.upsert(0, ids, rows)
    view = ix.filter(0, index.filter_bytes(ids[mask], runs=True))
    d = dedicated(ix, gpu_ctx, ids, rows, mask)
    allowed = set(ids[mask].tolist())
    for nq in (1, 5, 16, 65):
        got = ix.search(0, q[:nq], 10, view)
        assert same(got, d.search(0, q[:nq], 10))
        assert (got[3] == 10).all() and all(int(i) in allowed for i in got[0].ravel())
    all_rows = ix.search(0, q[:5], int(mask.sum()) if mask.sum() <= index.MAX_K else index.MAX_K, view)
    assert same(all_rows, d.search(0, q[:5], all_rows[0].shape[1]))
    view.close()
    d.close()
    ix.close()


def test_cosine_large_view_takes_the_f16_minima_pass(gpu_ctx, torch_cuda):
    """dim 64, 2^18 rows of which slightly more than 2^17 are allowed, 16 queries: the shape of the f16-minima pass (n >= 2^17,
    dim % 64 == 0, 16-byte aligned rows) on the view as on the dedicated index."""
    torch = torch_cuda
    n, dim, nq, k = 1 << 18, 64, 16, 10
    g = torch.Generator(device="cuda")
    g.manual_seed(64)
    rows = torch.randn((n, dim), dtype=torch.float32, device="cuda", generator=g)
    ids_np = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(5)
    rng = np.random.default_rng(64)
    mask = np.zeros(n, bool)
    mask[rng.choice(n, (1 << 17) + 1000, replace=False)] = True
    ids = dev_u64(torch, ids_np)
    t_mask = torch.from_numpy(mask).cuda()
    m_rows, m_ids = rows[t_mask].contiguous(), dev_u64(torch, ids_np[mask])
    q = (rows[t_mask][:nq] + 0.25 * torch.randn((nq, dim), dtype=torch.float32, device="cuda", generator=g)).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    ix = index.DeviceIndex(index.COSINE_F32, dim, index.APPEND_ONLY, gpu_ctx)
    d = index.DeviceIndex(index.COSINE_F32, dim, index.APPEND_ONLY, gpu_ctx)
    ix.append_dev(0, ids.data_ptr(), rows.data_ptr(), n, st)
    d.append_dev(0, m_ids.data_ptr(), m_rows.data_ptr(), int(mask.sum()), st)
    view = ix.filter(0, index.filter_bytes(ids_np[mask]))
    assert view.stats()["rows_allowed"] == (1 << 17) + 1000
    qh = q.cpu().numpy()
    got = ix.search(0, qh, k, view)
    assert same(got, d.search(0, qh, k))
    assert np.array_equal(got[0][:, 0], ids_np[mask][:nq])          # each query's own row comes first
    view.close()
    d.close()
    ix.close()


# ---- views ------------------------------------------------------------------------------------------------------------

class Model:
    """Row order of a mapped shard: upsert appends new ids, delete moves the last row into the hole."""

    def __init__(self):
        self.ids, self.rows = [], []

    def upsert(self, ids, rows):
        for i, r in zip(ids.tolist(), rows.tolist()):
            if i in self.ids:
                self.rows[self.ids.index(i)] = r
            else:
                self.ids.append(i)
                self.rows.append(r)

    def delete(self, ids):
        for i in ids.tolist():
            if i in self.ids:
                p = self.ids.index(i)
                self.ids[p], self.rows[p] = self.ids[-1], self.rows[-1]
                self.ids.pop()
                self.rows.pop()

    def arrays(self):
        return np.array(self.ids, np.uint64), np.array(self.rows, np.uint64)


def dev_search(torch, ix, view, q, k):
    """search_dev with the view on the current stream -> host arrays."""
    nq = q.size
    d_q = dev_u64(torch, q)
    o_ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    o_sc = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    o_d = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    o_c = torch.empty((nq,), dtype=torch.int32, device="cuda")
    ix.search_dev(0, d_q.data_ptr(), nq, k, o_ids.data_ptr(), o_sc.data_ptr(), o_d.data_ptr(), o_c.data_ptr(),
                  torch.cuda.current_stream().cuda_stream, view)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_sc.cpu().numpy(), o_d.cpu().numpy().view(np.uint32),
            o_c.cpu().numpy().view(np.uint32))


def test_view_goes_stale_after_upsert_delete_and_load(gpu_ctx, torch_cuda, tmp_path):
    rng = np.random.default_rng(21)
    n = 500
    ids = rng.permutation(np.arange(n, dtype=np.uint64) + np.uint64(1000))
    codes = rng.integers(0, 2**64, n, dtype=np.uint64)
    q = rng.integers(0, 2**64, 3, dtype=np.uint64)
    allowed = np.arange(900, 1700, 2, dtype=np.uint64)            # includes ids the shard gets only later
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    model = Model()
    ix.upsert(0, ids, codes)
    model.upsert(ids, codes)
    view = make_view(ix, index.filter_bytes(allowed))
    snapshot = str(tmp_path / "other.idx")
    other = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    other.upsert(0, np.array([1600, 1602, 1001], np.uint64), np.array([q[0], q[1], q[2]], np.uint64))
    other.save(snapshot)
    other.close()

    def current():
        m_ids, m_codes = model.arrays()
        mask = np.isin(m_ids, allowed)
        assert not view.stale
        got = dev_search(torch_cuda, ix, view, q, 8)
        d = dedicated(ix, gpu_ctx, m_ids, m_codes, mask)
        assert same(got, d.search(0, q, 8))
        d.close()
        st = view.stats()
        assert st["rows_allowed"] == int(mask.sum()) and st["rows_seen"] == m_ids.size and st["device_bytes"] >= 16 * int(mask.sum())

    def stale_then_refreshed_by_the_host_entry():
        assert view.stale
        with pytest.raises(errors.InvalidArgument, match="stale"):
            dev_search(torch_cuda, ix, view, q, 8)
        m_ids, m_codes = model.arrays()
        check(ix, gpu_ctx, view, m_ids, m_codes, q, 8, np.isin(m_ids, allowed))      # the host entry refreshes
        current()

    current()
    new_ids, new_codes = np.array([1500, 1002, 1004], np.uint64), np.array([q[0] ^ np.uint64(1), q[1], 77], np.uint64)
    ix.upsert(0, new_ids, new_codes)                               # 1500 is new and allowed; 1002 and 1004 change their codes
    model.upsert(new_ids, new_codes)
    stale_then_refreshed_by_the_host_entry()
    gone = np.array([1002, 1003, int(model.ids[0]), 5], np.uint64)
    assert ix.delete(0, gone) == 3
    model.delete(gone)
    stale_then_refreshed_by_the_host_entry()
    ix.load(snapshot)
    model.upsert(np.array([1600, 1602, 1001], np.uint64), np.array([q[0], q[1], q[2]], np.uint64))
    stale_then_refreshed_by_the_host_entry()
    ix.upsert(1, new_ids, new_codes)                               # another tenant: the view stays current
    current()
    view.refresh()
    current()
    view.close()
    ix.close()


def test_view_goes_stale_after_append_dev(gpu_ctx, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(22)
    ids = np.arange(300, dtype=np.uint64) * np.uint64(2)
    codes = rng.integers(0, 2**64, 300, dtype=np.uint64)
    q = rng.integers(0, 2**64, 2, dtype=np.uint64)
    d_ids, d_codes = dev_u64(torch, ids), dev_u64(torch, codes)
    st = torch.cuda.current_stream().cuda_stream
    ix = index.DeviceIndex(index.HAMMING64, 0, index.APPEND_ONLY, gpu_ctx)
    ix.append_dev(0, d_ids.data_ptr(), d_codes.data_ptr(), 200, st)
    allowed = ids[::3]
    view = make_view(ix, index.filter_bytes(allowed))
    assert view.stats()["rows_allowed"] == int(np.isin(ids[:200], allowed).sum())
    ix.append_dev(0, d_ids.data_ptr() + 8 * 200, d_codes.data_ptr() + 8 * 200, 100, st)
    assert view.stale
    with pytest.raises(errors.InvalidArgument, match="stale"):
        dev_search(torch, ix, view, q, 5)
    got = ix.search(0, q, 5, view)
    b = ref.hamming_topk(ids, codes, np.isin(ids, allowed), q, 5)
    assert np.array_equal(got[0], b[0]) and np.array_equal(got[2], b[1]) and not view.stale
    assert same(got, dev_search(torch, ix, view, q, 5))
    view.close()
    ix.close()


def test_two_views_of_one_tenant_on_two_streams(ham, torch_cuda):
    torch = torch_cuda
    ix, ids, codes, q = ham["ix"], ham["ids"], ham["codes"], ham["q"][:64]
    mask_b = np.arange(ids.size) % 3 == 0
    view_b = ix.filter(0, index.filter_bytes(ids[mask_b]))
    d_q = dev_u64(torch, q)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for view, s in ((ham["view"], sa), (view_b, sb), (ham["view"], sb), (view_b, sa)):
        o = (torch.empty((64, 10), dtype=torch.int64, device="cuda"), torch.empty((64, 10), dtype=torch.int32, device="cuda"),
             torch.empty((64,), dtype=torch.int32, device="cuda"))
        ix.search_dev(0, d_q.data_ptr(), 64, 10, o[0].data_ptr(), 0, o[1].data_ptr(), o[2].data_ptr(), s.cuda_stream, view)
        outs.append(o)
    torch.cuda.synchronize()
    for j, o in enumerate(outs):
        b = ref.hamming_topk(ids, codes, ham["mask"] if j in (0, 2) else mask_b, q, 10)
        assert np.array_equal(o[0].cpu().numpy().view(np.uint64), b[0]) and np.array_equal(o[1].cpu().numpy().view(np.uint32), b[1])
    view_b.close()


def test_view_outlives_its_index_detached_and_is_refused_by_another_index(gpu_ctx):
    lib = _lib.load()
    ids = np.arange(100, dtype=np.uint64)
    codes = ids * np.uint64(0x9E3779B97F4A7C15)
    a = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    b = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    a.upsert(0, ids, codes)
    b.upsert(0, ids, codes)
    view = a.filter(0, index.filter_bytes(ids[:10]))
    with pytest.raises(errors.InvalidArgument, match="another index"):
        b.search(0, codes[:1], 3, view)
    a.close()                                              # the index goes first: the view is detached
    for call in (lambda: view.stats(), lambda: view.stale, lambda: view.refresh(), lambda: b.search(0, codes[:1], 3, view)):
        with pytest.raises(errors.InvalidArgument):
            call()
    assert lib.ucfp_index_filter_stale(None) == -4 and lib.ucfp_index_filter_refresh(None) == -4
    assert lib.ucfp_index_filter_stats(None, None, None, None, None) == -4
    lib.ucfp_index_filter_destroy(None)
    view.close()
    b.close()


def test_argument_checks_k0_nq0_unknown_tenant_and_empty_filter(gpu_ctx):
    lib = _lib.load()
    ids = np.arange(100, dtype=np.uint64)
    codes = ids * np.uint64(0x9E3779B97F4A7C15)
    ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    ix.upsert(0, ids, codes)
    view = ix.filter(0, ids[:10].tolist())                 # an iterable of ids
    q = codes[:2].copy()
    o_ids, o_c = np.zeros((2, 4), np.uint64), np.full(2, 9, np.uint32)
    args = (q.ctypes.data, 2, 4, o_ids.ctypes.data, None, None, o_c.ctypes.data)
    assert lib.ucfp_index_search_filtered(None, view.handle, *args) == -4
    assert lib.ucfp_index_search_filtered(ix.handle, None, *args) == -4
    assert lib.ucfp_index_search_filtered(ix.handle, view.handle, q.ctypes.data, 2, index.MAX_K + 1, o_ids.ctypes.data, None, None,
                                          o_c.ctypes.data) == -4
    assert lib.ucfp_index_search_filtered(ix.handle, view.handle, None, 2, 4, o_ids.ctypes.data, None, None, o_c.ctypes.data) == -4
    assert lib.ucfp_index_search_filtered_dev(ix.handle, None, None, 0, 4, None, None, None, None, None) == -4
    assert lib.ucfp_index_search_filtered(ix.handle, view.handle, None, 0, 4, None, None, None, None) == 0            # nq = 0
    assert lib.ucfp_index_search_filtered(ix.handle, view.handle, q.ctypes.data, 2, 0, o_ids.ctypes.data, None, None,
                                          o_c.ctypes.data) == 0 and (o_c == 0).all()                                   # k = 0
    h = C.c_void_p()
    assert lib.ucfp_index_filter_create(ix.handle, 0, None, 8, C.byref(h)) == -4
    assert lib.ucfp_index_filter_create(None, 0, b"\0" * 8, 8, C.byref(h)) == -4
    with pytest.raises(errors.InvalidArgument, match="at byte"):
        ix.filter(0, b"\x01" + b"\0" * 7)
    with pytest.raises(errors.InvalidArgument):
        ix.search(1, q, 4, view)                           # the view is tenant 0's
    unfiltered = ix.search(0, q, 4)
    for v in (ix.filter(5, index.filter_bytes(ids)), ix.filter(0, index.filter_bytes([]))):     # unknown tenant; empty filter
        assert v.stats()["rows_allowed"] == 0
        got = ix.search(v.tenant, q, 4, v)
        assert same(got, ix.search(77, q, 4)) and (got[3] == 0).all() and (got[0] == INVALID).all()
        v.close()
    assert same(ix.search(0, q, 4), unfiltered)
    view.close()
    ix.close()


# ---- Python facade ----------------------------------------------------------------------------------------------------

def test_gpu_index_honours_query_filters(gpu_ctx):
    from ucfp_amd.core import Modality, QueryRequest
    rng = np.random.default_rng(40)
    n, dim = 400, 16
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    hashes = rng.integers(0, 2**64, n, dtype=np.uint64)
    space = "imgfprint-phash-v1"
    g = index.GpuIndex(gpu_ctx)
    g._cosine(dim).upsert(3, np.arange(n, dtype=np.uint64), emb)
    g._hamming(space).upsert(3, np.arange(n, dtype=np.uint64), hashes)
    allowed = np.arange(0, n, 7, dtype=np.uint64)
    data = index.filter_bytes(allowed)
    cos, hamx = g._cos[dim], g._ham[space]
    v_cos, v_ham = cos.filter(3, data), hamx.filter(3, data)
    c_ids, c_sc, _, c_cnt = cos.search(3, emb[5][None, :], 10, v_cos)
    hits = g.knn(3, emb[5], 10, data)
    assert [h.record_id for h in hits] == c_ids[0, :int(c_cnt[0])].tolist()
    assert [np.float32(h.score) for h in hits] == c_sc[0, :int(c_cnt[0])].tolist()
    assert all(h.record_id % 7 == 0 for h in hits) and len(hits) == 10
    h_ids, _, h_d, h_cnt = hamx.search(3, hashes[14:15], 10, v_ham)
    hits = g.hamming(3, space, int(hashes[14]), 10, filter=data)
    assert [h.record_id for h in hits] == h_ids[0].tolist() and [h.distance for h in hits] == h_d[0].tolist()
    assert hits[0].record_id == 14 and hits[0].distance == 0
    req = QueryRequest(tenant_id=3, modality=Modality.Image, k=10, vector=emb[5].tolist(), filter=data)
    assert [h.record_id for h in g.query(req)] == c_ids[0].tolist()
    req = QueryRequest(tenant_id=3, modality=Modality.Image, k=10, hash=int(hashes[14]), algorithm=space, filter=data)
    assert [h.record_id for h in g.query(req)] == h_ids[0].tolist()
    # without a filter: today's answers
    u_ids, _, _, _ = cos.search(3, emb[5][None, :], 10)
    assert [h.record_id for h in g.knn(3, emb[5], 10)] == u_ids[0].tolist() and u_ids[0, 0] == 5
    assert [h.record_id for h in g.query(QueryRequest(tenant_id=3, modality=Modality.Image, k=10, vector=emb[5].tolist()))] \
        == u_ids[0].tolist()
    assert g.hamming(3, space, int(hashes[15]), 10)[0].record_id == 15
    # a hybrid query with a filter raises as before; so does a filter on an index that takes none
    with pytest.raises(errors.UnsupportedError):
        g.query(QueryRequest(tenant_id=3, modality=Modality.Text, k=5, vector=emb[5].tolist(), terms=["whale"], filter=data))
    with pytest.raises(errors.UnsupportedError):
        g.query(QueryRequest(tenant_id=3, modality=Modality.Text, k=5, tlsh=b"\0" * 35, filter=data))
    with pytest.raises(errors.InvalidArgument):
        g.knn(3, emb[5], 10, [1, 2, 3])
    # the cache: at most MAX_VIEWS views, least recently used out; a stale one is refreshed by the search
    (first,) = [v for v in g._views.values() if v.index is cos]
    assert len(g._views) == 2
    cos.upsert(3, np.array([399], np.uint64), emb[5][None, :])         # 399 = 7 * 57: allowed, and now the twin of row 5
    assert first.stale
    hits = g.knn(3, emb[5], 10, data)
    assert hits[0].record_id == 399 and not first.stale       # (row 5 itself is not allowed)
    for j in range(index.MAX_VIEWS):
        g.knn(3, emb[5], 3, index.filter_bytes(allowed[: j + 2]))
    assert len(g._views) == index.MAX_VIEWS and first.handle is None              # evicted and closed
    assert len(g.knn(3, emb[5], 10, data)) == 10


# ---- no writes past the end -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["hamming", "cosine"])
def test_outputs_are_not_written_past_their_end(gpu_ctx, torch_cuda, kind):
    torch = torch_cuda
    rng = np.random.default_rng(50)
    n, dim, nq, k = 5000, 21, 9, 7          # dim % 4 != 0: the 4-byte gather
    ids = rng.permutation(np.arange(n, dtype=np.uint64) + np.uint64(1))
    if kind == "hamming":
        ix = index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
        rows = rng.integers(0, 2**64, n, dtype=np.uint64)
        q = dev_u64(torch, rows[:nq])
    else:
        ix = index.DeviceIndex(index.COSINE_F32, dim, 0, gpu_ctx)
        rows = rng.standard_normal((n, dim)).astype(np.float32)
        q = torch.from_numpy(rows[:nq].copy()).cuda()
    ix.upsert(0, ids, rows)
    view = ix.filter(0, index.filter_bytes(ids[::2], runs=True))
    guard = 4096
    sizes = [nq * k * 8, nq * k * 4, nq * k * 4, nq * 4]
    bufs = [torch.full((guard + s + guard,), 0xA5, dtype=torch.uint8, device="cuda") for s in sizes]
    ptrs = [b.data_ptr() + guard for b in bufs]
    ix.search_dev(0, q.data_ptr(), nq, k, ptrs[0], ptrs[1], ptrs[2], ptrs[3], torch.cuda.current_stream().cuda_stream, view)
    torch.cuda.synchronize()
    for b, s in zip(bufs, sizes):
        h = b.cpu().numpy()
        assert (h[:guard] == 0xA5).all() and (h[guard + s:] == 0xA5).all()
    view.check_guards()
    got_ids = bufs[0].cpu().numpy()[guard:guard + sizes[0]].view(np.uint64).reshape(nq, k)
    want = ix.search(0, rows[:nq], k, view)
    assert np.array_equal(got_ids, want[0])
    view.close()
    ix.close()


@pytest.mark.parametrize("kind", ["hamming", "hamming_append_only", "cosine_dim20", "cosine_dim21", "cosine_dim768"])
def test_view_buffers_are_not_written_past_their_ends(gpu_ctx, torch_cuda, kind):
    """The view's ids, rows, norms and ids-ascend state lie between guard patterns, its masks and counts have one behind
    them (ucfp_index_filter_check): intact after the build, after searches, after a refresh -- at shard sizes around the
    tile, for the 16-byte and the 4-byte cosine gather, with the allowed rows at both ends of the shard."""
    torch = torch_cuda
    rng = np.random.default_rng(60)
    st = torch.cuda.current_stream().cuda_stream
    hamming = kind.startswith("hamming")
    dim = 0 if hamming else int(kind.split("dim")[1])
    flags = index.APPEND_ONLY if kind == "hamming_append_only" else 0
    for n in (1, 64, 65, 4099):
        ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)
        rows = rng.integers(0, 2**64, n, dtype=np.uint64) if hamming else rng.standard_normal((n, dim)).astype(np.float32)
        ix = index.DeviceIndex(index.HAMMING64 if hamming else index.COSINE_F32, dim, flags, gpu_ctx)
        if flags:
            d_ids, d_rows = dev_u64(torch, ids), dev_u64(torch, rows)
            ix.append_dev(0, d_ids.data_ptr(), d_rows.data_ptr(), n, st)
        else:
            ix.upsert(0, ids, rows)
        for mask in (np.ones(n, bool), np.arange(n) % 2 == 0, np.arange(n) == n - 1, np.arange(n) >= n - min(n, 70)):
            view = ix.filter(0, ref.write_ids(ids[mask].tolist(), mixed_kind(rng)))
            view.check_guards()
            assert view.stats()["rows_allowed"] == int(mask.sum())
            for nq in (1, 9):
                got = ix.search(0, rows[:1].repeat(nq, axis=0) if not hamming else np.repeat(rows[:1], nq), 5, view)
                assert (got[3] == min(5, int(mask.sum()))).all()
            view.check_guards()
            view.refresh()
            view.check_guards()
            ms = view.build_ms()
            assert set(ms) == {"probe", "scan", "readback", "gather"} and all(v > 0 for v in ms.values())
            view.close()
        empty = ix.filter(0, index.filter_bytes([1]))            # a view of 0 rows: nothing to guard but the scratch
        empty.check_guards()
        assert empty.build_ms() == {"probe": 0.0, "scan": 0.0, "readback": 0.0, "gather": 0.0}
        empty.close()
        ix.close()
