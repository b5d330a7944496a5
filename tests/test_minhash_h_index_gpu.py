"""Exact search over MinHash records of any slot count H (minhash_index.hip): ids, agree, score bytes
and counts equal the restatement (tests/minhash_h_ref.py).  Rows are built from the queries by copying a chosen number of
their slots, so every agreement is known by construction: 0, H, and several rows at the same value (ties by id).  Row
counts sit around a 64-row group and a 512-row block, query counts take every arm of the dispatch, H takes one chunk of
128 slots with pad (16, 64), two (144, 256) and eight (1024)."""

import numpy as np
import pytest

import minhash_h_ref as ref

pytestmark = pytest.mark.gpu

HS = [16, 64, 144, 256, 1024]
NS = [1, 63, 65, 513]
NQS = [1, 5, 17, 33, 65]
N_MAX, NQ_MAX = 513, 65


def _ids(rng, n):
    """A shuffled multiple of 0x9E3779B1 beyond 2^32: row order is not id order."""
    return rng.permutation((np.arange(n, dtype=np.uint64) + np.uint64(5)) * np.uint64(0x9E3779B1))


def _build(h, seed=0):
    """Queries, rows and the agreement matrix.  Row r copies `want[r]` slots of query r % NQ_MAX (the others are the query's
    slot with one bit flipped, so they differ from it; against the other queries a row agrees nowhere, their slots being
    independent draws).  want takes 0, h and runs of equal values."""
    rng = np.random.default_rng(1000 * h + seed)
    q = rng.integers(0, 1 << 64, (NQ_MAX, h), dtype=np.uint64)
    levels = np.array([0, h, h // 2, h // 2, h // 2, 1, h - 1, h - 1, 3, h], np.int64)
    want = levels[rng.integers(0, levels.size, N_MAX)]
    want[:10] = levels                                    # every level is present from n = 63 on; row 0 agrees nowhere
    rows = np.empty((N_MAX, h), np.uint64)
    for r in range(N_MAX):
        src = q[r % NQ_MAX]
        flip = np.uint64(1) << rng.integers(0, 64, h).astype(np.uint64)
        rows[r] = src ^ flip
        keep = rng.permutation(h)[:want[r]]
        rows[r, keep] = src[keep]
    qrec = ref.records_of(q, h, header=rng.integers(0, 256, (NQ_MAX, 8), dtype=np.uint8))   # headers take no part
    rrec = ref.records_of(rows, h)
    A = ref.agree_matrix(qrec, rrec, h)
    assert all(A[r % NQ_MAX, r] == want[r] for r in range(N_MAX))
    return qrec, rrec, _ids(rng, N_MAX), A


@pytest.fixture(scope="module")
def pools():
    return {h: _build(h) for h in HS}


def _check(got, want, k):
    g_ids, g_a, g_s, g_n = got
    w_ids, w_a, w_s, w_n = want
    assert g_ids.shape == g_a.shape == g_s.shape == (w_n.size, k)
    assert np.array_equal(g_n, w_n), (g_n[:8], w_n[:8])
    assert np.array_equal(g_a, w_a), np.argwhere(g_a != w_a)[:4]
    assert np.array_equal(g_ids, w_ids), np.argwhere(g_ids != w_ids)[:4]
    assert g_s.tobytes() == w_s.tobytes()


@pytest.mark.parametrize("h", HS)
def test_sizes_arms_and_cuts(gpu_ctx, pools, h):
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.index import MinHashIndex
    qrec, rrec, ids, A = pools[h]
    for n in NS:
        ix = MinHashIndex(ctx=gpu_ctx, h=h)
        assert ix.h == h and int(ix._lib.ucfp_minhash_index_slots(ix.handle)) == h
        ix.upsert(5, ids[:n], rrec[:n])
        assert ix.size(5) == n
        for nq in NQS:
            for min_agree in (0, 1, h):
                k = 7 if nq > 5 else 128                   # 128 (the largest k) > n for the three small row counts
                got = ix.query(5, qrec[:nq], k, min_agree)
                _check(got, ref.topk_from_agree(ids[:n], A[:nq, :n], h, k, min_agree), k)
                if min_agree == 0:
                    assert (got[3] == min(n, k)).all()
        with pytest.raises(InvalidArgument):
            ix.query(5, qrec[:1], 5, h + 1)
        with pytest.raises(InvalidArgument):               # the C ABI's own refusal, behind the wrapper's
            _raw_query(ix, qrec[:1], 5, h + 1)
        ix.close()


def _raw_query(ix, q, k, min_agree):
    from ucfp_amd import _lib
    q = np.ascontiguousarray(q)
    nq = q.shape[0]
    ids, agree = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.uint32)
    scores, counts = np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)
    _lib.check(ix._lib.ucfp_minhash_index_query(ix.handle, 5, q.ctypes.data, nq, k, min_agree, ids.ctypes.data, agree.ctypes.data,
                                                scores.ctypes.data, counts.ctypes.data))
    return ids, agree, scores, counts


@pytest.mark.parametrize("h", [16, 144, 1024])
def test_pass_loop(gpu_ctx, pools, h, monkeypatch):
    """UCFP_MINHASH_KEY_BYTES small: 4096 bytes of keys hold one query over 513 rows, so 17 queries take 17 passes."""
    from ucfp_amd.index import MinHashIndex
    qrec, rrec, ids, A = pools[h]
    monkeypatch.setenv("UCFP_MINHASH_KEY_BYTES", "4096")
    ix = MinHashIndex(ctx=gpu_ctx, h=h)
    monkeypatch.delenv("UCFP_MINHASH_KEY_BYTES")
    ix.upsert(0, ids, rrec)
    for k in (3, 40):
        _check(ix.query(0, qrec[:17], k, 1), ref.topk_from_agree(ids, A[:17], h, k, 1), k)
    ix.close()


@pytest.mark.parametrize("h", [64, 256])
def test_upsert_delete_query_and_the_device_entries(gpu_ctx, torch_cuda, pools, h):
    from ucfp_amd.index import MinHashIndex
    torch = torch_cuda
    qrec, rrec, ids, A = pools[h]
    n = 130
    ix = MinHashIndex(ctx=gpu_ctx, h=h)
    d_ids = torch.from_numpy(ids[:n].view(np.int64).copy()).cuda()
    d_rows = torch.from_numpy(rrec[:n].copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    ix.upsert_dev(1, d_ids.data_ptr(), d_rows.data_ptr(), n, stream)
    _check(ix.query(1, qrec[:5], 9, 0), ref.topk_from_agree(ids[:n], A[:5, :n], h, 9, 0), 9)
    # a known id replaces its row; deleted rows are gone; another tenant sees nothing of it
    ix.upsert(1, ids[3:4], rrec[200:201])
    A2 = A[:, :n].copy()
    A2[:, 3] = A[:, 200]
    _check(ix.query(1, qrec[:5], 9, 0), ref.topk_from_agree(ids[:n], A2[:5], h, 9, 0), 9)
    gone = np.arange(0, n, 3)
    assert ix.delete(1, np.concatenate([ids[gone], [np.uint64(1)]])) == gone.size
    left = np.setdiff1d(np.arange(n), gone)
    _check(ix.query(1, qrec[:17], 9, 1), ref.topk_from_agree(ids[left], A2[:17][:, left], h, 9, 1), 9)
    assert ix.query(2, qrec[:2], 4)[3].tolist() == [0, 0]
    # the device query entry, records and answers on the device
    nq, k = 6, 5
    d_q = torch.from_numpy(qrec[:nq].copy()).cuda()
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_a = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    ix.query_dev(1, d_q.data_ptr(), nq, k, 1, o_ids.data_ptr(), o_a.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), stream)
    torch.cuda.synchronize()
    got = (o_ids.cpu().numpy().view(np.uint64), o_a.cpu().numpy().view(np.uint32), o_s.cpu().numpy(), o_n.cpu().numpy().view(np.uint32))
    _check(got, ref.topk_from_agree(ids[left], A2[:nq][:, left], h, k, 1), k)
    ix.close()


def test_a_128_slot_handle_is_what_it_was(gpu_ctx):
    """create, create_h(128) and MinHashIndex() answer alike, byte for byte, and take 1032-byte records only."""
    import ctypes as C
    import minhash_index_ref as ref128
    from ucfp_amd import _lib
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.index import MinHashIndex
    rng = np.random.default_rng(3)
    base = rng.integers(0, 1 << 64, 128, dtype=np.uint64)
    flips = np.array([0, 1, 1 << 32, 1 << 63], np.uint64)
    rows = ref128.records_of(base[None, :] ^ flips[rng.integers(0, 4, (200, 128))])
    queries = ref128.records_of(base[None, :] ^ flips[rng.integers(0, 4, (17, 128))])
    ids = _ids(rng, 200)
    want = ref128.topk_from_agree(ids, ref128.agree_matrix(queries, rows), 10, 1)
    a, b = MinHashIndex(ctx=gpu_ctx), MinHashIndex(ctx=gpu_ctx, h=128)
    lib = _lib.load()
    old = C.c_void_p()
    _lib.check(lib.ucfp_minhash_index_create(gpu_ctx.handle, 0, C.byref(old)))
    assert int(lib.ucfp_minhash_index_slots(old)) == 128 and a.h == b.h == 128
    lib.ucfp_minhash_index_destroy(old)
    for ix in (a, b):
        ix.upsert(0, ids, rows)
        _check(ix.query(0, queries, 10), want, 10)
        _check(ix.query(0, queries, 10, 128), ref128.topk_from_agree(ids, ref128.agree_matrix(queries, rows), 10, 128), 10)
        assert np.array_equal(ix.query(0, queries[:1], 3)[2], want[2][:1, :3])
        with pytest.raises(InvalidArgument):
            ix.query(0, queries, 10, 129)
        with pytest.raises(InvalidArgument):
            ix.upsert(0, ids[:2], np.zeros((2, 520), np.uint8))
        ix.close()


def test_gpu_index_files_records_by_slot_count(gpu_ctx, tmp_path):
    from ucfp_amd import store, text
    from ucfp_amd.core import Modality, QueryRequest, Record
    from ucfp_amd.index import GpuIndex
    words = ["w%d" % i for i in range(400)]
    rng = np.random.default_rng(9)
    n = 12
    docs = [" ".join(words[j] for j in rng.integers(0, 400, 80)) for _ in range(n)]
    edited = [d.replace(d.split()[3], "edited", 1) for d in docs]
    tag = text.ALGORITHM_MINHASH_128
    r64, s64 = text.minhash_batch(docs, text.TextOpts(h=64), gpu_ctx)
    r128, s128 = text.minhash_batch(docs, text.TextOpts(), gpu_ctx)
    e64, _ = text.minhash_batch(edited, text.TextOpts(h=64), gpu_ctx)
    e128, _ = text.minhash_batch(edited, text.TextOpts(), gpu_ctx)
    assert not s64.any() and not s128.any() and r64.shape == (n, 520) and r128.shape == (n, 1032)

    def rec(rid, fp):
        return Record(tenant_id=3, record_id=rid, modality=Modality.Text, format_version=1, algorithm=tag, config_hash=0,
                      fingerprint=fp.tobytes())

    path = str(tmp_path / "side.log")
    gi = GpuIndex(gpu_ctx, sidecar=store.Sidecar(path))
    gi.upsert([rec(100 + i, r64[i]) for i in range(n)] + [rec(200 + i, r128[i]) for i in range(n)])

    def check(index):
        assert sorted(index._minhash_keys()) == [(tag, 64), (tag, 128)]
        assert index._minhash_get(tag, 64).size(3) == n and index._minhash_get(tag, 128).size(3) == n
        for i in (0, 5, 11):
            w = ref.topk_h(np.arange(100, 100 + n, dtype=np.uint64), r64, e64[i:i + 1], 64, 4, 1)
            for hits in (index.similar_text(3, e64[i].tobytes(), 4),
                         index.query(QueryRequest.from_json({"tenant_id": 3, "modality": "Text", "k": 4, "minhash": e64[i].tobytes().hex()}))):
                assert hits[0].record_id == 100 + i
                assert [h.record_id for h in hits] == w[0][0, :int(w[3][0])].tolist()
                assert [h.distance for h in hits] == [64 - int(a) for a in w[1][0, :int(w[3][0])]]
                assert [np.float32(h.score) for h in hits] == w[2][0, :int(w[3][0])].tolist()
            assert index.similar_text(3, e128[i].tobytes(), 4)[0].record_id == 200 + i
            assert index.similar_text(3, edited[i], 4)[0].record_id == 200 + i          # a text is fingerprinted at the default H
        assert index.similar_text(3, bytes(8 + 8 * 256), 4, min_agree=0) == []           # no record of H = 256 was stored

    check(gi)
    gi.flush()
    check(store.rebuild(path, gpu_ctx))
    # overwrite rule: a key re-ingested at another H changes index
    gi.upsert([rec(100, r128[0])])
    assert gi._minhash_get(tag, 64).size(3) == n - 1 and gi._minhash_get(tag, 128).size(3) == n + 1
    gi.delete(3, [101, 201])
    assert gi._minhash_get(tag, 64).size(3) == n - 2 and gi._minhash_get(tag, 128).size(3) == n
