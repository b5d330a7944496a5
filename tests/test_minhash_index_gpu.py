"""MinHash search on the device (minhash_index.hip): ids, agree, score bytes and counts equal the exact top-k
by (agree descending, id ascending) of the restatement (tests/minhash_index_ref.py) -- over rows whose slots come from four
values per position (so agreements spread around 32 with many ties and every disagreement sits in one dword half), rows
planted at every agreement 0 .. 128, the agreement cut, the pass loop, tenants, mutations, the device entry points, the
LSH shard over the same rows, and end to end from text.minhash_batch through GpuIndex.query and store.rebuild."""
import numpy as np
import pytest

import minhash_index_ref as ref

pytestmark = pytest.mark.gpu

INVALID_ID = 0xFFFFFFFFFFFFFFFF
N_POOL, NQ_POOL = 1000, 65
N_SLICES = 513        # ucfp::select_plan(n, 3): slices = min(ceil(4096 / 3), (n + 511) / 512) -> 2 from n = 513 on
N_TREE = 32_769       # the same plan gives 65 slices, one more than the fan-in of a merge-tree level
FLIPS = np.array([0, 1, 1 << 32, 1 << 63], np.uint64)


def _draw(rng, base, n):
    """n records: slot i is base_i, base_i ^ 1, base_i ^ 2^32 or base_i ^ 2^63; random headers, which take no part."""
    slots = base[None, :] ^ FLIPS[rng.integers(0, 4, (n, 128))]
    return ref.records_of(slots, header=rng.integers(0, 256, (n, 8), dtype=np.uint8))


def _ids(rng, n):
    """A shuffled multiple of 0x9E3779B1 beyond 2^32: row order is not id order."""
    return rng.permutation((np.arange(n, dtype=np.uint64) + np.uint64(5)) * np.uint64(0x9E3779B1))


@pytest.fixture(scope="module")
def pool():
    """Rows, ids, queries and the restatement's agreement matrix, computed once and shared."""
    rng = np.random.default_rng(17)
    base = rng.integers(0, 1 << 64, 128, dtype=np.uint64)
    rows, queries = _draw(rng, base, N_POOL), _draw(rng, base, NQ_POOL)
    ids = _ids(rng, N_POOL)
    assert int(ids.min()) > 1 << 32
    A = ref.agree_matrix(queries, rows)
    assert 20 < A.mean() < 44 and len(np.unique(A[0])) < 60       # many ties
    return rows, ids, queries, A


def _check(got, want, k):
    g_ids, g_a, g_s, g_n = got
    w_ids, w_a, w_s, w_n = want
    assert g_ids.shape == g_a.shape == g_s.shape == (w_n.size, k)
    assert np.array_equal(g_n, w_n), (g_n[:8], w_n[:8])
    assert np.array_equal(g_a, w_a), np.argwhere(g_a != w_a)[:4]
    assert np.array_equal(g_ids, w_ids), np.argwhere(g_ids != w_ids)[:4]
    assert g_s.tobytes() == w_s.tobytes()


# nq = 1, 4 | 5, 16 | 17, 32 | 33 are the sizes at which mh_keys changes its query tile (1, 4, 16 queries per wave, then two
# and four waves of 16); 64 | 65 is the edge of a block's 64 queries; n = 512 | 513 the edge of a block's rows
NQS = [1, 3, 4, 5, 15, 16, 17, 32, 33, 64, 65]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 512, 1000])
def test_sizes(gpu_ctx, pool, n):
    from ucfp_amd.index import MinHashIndex
    rows, ids, queries, A = pool
    ix = MinHashIndex(ctx=gpu_ctx)
    ix.upsert(5, ids[:n], rows[:n])
    assert ix.size(5) == n
    for nq in NQS:
        for k in (1, 10, 128):
            got = ix.query(5, queries[:nq], k)
            _check(got, ref.topk_from_agree(ids[:n], A[:nq, :n], k), k)
            if k > n:      # the pool has no all-disagreeing pair at these sizes, so every row is a hit
                assert (A[:nq, :n] > 0).all()
                assert (got[3] == n).all() and (got[0][:, n:] == INVALID_ID).all() and (got[2][:, n:] == -1.0).all()
                assert (got[1][:, n:] == 0xFFFFFFFF).all()
    ix.close()


@pytest.mark.parametrize("n", [N_SLICES, N_TREE])
def test_several_slices(gpu_ctx, n):
    """Row counts at which the selector cuts the rows into 2 slices, and into 65 (two levels of the merge tree)."""
    from ucfp_amd.index import MinHashIndex
    rng = np.random.default_rng(n)
    base = rng.integers(0, 1 << 64, 128, dtype=np.uint64)
    rows, queries, ids = _draw(rng, base, n), _draw(rng, base, 3), _ids(rng, n)
    A = ref.agree_matrix(queries, rows)
    ix = MinHashIndex(ctx=gpu_ctx)
    ix.upsert(0, ids, rows)
    for k in (10, 128):
        _check(ix.query(0, queries, k), ref.topk_from_agree(ids, A, k), k)
    ix.close()


def test_planted_agreements(gpu_ctx):
    """Rows at every agreement 0 .. 128 with one query (128 - a slots changed, each in one dword half), some of them
    under several ids: every value is reported exactly, and equal rows come in id order."""
    from ucfp_amd.index import MinHashIndex
    rng = np.random.default_rng(19)
    q = rng.integers(0, 1 << 64, 128, dtype=np.uint64)
    rows = np.tile(q, (129, 1))
    for a in range(129):
        pos = rng.choice(128, 128 - a, replace=False)
        rows[a, pos] ^= FLIPS[rng.integers(1, 4, pos.size)]
    dup = [128, 128, 100, 77, 77, 77, 1, 0, 0]
    slots = np.concatenate([rows, rows[dup]])
    agree = np.array(list(range(129)) + dup)
    recs, qrec = ref.records_of(slots), ref.records_of(q[None, :], header=np.full((1, 8), 0xAB, np.uint8))
    ids = _ids(rng, slots.shape[0])
    A = ref.agree_matrix(qrec, recs)
    assert np.array_equal(A[0], agree)
    ix = MinHashIndex(ctx=gpu_ctx)
    ix.upsert(1, ids, recs)                    # every row: the best 128 of 138
    low = agree <= 100
    ix.upsert(2, ids[low], recs[low])          # the rows at 0 .. 100: all 108 of them
    for min_agree in (0, 1):
        got = ix.query(1, qrec, 128, min_agree)
        _check(got, ref.topk_from_agree(ids, A, 128, min_agree), 128)
        assert got[1][0, :3].tolist() == [128, 128, 128] and got[0][0, 0] < got[0][0, 1] < got[0][0, 2]
        assert got[2][0, 0] == 1.0
    got = ix.query(2, qrec, 128, 0)
    _check(got, ref.topk_from_agree(ids[low], A[:, low], 128, 0), 128)
    assert int(got[3][0]) == int(low.sum()) == 108
    assert sorted(set(got[1][0, :108].tolist())) == list(range(101))
    assert int(ix.query(2, qrec, 128, 1)[3][0]) == 105        # the three rows at 0 are out
    ix.close()


def test_min_agree(gpu_ctx, pool):
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.index import MinHashIndex
    rows, ids, queries, A = pool
    rows = rows.copy()
    rows[7, 8:] = queries[2, 8:]               # an exact copy of query 2 (another header)
    A = A.copy()
    A[:, 7] = ref.agree_matrix(queries, rows[7:8])[:, 0]
    assert A[2, 7] == 128 and (np.delete(A[2], 7) < 128).all()
    ix = MinHashIndex(ctx=gpu_ctx)
    ix.upsert(0, ids, rows)
    q = queries[:5]
    for min_agree in (0, 1, 32, 40, 128):
        for k in (10, 128):
            _check(ix.query(0, q, k, min_agree), ref.topk_from_agree(ids, A[:5], k, min_agree), k)
    got = ix.query(0, q, 10, 128)
    assert got[3].tolist() == [0, 0, 1, 0, 0] and int(got[0][2, 0]) == int(ids[7])
    with pytest.raises(InvalidArgument):
        ix.query(0, q, 10, 129)
    with pytest.raises(InvalidArgument):
        ix.query(0, q, 129, 1)
    ix.close()
    # rows that agree nowhere: min_agree = 0 still makes every row a hit, in id order
    rng = np.random.default_rng(23)
    strangers = ref.records_of(rng.integers(0, 1 << 64, (300, 128), dtype=np.uint64))
    s_ids = _ids(rng, 300)
    ix = MinHashIndex(ctx=gpu_ctx)
    ix.upsert(0, s_ids, strangers)
    g_ids, g_a, g_s, g_n = ix.query(0, queries[:1], 128, 0)
    assert g_ids[0].tolist() == sorted(s_ids.tolist())[:128] and not g_a.any() and not g_s.any() and g_n.tolist() == [128]
    assert ix.query(0, queries[:1], 128)[3].tolist() == [0]       # the default cut is 1
    ix.close()


def test_pass_loop(gpu_ctx, pool, monkeypatch):
    """A key matrix smaller than the batch: 7 queries over 300 rows in passes of 3, 3 and 1."""
    from ucfp_amd.index import MinHashIndex
    rows, ids, queries, A = pool
    monkeypatch.setenv("UCFP_MINHASH_KEY_BYTES", "4096")
    ix = MinHashIndex(ctx=gpu_ctx)
    monkeypatch.delenv("UCFP_MINHASH_KEY_BYTES")
    one = MinHashIndex(ctx=gpu_ctx)
    for x in (ix, one):
        x.upsert(0, ids[:300], rows[:300])
    for k in (10, 128):
        got = ix.query(0, queries[:7], k)
        _check(got, ref.topk_from_agree(ids[:300], A[:7, :300], k), k)
        _check(got, one.query(0, queries[:7], k), k)
    ix.close()
    one.close()


def test_tenants_mutations_and_empty_answers(gpu_ctx, pool):
    from ucfp_amd.index import MinHashIndex
    rows, ids, queries, A = pool
    ix = MinHashIndex(ctx=gpu_ctx)
    a_ids, b_ids = ids[:300], ids[300:500]
    ix.upsert(1, a_ids, rows[:300])
    ix.upsert(2, b_ids, [r.tobytes() for r in rows[300:500]])          # a list of bytes
    assert (ix.size(1), ix.size(2), ix.size(3)) == (300, 200, 0)
    q = queries[:5]
    _check(ix.query(1, q, 10), ref.topk_from_agree(a_ids, A[:5, :300], 10), 10)
    _check(ix.query(2, q.tobytes(), 10), ref.topk_from_agree(b_ids, A[:5, 300:500], 10), 10)      # records back to back
    # unknown tenant, k = 0, nq = 0
    e_ids, e_a, e_s, e_n = ix.query(9, q, 10)
    assert (e_ids == INVALID_ID).all() and (e_a == 0xFFFFFFFF).all() and (e_s == -1.0).all() and not e_n.any()
    assert not ix.query(1, q, 0)[3].any()
    assert ix.query(1, np.zeros((0, 1032), np.uint8), 10)[3].shape == (0,)
    # upsert of a known id replaces its row: the best row of query 0 becomes a copy of query 1, and the answers follow
    first = int(ix.query(1, q[:1], 1)[0][0, 0])
    pos = int(np.flatnonzero(a_ids == np.uint64(first))[0])
    changed = rows[:300].copy()
    changed[pos] = queries[1]
    ix.upsert(1, a_ids[pos:pos + 1], changed[pos:pos + 1])
    assert ix.size(1) == 300
    _check(ix.query(1, q, 10), ref.topk_from_agree(a_ids, ref.agree_matrix(q, changed), 10), 10)
    top = ix.query(1, q[1:2], 1)
    assert int(top[0][0, 0]) == first and int(top[1][0, 0]) == 128
    # delete: known ids go, unknown ones are not counted, the other tenant is untouched
    gone = a_ids[:50]
    assert ix.delete(1, np.concatenate([gone, np.array([1], np.uint64)])) == 50 and ix.delete(1, gone) == 0
    assert (ix.size(1), ix.size(2)) == (250, 200)
    ix.flush()
    _check(ix.query(1, q, 10), ref.topk_from_agree(a_ids[50:], ref.agree_matrix(q, changed[50:]), 10), 10)
    _check(ix.query(2, q, 10), ref.topk_from_agree(b_ids, A[:5, 300:500], 10), 10)
    assert ix.delete(2, b_ids) == 200 and not ix.query(2, q, 10)[3].any()       # an emptied tenant
    ix.close()


def test_device_entry_points(gpu_ctx, torch_cuda, pool):
    from ucfp_amd.index import MinHashIndex
    torch = torch_cuda
    rows, ids, queries, A = pool
    n, nq, k = 777, 33, 10
    d_ids = torch.from_numpy(ids[:n].view(np.int64).copy()).cuda()
    d_rows = torch.from_numpy(rows[:n].copy()).cuda()
    d_q = torch.from_numpy(queries[:nq].copy()).cuda()
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_a = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    ix = MinHashIndex(ctx=gpu_ctx)
    with torch.cuda.stream(side):
        ix.upsert_dev(0, d_ids.data_ptr(), d_rows.data_ptr(), n, side.cuda_stream)
        assert ix.size(0) == n
        ix.query_dev(0, d_q.data_ptr(), nq, k, 1, o_ids.data_ptr(), o_a.data_ptr(), o_s.data_ptr(), o_n.data_ptr(),
                     side.cuda_stream)
    side.synchronize()
    got = (o_ids.cpu().numpy().view(np.uint64), o_a.cpu().numpy().view(np.uint32), o_s.cpu().numpy(), o_n.cpu().numpy().view(np.uint32))
    _check(got, ref.topk_from_agree(ids[:n], A[:nq, :n], k), k)
    _check(ix.query(0, queries[:nq], k), got, k)            # the host twin
    ix.close()


def test_against_the_lsh_shard(gpu_ctx, pool):
    """Whatever the banded shard returns carries the same score in the exact index, and the exact best is never worse."""
    from ucfp_amd import text
    from ucfp_amd.index import MinHashIndex
    rows, ids, _, _ = pool
    rng = np.random.default_rng(29)
    # queries near stored rows (a tenth to a half of the slots changed), so that the shard finds candidates
    src = rng.integers(0, N_POOL, 40)
    qs = ref.slots_of(rows[src]).copy()
    for i in range(40):
        pos = rng.choice(128, int(rng.integers(12, 64)), replace=False)
        qs[i, pos] ^= FLIPS[rng.integers(1, 4, pos.size)]
    queries = ref.records_of(qs)
    lsh = text.LshIndex(ctx=gpu_ctx)
    lsh.build(ids, rows)
    l_ids, l_sc, l_n = lsh.query(queries, 10)
    lsh.close()
    ix = MinHashIndex(ctx=gpu_ctx)
    ix.upsert(0, ids, rows)
    e_ids, e_a, e_sc, e_n = ix.query(0, queries, 128, 0)
    A = ref.agree_matrix(queries, rows)
    row_of = {int(i): r for r, i in enumerate(ids.tolist())}
    assert int(l_n.sum()) >= 20
    seen = 0
    for q in range(40):
        exact = {int(i): s for i, s in zip(e_ids[q, :int(e_n[q])].tolist(), e_sc[q].tolist())}
        for j in range(int(l_n[q])):
            i = int(l_ids[q, j])
            assert np.float32(l_sc[q, j]) == np.float32(A[q, row_of[i]]) / np.float32(128.0)
            if i in exact:
                assert np.float32(exact[i]) == np.float32(l_sc[q, j])
                seen += 1
            else:          # not among the best 128: then it is no better than the last of them
                assert l_sc[q, j] <= e_sc[q, 127]
        if l_n[q]:
            assert e_sc[q, 0] >= l_sc[q, 0]
    assert seen >= 20
    ix.close()


def test_gpu_index_end_to_end(gpu_ctx, tmp_path):
    """text.minhash_batch -> GpuIndex.upsert -> similar_text / query with a `minhash` body: every edited copy finds its
    original first; the answers equal the restatement; a key re-ingested under another algorithm leaves the index; and
    the same after store.rebuild."""
    import random
    from ucfp_amd import store, text
    from ucfp_amd.core import HitSource, Modality, QueryRequest, Record
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.index import GpuIndex
    rnd = random.Random(31)

    def word():
        return "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randrange(3, 10)))

    n = 200
    originals = [" ".join(word() for _ in range(60)) for _ in range(n)]
    copies = []
    for doc in originals:
        w = doc.split()
        w[rnd.randrange(len(w))] = "edited"
        copies.append(" ".join(w))
    recs, status = text.minhash_batch(originals + copies, text.TextOpts())
    assert not status.any()
    o_recs, c_recs = recs[:n], recs[n:]
    tag = text.ALGORITHM_MINHASH_128
    records = [Record(tenant_id=3, record_id=1000 + i, modality=Modality.Text, format_version=1, algorithm=tag,
                      config_hash=0, fingerprint=o_recs[i].tobytes(), text=originals[i]) for i in range(n)]
    records += [Record(tenant_id=4, record_id=7, modality=Modality.Text, format_version=1, algorithm=tag, config_hash=0,
                       fingerprint=o_recs[0].tobytes()),                       # another tenant
                Record(tenant_id=3, record_id=5000, modality=Modality.Text, format_version=1, algorithm=tag, config_hash=0,
                       fingerprint=o_recs[1].tobytes()[:1024])]                # not a whole record: feeds no MinHash index
    path = str(tmp_path / "side.log")
    gi = GpuIndex(gpu_ctx, sidecar=store.Sidecar(path))
    gi.upsert(records)
    assert {t: ix.size(3) for t, ix in gi._mh.items()} == {tag: n} and gi._mh[tag].size(4) == 1
    o_ids = np.arange(1000, 1000 + n, dtype=np.uint64)
    A = ref.agree_matrix(c_recs, o_recs)
    assert (A[np.arange(n), np.arange(n)] >= 64).all()

    def check_all(index):
        for i in range(0, n, 7):
            w_ids, w_a, w_s, w_n = ref.topk_from_agree(o_ids, A[i], 5, 1)
            for hits in (index.similar_text(3, copies[i], 5), index.similar_text(3, c_recs[i].tobytes(), 5),
                         index.query(QueryRequest.from_json({"tenant_id": 3, "modality": "Text", "k": 5,
                                                             "minhash": c_recs[i].tobytes().hex()}))):
                assert hits[0].record_id == 1000 + i
                assert [h.record_id for h in hits] == w_ids[0, :int(w_n[0])].tolist()
                assert [h.distance for h in hits] == [128 - int(a) for a in w_a[0, :int(w_n[0])]]
                assert [np.float32(h.score) for h in hits] == w_s[0, :int(w_n[0])].tolist()
                assert all(h.source == HitSource.MinHash == "minhash" and h.tenant_id == 3 for h in hits)

    check_all(gi)
    # the cut: min_agree, threshold and the body's min_similarity are the same thing
    a0 = int(A[0, 0])
    assert [h.record_id for h in gi.similar_text(3, copies[0], 5, min_agree=a0)] == [1000]
    assert gi.similar_text(3, copies[0], 5, min_agree=a0 + 1) == []
    assert [h.record_id for h in gi.similar_text(3, copies[0], 5, threshold=a0 / 128)] == [1000]
    req = QueryRequest.from_json({"tenant_id": 3, "modality": "Text", "minhash": list(c_recs[0].tobytes()),
                                  "min_similarity": a0 / 128, "algorithm": tag})
    assert [h.record_id for h in gi.query(req)] == [1000]
    with pytest.raises(InvalidArgument):
        gi.similar_text(3, copies[0], 5, min_agree=3, threshold=0.5)
    with pytest.raises(InvalidArgument):
        gi.similar_text(3, copies[0], 5, min_agree=129)
    with pytest.raises(InvalidArgument):
        gi.similar_text(3, b"\0" * 1031, 5)
    assert gi.similar_text(3, copies[0], 0) == [] and gi.similar_text(9, copies[0], 5) == []
    assert [h.record_id for h in gi.similar_text(4, copies[0], 5)] == [7]
    gi.flush()
    gi2 = store.rebuild(path, gpu_ctx)
    assert {t: ix.size(3) for t, ix in gi2._mh.items()} == {tag: n} and gi2._mh[tag].size(4) == 1
    check_all(gi2)
    # a second tag: the same bytes under `minhash-lsh-h128` are an index of their own, and `algorithm` is then required
    gi.upsert([Record(tenant_id=3, record_id=2000, modality=Modality.Text, format_version=1, algorithm=text.ALGORITHM_LSH,
                      config_hash=0, fingerprint=o_recs[0].tobytes())])
    assert gi._mh[text.ALGORITHM_LSH].size(3) == 1 and gi._mh[tag].size(3) == n
    with pytest.raises(InvalidArgument):
        gi.similar_text(3, copies[0], 5)
    assert [h.record_id for h in gi.similar_text(3, copies[0], 5, algorithm=text.ALGORITHM_LSH)] == [2000]
    assert gi.similar_text(3, copies[0], 5, algorithm=tag)[0].record_id == 1000
    # overwrite rule: id 1000 re-ingested as a TLSH record leaves the MinHash index; re-tagged, it changes index
    gi.upsert([text.fingerprint_tlsh(originals[0], text.TextOpts(), 3, 1000)])
    assert gi._mh[tag].size(3) == n - 1
    assert 1000 not in [h.record_id for h in gi.similar_text(3, copies[0], 5, algorithm=tag)]
    gi.upsert([Record(tenant_id=3, record_id=1001, modality=Modality.Text, format_version=1, algorithm=text.ALGORITHM_LSH,
                      config_hash=0, fingerprint=o_recs[1].tobytes())])
    assert gi._mh[tag].size(3) == n - 2 and gi._mh[text.ALGORITHM_LSH].size(3) == 2
    gi.delete(3, [2000])
    assert gi._mh[text.ALGORITHM_LSH].size(3) == 1
