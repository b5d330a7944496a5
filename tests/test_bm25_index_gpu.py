"""BM25 index on the device: every id, score (compared as bits), hit count and explain value equals the
numpy restatement (tests/bm25_ref.py), on both scoring paths and at the switch-over; duplicate and unknown terms,
tenants, mutations, zero-score hits, the device entry points and the error statuses; and GpuIndex end to end: BM25 over
Record.text, the filter error, and the hybrid query against RRF of the two lists."""
import numpy as np
import pytest

from bm25_ref import Bm25Ref, contribution, explain_cut, idf, norm, rrf_ref

pytestmark = pytest.mark.gpu

UCFP_E_INVALID = -4
LDS_POSTINGS = 6144       # UCFP_BM25_LDS_POSTINGS: a query with more postings is scored by ordinal ranges


def _index(ctx):
    from ucfp_amd.index import Bm25Index
    return Bm25Index(ctx=ctx)


def _pairs(docs: dict):
    """{id: {key: tf}} -> ids, keys, tfs, offsets (ids in dict order)."""
    ids = np.array(list(docs), np.uint64)
    keys, tfs, offs = [], [], [0]
    for d in docs.values():
        keys.extend(d.keys())
        tfs.extend(d.values())
        offs.append(len(keys))
    return ids, np.array(keys, np.uint64), np.array(tfs, np.uint32), np.array(offs, np.uint64)


def _upsert(ix, tenant, docs):
    ix.upsert_pairs(tenant, *_pairs(docs))


def _check(ix, tenant, docs, queries, k, explain=True):
    """Every output of one batch equals the restatement, bit for bit."""
    ref = Bm25Ref(docs)
    got = ix.query_keys(tenant, queries, k, explain=explain)
    ids, scores, counts = got[:3]
    off = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(int)
    for q, terms in enumerate(queries):
        hits, idfs = ref.search(list(terms), k, explain=True)
        assert counts[q] == len(hits), (q, counts[q], len(hits))
        assert [int(x) for x in ids[q, :len(hits)]] == [h[0] for h in hits], q
        assert np.array_equal(scores[q, :len(hits)].view(np.uint32),
                              np.array([h[1] for h in hits], np.float32).view(np.uint32)), q
        assert (ids[q, len(hits):] == 0xFFFFFFFFFFFFFFFF).all() and (scores[q, len(hits):] == -1).all()
        if not explain:
            continue
        g_idf, g_tf, g_c = got[3:]
        m = len(terms)
        assert np.array_equal(g_idf[off[q]:off[q + 1]].view(np.uint32), np.array(idfs, np.float32).view(np.uint32)), q
        tf = g_tf[k * off[q]:k * off[q + 1]].reshape(k, m) if m else np.zeros((k, 0), np.uint32)
        c = g_c[k * off[q]:k * off[q + 1]].reshape(k, m) if m else np.zeros((k, 0), np.float32)
        for h, (_, _, th) in enumerate(hits):
            want_tf = np.zeros(m, np.uint32)
            want_c = np.zeros(m, np.float32)
            pos = [j for j in range(m) if terms[j] in docs[int(ids[q, h])]]
            for j, (t, w, f, cc) in zip(pos, th):
                assert t == terms[j]
                want_tf[j], want_c[j] = f, cc
            assert np.array_equal(tf[h], want_tf) and np.array_equal(c[h].view(np.uint32), want_c.view(np.uint32)), (q, h)
        assert not tf[len(hits):].any() and not c[len(hits):].any()


def _zipf_docs(rng, n_docs, vocab, mean_len=30, id_space=1 << 40):
    docs = {}
    for rid in rng.choice(id_space, n_docs, replace=False).tolist():
        n = int(rng.integers(0, 2 * mean_len))
        toks = np.minimum((vocab * rng.random(n) ** 3).astype(np.int64), vocab - 1)
        u, c = np.unique(toks, return_counts=True)
        docs[rid] = dict(zip(u.tolist(), c.tolist()))
    return docs


def _zipf_queries(rng, nq, vocab):
    return [np.minimum((vocab * 1.2 * rng.random(int(rng.integers(0, 9))) ** 2).astype(np.int64), 2 * vocab).tolist()
            for _ in range(nq)]


@pytest.mark.parametrize("seed, n_docs", [(1, 12000), (2, 3000)])
def test_random_corpus_matches_reference(gpu_ctx, seed, n_docs):
    rng = np.random.default_rng(seed)
    docs = _zipf_docs(rng, n_docs, 4000)
    ix = _index(gpu_ctx)
    _upsert(ix, 5, docs)
    ref = Bm25Ref(docs)
    queries = _zipf_queries(rng, 200, 4000)
    v = [ref.postings(q) for q in queries]
    assert min(v) <= LDS_POSTINGS and (max(v) > LDS_POSTINGS) == (n_docs > 10000)   # 12000: both paths in one batch
    for k in (1, 10, 128):
        _check(ix, 5, docs, queries, k)
    _check(ix, 5, docs, queries, 7, explain=False)
    ix.close()


def test_switch_over_at_the_threshold(gpu_ctx):
    """V = LDS_POSTINGS (one LDS table) and V = LDS_POSTINGS + 1 (ordinal ranges) agree with the restatement."""
    rng = np.random.default_rng(3)
    n = 20000
    docs = {}
    common = set(rng.choice(n, LDS_POSTINGS, replace=False).tolist())
    for i in range(n):
        d = {1000 + int(x): 1 + int(x) % 3 for x in rng.integers(0, 50, int(rng.integers(0, 6)))}
        if i in common:
            d[7] = int(rng.integers(1, 5))
        docs[3 * i + 1] = d
    docs[5] = {8: 2}                                  # key 8: one posting
    ref = Bm25Ref(docs)
    queries = [[7], [7, 8], [8, 7], [7, 7], [8], [1003, 7, 8, 1004]]
    assert [ref.postings(q) for q in queries[:3]] == [LDS_POSTINGS, LDS_POSTINGS + 1, LDS_POSTINGS + 1]
    ix = _index(gpu_ctx)
    _upsert(ix, 0, docs)
    for k in (5, 128):
        _check(ix, 0, docs, queries, k)
    ix.close()


def test_stopword_in_a_million_documents(gpu_ctx):
    rng = np.random.default_rng(4)
    n = 1_000_000
    ids = rng.permutation(n).astype(np.uint64) * np.uint64(7) + np.uint64(3)
    tf0 = rng.integers(1, 6, n).astype(np.uint32)
    other = rng.integers(1, 100000, n).astype(np.uint64)
    keys = np.stack([np.zeros(n, np.uint64), other], 1).reshape(-1)
    tfs = np.stack([tf0, rng.integers(1, 4, n).astype(np.uint32)], 1).reshape(-1)
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(2)
    ix = _index(gpu_ctx)
    ix.upsert_pairs(1, ids, keys, tfs, offs)
    assert ix.size(1) == (n, 2 * n)
    dl = (tf0 + tfs[1::2]).astype(np.int64)
    avgdl = np.float32(int(dl.sum())) / np.float32(n)
    w = idf(n, n)
    score = contribution(w, tf0, norm(dl, avgdl))
    order = np.lexsort((ids, -score))[:128]
    g_ids, g_sc, g_n = ix.query_keys(1, [[0]], 128)
    assert g_n[0] == 128
    assert np.array_equal(g_ids[0], ids[order]) and np.array_equal(g_sc[0].view(np.uint32), score[order].view(np.uint32))
    # the stopword with a rare term after it: the rare term's documents lead
    rare = int(other[0])
    has = other == rare
    s2 = score.copy()
    w2 = idf(n, int(has.sum()))
    s2[has] = s2[has] + contribution(w2, tfs[1::2][has], norm(dl[has], avgdl))
    order = np.lexsort((ids, -s2))[:128]
    g_ids, g_sc, g_n = ix.query_keys(1, [[0, rare]], 128)
    assert np.array_equal(g_ids[0], ids[order]) and np.array_equal(g_sc[0].view(np.uint32), s2[order].view(np.uint32))
    ix.close()


def test_duplicates_unknown_terms_and_tenants(gpu_ctx):
    docs = {1: {10: 1, 11: 2}, 2: {10: 3}, 3: {12: 1}, 9: {}}
    other = {1: {10: 5}, 4: {10: 1, 13: 1}}
    ix = _index(gpu_ctx)
    _upsert(ix, 1, docs)
    _upsert(ix, 2, other)
    queries = [[10, 10], [10, 10, 11, 99], [99], [], [12, 10, 12]]
    _check(ix, 1, docs, queries, 10)
    _check(ix, 2, other, queries, 10)
    ids, sc, n = ix.query_keys(3, queries, 10)                 # unknown tenant
    assert not n.any() and (ids == 0xFFFFFFFFFFFFFFFF).all()
    ix.close()


def test_mutations(gpu_ctx):
    rng = np.random.default_rng(6)
    docs = _zipf_docs(rng, 800, 300)
    ix = _index(gpu_ctx)
    _upsert(ix, 0, docs)
    queries = _zipf_queries(rng, 40, 300)
    _check(ix, 0, docs, queries, 20)
    ids = list(docs)
    re_up = {i: {int(k): int(v) for k, v in zip(rng.integers(0, 300, 3), rng.integers(1, 4, 3))} for i in ids[:100]}
    re_up = {i: d for i, d in re_up.items()}
    _upsert(ix, 0, re_up)
    docs.update(re_up)
    _check(ix, 0, docs, queries, 20)
    assert ix.delete(0, np.array(ids[100:300] + [12345678901], np.uint64)) == 200
    for i in ids[100:300]:
        del docs[i]
    _check(ix, 0, docs, queries, 20)
    assert ix.size(0)[0] == len(docs)
    assert ix.delete(0, np.array(list(docs), np.uint64)) == len(docs)      # a tenant emptied by deletes
    ix.flush()
    assert ix.size(0) == (0, 0)
    got = ix.query_keys(0, queries, 20, explain=True)
    assert not got[2].any() and not got[3].any() and not got[4].any()
    ix.close()


def test_zero_score_hits_through_upsert_dev(gpu_ctx, torch_cuda):
    """One key in all 2^23 + 1 documents: idf rounds to logf(1) = 0, every score is 0 and every document is a hit."""
    torch = torch_cuda
    n = (1 << 23) + 1
    ids = torch.arange(n, dtype=torch.int64, device="cuda").flip(0) * 3
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    tfs = (torch.arange(n, device="cuda") % 4 + 1).to(torch.int32)
    offs = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    ix = _index(gpu_ctx)
    st = torch.cuda.current_stream().cuda_stream
    ix.upsert_dev(2, ids.data_ptr(), keys.data_ptr(), tfs.data_ptr(), offs.data_ptr(), n, st)
    assert ix.size(2) == (n, n)
    assert idf(n, n) == 0.0
    g_ids, g_sc, g_n = ix.query_keys(2, [[0], [0, 0]], 128)
    assert list(g_n) == [128, 128]
    assert (g_ids == np.arange(128, dtype=np.uint64) * np.uint64(3)).all()
    assert (g_sc.view(np.uint32) == 0).all()
    ix.close()


def test_dev_entry_points_and_errors(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib
    from ucfp_amd.errors import UcfpError
    torch = torch_cuda
    rng = np.random.default_rng(8)
    docs = _zipf_docs(rng, 20000, 2000, mean_len=20)
    ix = _index(gpu_ctx)
    _upsert(ix, 0, docs)
    queries = _zipf_queries(rng, 64, 2000)
    k = 16
    want = ix.query_keys(0, queries, k, explain=True)
    total = sum(len(q) for q in queries)
    qk = torch.from_numpy(np.array(sum(queries, []) + [0], np.int64)).cuda()
    qo = torch.from_numpy(np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)).cuda()
    o_ids = torch.zeros((64, k), dtype=torch.int64, device="cuda")
    o_s = torch.zeros((64, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(64, dtype=torch.int32, device="cuda")
    o_idf = torch.zeros(total, dtype=torch.float32, device="cuda")
    o_tf = torch.zeros(total * k, dtype=torch.int32, device="cuda")
    o_c = torch.zeros(total * k, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ix.query_dev(0, qk.data_ptr(), qo.data_ptr(), 64, k, o_ids.data_ptr(), o_s.data_ptr(), o_n.data_ptr(),
                 o_idf.data_ptr(), o_tf.data_ptr(), o_c.data_ptr(), st)
    torch.cuda.synchronize()
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(o_s.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(o_n.cpu().numpy().view(np.uint32), want[2])
    assert np.array_equal(o_idf.cpu().numpy().view(np.uint32), want[3].view(np.uint32))
    assert np.array_equal(o_tf.cpu().numpy().view(np.uint32), want[4])
    assert np.array_equal(o_c.cpu().numpy().view(np.uint32), want[5].view(np.uint32))
    # errors: nothing changes
    before = ix.size(0)
    bad = [({7: {1: 1}}, lambda i, k_, t, o: (i, np.array([1, 1], np.uint64), np.array([1, 2], np.uint32),
                                               np.array([0, 2], np.uint64))),          # a key twice
           ({7: {1: 0}}, None),                                                          # tf = 0
           ({7: {1: 1}}, lambda i, k_, t, o: (i, k_, t, np.array([1, 1], np.uint64))),   # offsets[0] != 0
           ({7: {1: 1}, 8: {2: 1}}, lambda i, k_, t, o: (i, k_, t, np.array([0, 2, 1], np.uint64)))]   # decreasing
    for d, fix in bad:
        args = _pairs(d)
        if fix:
            args = fix(*args)
        with pytest.raises(UcfpError):
            ix.upsert_pairs(0, *args)
        assert _lib.load().ucfp_bm25_index_upsert(ix.handle, 0, args[0].ctypes.data, args[1].ctypes.data,
                                                  args[2].ctypes.data, args[3].ctypes.data, args[0].size) == UCFP_E_INVALID
    assert ix.size(0) == before
    with pytest.raises(UcfpError):
        ix.query_keys(0, queries[:2], 129)
    o = np.array([0, 2, 1], np.uint64)
    kk = np.zeros(4, np.uint64)
    out = np.zeros(8, np.uint64)
    assert _lib.load().ucfp_bm25_index_query(ix.handle, 0, kk.ctypes.data, o.ctypes.data, 2, 2, out.ctypes.data,
                                             out.ctypes.data, out.ctypes.data, None, None, None) == UCFP_E_INVALID
    bad_o = torch.from_numpy(o.view(np.int64)).cuda()
    with pytest.raises(UcfpError):
        ix.query_dev(0, qk.data_ptr(), bad_o.data_ptr(), 2, k, o_ids.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), stream=st)
    # k = 0: no hits
    assert not ix.query_keys(0, queries[:3], 0)[2].any()
    ix.close()


# ---------------------------------------------------------------- GpuIndex, from records made by text.py

def _text_rec(tenant, rid, text, emb=None):
    from ucfp_amd import text as T
    r = T.fingerprint_minhash(text, tenant, rid)
    r.embedding = emb
    return r


def test_bm25_round_trip_via_upsert(gpu_ctx):
    from ucfp_amd.core import HitSource
    from ucfp_amd.index import GpuIndex
    g = GpuIndex(gpu_ctx)
    g.upsert([_text_rec(1, 100, "rust async language"), _text_rec(1, 101, "go async language")])
    hits = g.bm25(1, ["rust"], 10)
    assert len(hits) == 1 and hits[0].record_id == 100 and hits[0].source == HitSource.Bm25
    # re-ingested without text: gone from BM25 (embedded/mod.rs:213-219); delete removes too
    r = _text_rec(1, 100, "rust async language")
    r.text = None
    g.upsert([r])
    assert g.bm25(1, ["rust"], 10) == []
    assert [h.record_id for h in g.bm25(1, ["ASYNC!"], 10)] == [101]
    g.delete(1, [101])
    assert g.bm25(1, ["async"], 10) == []
    g.flush()


def test_bm25_filter_param_is_unsupported(gpu_ctx):
    from ucfp_amd.errors import UnsupportedError
    from ucfp_amd.index import GpuIndex
    g = GpuIndex(gpu_ctx)
    with pytest.raises(UnsupportedError):
        g.bm25(1, ["foo"], 10, b"\x00")


def test_hybrid_query_is_rrf_of_knn_and_bm25(gpu_ctx):
    from ucfp_amd.core import HitSource, QueryRequest, hit_to_json
    from ucfp_amd.index import GpuIndex
    rng = np.random.default_rng(9)
    words = ["rust", "async", "go", "language", "safety", "fast", "memory", "tokio", "thread", "web"]
    g = GpuIndex(gpu_ctx)
    recs, texts = [], {}
    for rid in range(1, 61):
        t = " ".join(rng.choice(words, int(rng.integers(1, 8))).tolist())
        texts[rid] = t
        recs.append(_text_rec(4, rid, t, rng.standard_normal(8).astype(np.float32).tolist()))
    g.upsert(recs)
    vec = rng.standard_normal(8).astype(np.float32).tolist()
    body = {"tenant_id": 4, "modality": "Text", "k": 12, "vector": vec, "terms": ["Rust memory", "rust"], "explain": True}
    hits = g.query(QueryRequest.from_json(body))
    knn = g.knn(4, vec, 12)
    bm = g.bm25(4, ["Rust memory", "rust"], 12, explain=True)
    want = rrf_ref([[h.record_id for h in knn], [h.record_id for h in bm]], ["vector", "bm25"], 60)[:12]
    assert [h.record_id for h in hits] == [w[0] for w in want]
    for h, (_, tot, vs, bs, vr, br) in zip(hits, want):
        assert h.source == HitSource.Fused and np.float32(h.score) == tot
        assert (h.vector_rank, h.bm25_rank) == (vr, br)
        assert (h.vector_score is None) == (vs is None) and (h.bm25_score is None) == (bs is None)
    by_id = {h.record_id: h.term_hits for h in bm}
    assert any(h.term_hits for h in hits)
    for h in hits:
        assert h.term_hits == by_id.get(h.record_id, [])
    # the explain values of the bm25 list are the restatement's
    from ucfp_amd.terms import query_terms, tokenize
    docs = {}
    for rid, t in texts.items():
        d = {}
        for tok in tokenize(t):
            d[tok] = d.get(tok, 0) + 1
        docs[rid] = d
    ref, _ = Bm25Ref(docs).search(query_terms(["Rust memory", "rust"]), 12, explain=True)
    assert [h.record_id for h in bm] == [r[0] for r in ref]
    for h, (_, s, th) in zip(bm, ref):
        assert np.float32(h.score) == s
        assert [(t.term, np.float32(t.idf), t.tf, np.float32(t.contribution)) for t in h.term_hits] == \
               [(t, w, f, c) for t, w, f, c in explain_cut(th)]
    # terms only: bm25 hits carry bm25_score / bm25_rank; the JSON has the term_hits objects
    only = g.query(QueryRequest.from_json({"tenant_id": 4, "modality": "Text", "k": 5, "terms": ["rust"], "explain": 1}))
    assert [h.record_id for h in only] == [h.record_id for h in g.bm25(4, ["rust"], 5)]
    assert all(h.bm25_rank == i + 1 and h.bm25_score == h.score for i, h in enumerate(only))
    assert set(hit_to_json(only[0])["term_hits"][0]) == {"term", "idf", "tf", "contribution"}
    # vector only is unchanged
    vo = g.query(QueryRequest.from_json({"tenant_id": 4, "modality": "Text", "k": 5, "vector": vec}))
    assert [h.record_id for h in vo] == [h.record_id for h in knn[:5]] and all(h.source == HitSource.Vector for h in vo)
