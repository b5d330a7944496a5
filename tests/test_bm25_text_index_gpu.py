"""Bm25Index(keys="hashed"): texts tokenised, hashed and counted on the device give the ids, score bits and
term_hits that the numbered index (the host loop) and the restatement (tests/bm25_ref.py) give -- over a corpus with
non-ASCII and empty documents, through replacing upserts and deletes, for search_texts, and behind GpuIndex."""
import numpy as np
import pytest

from bm25_ref import Bm25Ref, explain_cut, rrf_ref

pytestmark = pytest.mark.gpu

TENANT = 3
FOREIGN = ["café", "naïve", "Über", "ΣΊΣΥΦΟΣ", "Οδυσσεύς", "λόγος", "漢字", "東京", "İstanbul", "straße"]
SEPS = [" ", ", ", ". ", "_", "'", ": ", "; ", "\n", " - "]


def _vocab(rng, n):
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8)
    words = set()
    while len(words) < n:
        words.add(bytes(letters[rng.integers(0, 36, int(rng.integers(1, 9)))]).decode())
    return sorted(words)


def _doc(rng, vocab, foreign):
    n = int(rng.integers(1, 60))
    idx = np.minimum((len(vocab) * rng.random(n) ** 3).astype(np.int64), len(vocab) - 1)
    words = [vocab[i] for i in idx]
    words = [w.upper() if rng.random() < 0.1 else w.capitalize() if rng.random() < 0.1 else w for w in words]
    if foreign:
        for _ in range(int(rng.integers(1, 4))):
            words.insert(int(rng.integers(0, len(words) + 1)), FOREIGN[int(rng.integers(len(FOREIGN)))])
    return "".join(w + SEPS[int(rng.integers(len(SEPS)))] for w in words)


def _corpus(seed=11, n=3000, vocab_size=1500):
    rng = np.random.default_rng(seed)
    vocab = _vocab(rng, vocab_size)
    ids = rng.choice(1 << 40, n, replace=False).astype(np.uint64)
    texts = ["" if i % 400 == 7 else " .,_ " if i % 400 == 9 else _doc(rng, vocab, i % 10 == 3) for i in range(n)]
    return rng, vocab, ids, texts


def _queries(rng, vocab, nq):
    out = []
    for q in range(nq):
        m = int(rng.integers(1, 7))
        idx = np.minimum((len(vocab) * rng.random(m) ** 2).astype(np.int64), len(vocab) - 1)
        terms = [vocab[i] for i in idx]
        if q % 5 == 0:
            terms.append(FOREIGN[q // 5 % len(FOREIGN)])
        if q % 7 == 0:
            terms.append(terms[0].upper() + "_" + terms[-1])       # re-tokenised: two terms, one a duplicate
        out.append(terms)
    return out


def _ref_docs(ids, texts):
    from ucfp_amd.terms import tokenize
    docs = {}
    for i, t in zip(ids.tolist(), texts):
        d = {}
        for tok in tokenize(t):
            d[tok] = d.get(tok, 0) + 1
        docs[i] = d
    return docs


def _flat(hits):
    """Every field of a hit list, floats as their f32 bits."""
    bits = lambda x: int(np.float32(x).view(np.uint32))
    return [(h.tenant_id, h.record_id, bits(h.score), h.source, [(t.term, bits(t.idf), t.tf, bits(t.contribution)) for t in h.term_hits])
            for h in hits]


def _agree(hashed, numbered, docs, queries, k):
    from ucfp_amd.terms import query_terms
    ref = Bm25Ref(docs)
    nonempty = 0
    for terms in queries:
        a = hashed.search(TENANT, terms, k, explain=True)
        b = numbered.search(TENANT, terms, k, explain=True)
        assert _flat(a) == _flat(b), terms
        want, _ = ref.search(query_terms(terms), k, explain=True)
        bits = lambda x: int(np.float32(x).view(np.uint32))
        assert [(h[1], h[2]) for h in _flat(a)] == [(r[0], bits(r[1])) for r in want], terms
        for h, (_, _, th) in zip(_flat(a), want):
            assert h[4] == [(t, bits(w), f, bits(c)) for t, w, f, c in explain_cut(th)], terms
        nonempty += bool(a)
    assert nonempty > len(queries) // 2
    assert hashed.size(TENANT) == numbered.size(TENANT) == (len(docs), sum(len(d) for d in docs.values()))


def test_hashed_index_equals_numbered_index_and_reference(gpu_ctx):
    from ucfp_amd.index import Bm25Index
    rng, vocab, ids, texts = _corpus()
    assert sum(not t.isascii() for t in texts) >= 250 and texts.count("") >= 5
    hashed, numbered = Bm25Index(ctx=gpu_ctx, keys="hashed"), Bm25Index(ctx=gpu_ctx)
    hashed.upsert(TENANT, ids, texts)
    numbered.upsert(TENANT, ids, texts)
    assert hashed.keys == {} and numbered.keys
    docs = _ref_docs(ids, texts)
    queries = _queries(rng, vocab, 200)
    _agree(hashed, numbered, docs, queries, 10)
    # mutations: replace some documents (two of them with nothing), delete others, on both
    swap = rng.choice(len(ids), 300, replace=False)
    new_texts = [_doc(rng, vocab, j % 4 == 0) if j % 50 else "" for j in range(swap.size)]
    gone = ids[rng.choice(len(ids), 200, replace=False)]
    for ix in (hashed, numbered):
        ix.upsert(TENANT, ids[swap], new_texts)
        assert ix.delete(TENANT, gone) == 200
    for j, t in zip(swap.tolist(), new_texts):
        texts[j] = t
    keep = ~np.isin(ids, gone)
    docs = _ref_docs(ids[keep], [t for t, kp in zip(texts, keep) if kp])
    _agree(hashed, numbered, docs, queries[:80], 128)
    hashed.close()
    numbered.close()


def test_search_texts_equals_search(gpu_ctx):
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.index import Bm25Index
    rng, vocab, ids, texts = _corpus(seed=12, n=600, vocab_size=300)
    ix = Bm25Index(ctx=gpu_ctx, keys="hashed")
    ix.upsert(TENANT, ids, texts)
    qs = [" ".join(q) for q in _queries(rng, vocab, 40)] + ["", " _ ", "zzzzneverindexed", vocab[0] + " " + vocab[0].upper()]
    for explain in (False, True):
        got = ix.search_texts(TENANT, qs, 10, explain=explain)
        assert len(got) == len(qs)
        for q, hits in zip(qs, got):
            assert _flat(hits) == _flat(ix.search(TENANT, [q], 10, explain=explain)), q
    assert got[-4] == [] and got[-3] == [] and got[-2] == [] and got[-1]
    # a term never indexed is an unknown key: it matches nothing and changes nothing
    base = vocab[0] + " " + vocab[3]
    with_unknown = vocab[0] + " zzzzneverindexed " + vocab[3] + " 漢漢漢"
    a, b = ix.search_texts(TENANT, [base, with_unknown], 20, explain=True)
    assert a and _flat(a) == _flat(b)
    assert _flat(ix.search(TENANT, [with_unknown], 20, explain=True)) == _flat(a)
    assert ix.search_texts(TENANT, qs, 0) == [[] for _ in qs] and ix.search_texts(TENANT, [], 5) == []
    with pytest.raises(InvalidArgument):
        Bm25Index(ctx=gpu_ctx).search_texts(TENANT, ["a"], 5)
    ix.close()


def test_dev_outputs_feed_the_index_as_they_are(gpu_ctx, torch_cuda):
    """Resident text -> ucfp_bm25_terms_batch_dev -> ucfp_bm25_index_upsert_dev / _query_dev on one stream, no host copy
    of a pair: the answers are those of the numbered index over the same texts."""
    from ucfp_amd import _lib
    from ucfp_amd.index import Bm25Index
    torch, lib = torch_cuda, _lib.load()
    rng, vocab, ids, texts = _corpus(seed=14, n=800, vocab_size=400)
    texts = [t if t.isascii() else "" for t in texts]
    queries = [" ".join(q) for q in _queries(rng, vocab, 30) if all(t.isascii() for t in q)] + ["", "zzzzneverindexed " + vocab[0]]
    st = torch.cuda.current_stream().cuda_stream

    def resident(strings):
        blobs = [s.encode("ascii") for s in strings]
        offs = np.zeros(len(blobs) + 1, np.int64)
        np.cumsum([len(b) for b in blobs], out=offs[1:])
        d_blob = torch.from_numpy(np.frombuffer(b"".join(blobs) + b"\0", np.uint8).copy()).cuda()
        return d_blob, torch.from_numpy(offs).cuda(), int(offs[-1]), len(blobs)

    def terms_dev(strings, form):
        d_blob, d_offs, total, n = resident(strings)
        cap = int(lib.ucfp_bm25_terms_max_pairs(total, n))
        out = (torch.zeros(cap + 1, dtype=torch.int64, device="cuda"), torch.zeros(cap + 1, dtype=torch.int32, device="cuda"),
               torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
        _lib.check(lib.ucfp_bm25_terms_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, total, form, out[0].data_ptr(),
                                                 out[1].data_ptr() if form == 0 else None, cap, out[2].data_ptr(), out[3].data_ptr(), st))
        return out

    hashed, numbered = Bm25Index(ctx=gpu_ctx, keys="hashed"), Bm25Index(ctx=gpu_ctx)
    d_keys, d_tfs, d_po, d_st = terms_dev(texts, 0)
    d_ids = torch.from_numpy(ids.view(np.int64).copy()).cuda()
    hashed.upsert_dev(TENANT, d_ids.data_ptr(), d_keys.data_ptr(), d_tfs.data_ptr(), d_po.data_ptr(), len(texts), st)
    numbered.upsert(TENANT, ids, texts)
    assert not d_st.any().item() and hashed.size(TENANT) == numbered.size(TENANT)
    q_keys, _, q_po, q_st = terms_dev(queries, 1)
    nq, k = len(queries), 10
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_sc = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    hashed.query_dev(TENANT, q_keys.data_ptr(), q_po.data_ptr(), nq, k, o_ids.data_ptr(), o_sc.data_ptr(), o_n.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert not q_st.any().item()
    g_ids, g_sc, g_n = o_ids.cpu().numpy().view(np.uint64), o_sc.cpu().numpy(), o_n.cpu().numpy()
    for q, text in enumerate(queries):
        want = numbered.search(TENANT, [text], k)
        assert int(g_n[q]) == len(want), text
        assert g_ids[q, :len(want)].tolist() == [h.record_id for h in want], text
        assert np.array_equal(g_sc[q, :len(want)].view(np.uint32), np.array([h.score for h in want], np.float32).view(np.uint32)), text
    assert g_n[:-2].any() and g_n[-2] == 0 and g_n[-1] > 0
    hashed.close()
    numbered.close()


def test_gpu_index_with_hashed_bm25_keys(gpu_ctx):
    from ucfp_amd import text as T
    from ucfp_amd.core import QueryRequest
    from ucfp_amd.index import GpuIndex
    rng = np.random.default_rng(13)
    words = ["rust", "async", "go", "language", "safety", "fast", "memory", "tokio", "thread", "web", "Größe", "naïve"]
    recs = []
    for rid in range(1, 81):
        r = T.fingerprint_minhash("one record with some text", 4, rid)     # BM25 reads Record.text only
        r.text = " ".join(rng.choice(words, int(rng.integers(1, 8))).tolist()) + ("" if rid % 9 else " it's_3.14")
        r.embedding = rng.standard_normal(8).astype(np.float32).tolist()
        recs.append(r)
    g_h, g_n = GpuIndex(gpu_ctx, bm25_keys="hashed"), GpuIndex(gpu_ctx)
    for g in (g_h, g_n):
        g.upsert(recs)
    assert g_h._bm.hashed and not g_n._bm.hashed and g_h._bm.keys == {}
    for terms in (["rust"], ["Rust memory", "rust"], ["größe"], ["it's"], ["3.14 web"], ["unknownterm"], ["unknownterm go"]):
        for explain in (False, True):
            assert _flat(g_h.bm25(4, terms, 12, explain=explain)) == _flat(g_n.bm25(4, terms, 12, explain=explain)), terms
    assert g_h.bm25(4, ["rust"], 12) and g_h.bm25(4, ["14"], 12)
    vec = rng.standard_normal(8).astype(np.float32).tolist()
    body = {"tenant_id": 4, "modality": "Text", "k": 12, "vector": vec, "terms": ["Rust memory", "rust"], "explain": True}
    h_h, h_n = g_h.query(QueryRequest.from_json(body)), g_n.query(QueryRequest.from_json(body))
    assert h_h and h_h == h_n
    want = rrf_ref([[h.record_id for h in g_h.knn(4, vec, 12)], [h.record_id for h in g_h.bm25(4, ["Rust memory", "rust"], 12)]],
                   ["vector", "bm25"], 60)[:12]
    assert [h.record_id for h in h_h] == [w[0] for w in want]
    g_h.delete(4, [1, 2, 3])
    g_n.delete(4, [1, 2, 3])
    assert _flat(g_h.bm25(4, ["rust go web"], 50)) == _flat(g_n.bm25(4, ["rust go web"], 50))
