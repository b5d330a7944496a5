"""BM25 and RRF on the CPU: the numpy restatement (tests/bm25_ref.py) against a literal transcription
of the reference's search_explain; the reference's own tests of bm25.rs and matcher/mod.rs replayed on the
restatement and on ucfp_amd.matcher; the tokenizer; the `terms` / `explain` wire fields and the JSON of BM25 and fused
hits."""
import json

import numpy as np
import pytest

from bm25_ref import Bm25Ref, explain_cut, idf, rrf_ref, search_explain_literal
from ucfp_amd.core import Hit, HitSource, QueryRequest, TermHit, hit_to_json
from ucfp_amd.errors import InvalidArgument
from ucfp_amd.matcher import rrf, rrf_with_sources
from ucfp_amd.terms import is_alphanumeric, query_terms, tokenize


def _docs(texts: dict) -> dict:
    out = {}
    for rid, t in texts.items():
        d = {}
        for tok in tokenize(t):
            d[tok] = d.get(tok, 0) + 1
        out[rid] = d
    return out


def _search(texts, terms, k=10, explain=False):
    hits, _ = Bm25Ref(_docs(texts)).search(query_terms(terms), k, explain)
    return hits


def test_restatement_equals_literal_search_explain():
    rng = np.random.default_rng(11)
    for case in range(300):
        n_docs, vocab = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        docs = {}
        for rid in rng.choice(1000, n_docs, replace=False).tolist():
            n = int(rng.integers(0, 25))
            toks = (vocab * rng.random(n) ** 2).astype(int).tolist()
            d = {}
            for t in toks:
                d[t] = d.get(t, 0) + int(rng.integers(1, 3)) if case % 2 else d.get(t, 0) + 1
            docs[rid] = d
        terms = (vocab * 1.3 * rng.random(int(rng.integers(1, 9))) ** 2).astype(int).tolist()   # some unknown
        k = int(rng.integers(1, 50))
        got, _ = Bm25Ref(docs).search(terms, k, explain=True)
        lit = search_explain_literal(docs, terms, k, explain=True)
        want = sorted(lit.items(), key=lambda kv: (-kv[1][0], kv[0]))[:k]
        assert [r for r, _, _ in got] == [r for r, _ in want], case
        for (r, s, th), (_, (ls, lth)) in zip(got, want):
            assert np.float32(s).view(np.uint32) == np.float32(ls).view(np.uint32), (case, r)
            assert [(t, np.float32(w).view(np.uint32), tf, np.float32(c).view(np.uint32)) for t, w, tf, c in th] == \
                   [(t, np.float32(w).view(np.uint32), tf, np.float32(c).view(np.uint32)) for t, w, tf, c in lth]


def test_zero_idf_still_hits():
    # df = N > 2^23: (N - df + 0.5) / (df + 0.5) + 1 rounds to 1 and logf(1) = 0
    assert idf((1 << 23) + 1, (1 << 23) + 1) == 0.0
    assert idf(3, 3) > 0.0


# ---- bm25.rs tests (:659-782)

def test_tokenize_lowercases_and_splits():
    assert tokenize("Hello, World!  It's GREAT.") == ["hello", "world", "it", "s", "great"]


def test_round_trip_single_doc():
    hits = _search({100: "the quick brown fox"}, ["fox"])
    assert len(hits) == 1 and hits[0][0] == 100 and hits[0][1] > 0.0


def test_ranks_by_relevance():
    hits = _search({100: "rust rust rust async", 101: "rust async language", 102: "go language"}, ["rust"])
    assert [h[0] for h in hits] == [100, 101]


def test_multi_term_query():
    hits = _search({1: "rust async language", 2: "go async language", 3: "rust safety"}, ["rust", "async"])
    assert hits[0][0] == 1


def test_tenant_isolation():
    assert [h[0] for h in _search({100: "tenant one document"}, ["document"])] == [100]
    assert [h[0] for h in _search({200: "tenant two document"}, ["document"])] == [200]


def test_unknown_term_returns_empty():
    assert _search({1: "the quick brown fox"}, ["zebra"]) == []


def test_delete_removes_from_scoring():
    texts = {100: "rust async", 101: "rust safety"}
    del texts[100]
    assert [h[0] for h in _search(texts, ["rust"])] == [101]


def test_re_upsert_replaces_tf():
    texts = {100: "rust rust rust rust rust rust"}
    texts[100] = "rust other words here"
    texts[101] = "rust rust rust rust rust"
    assert _search(texts, ["rust"])[0][0] == 101


def test_empty_text_records_doc_len_zero():
    docs = _docs({100: "   ,,, ...   "})
    assert docs == {100: {}}
    ref = Bm25Ref(docs)
    assert ref.n == 1 and ref.search(["anything"], 10)[0] == []


# ---- tokenizer

def test_tokenizer_other_alphabetic_final_sigma_dotted_i():
    for ch in ("Ⓐ", "ः", "ͅ", "ְ"):       # Other_Alphabetic: alphanumeric in Rust, not in Python
        assert is_alphanumeric(ch) and not ch.isalnum(), hex(ord(ch))
    assert tokenize("ⒶⒷ-xःy") == ["ⓐⓑ", "xःy"]
    assert tokenize("ΟΔΟΣ ΣΑ") == ["\u03bf\u03b4\u03bf\u03c2", "\u03c3\u03b1"]     # Final_Sigma: only at a word's end
    assert tokenize("İstanbul") == ["i\u0307stanbul"]
    assert tokenize("a²b ½ x_y") == ["a²b", "½", "x", "y"]   # No is numeric; '_' splits
    assert query_terms(["Hello, World", "hello", ""]) == ["hello", "world", "hello"]


def test_tokenizer_table_matches_alphabetic_or_numeric():
    regex = pytest.importorskip("regex")
    pat = regex.compile(r"[\p{Alphabetic}\p{N}]")
    bad = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000
           and bool(pat.match(chr(cp))) != is_alphanumeric(chr(cp))]
    assert not bad, [hex(c) for c in bad[:10]]


# ---- matcher/mod.rs tests (:223-278)

def _h(rid, score, src):
    return Hit(tenant_id=1, record_id=rid, score=score, source=src)


def test_rrf_with_sources_populates_breakdown_for_overlap():
    vec_hits = [_h(10, 0.9, HitSource.Vector), _h(20, 0.8, HitSource.Vector)]
    bm_hits = [_h(20, 4.5, HitSource.Bm25), _h(30, 4.0, HitSource.Bm25)]
    fused = rrf_with_sources([vec_hits, bm_hits], [HitSource.Vector, HitSource.Bm25], 60)
    twenty = next(h for h in fused if h.record_id == 20)
    assert twenty.vector_score is not None and twenty.bm25_score is not None
    assert (twenty.vector_rank, twenty.bm25_rank) == (2, 1)
    assert abs(twenty.score - (twenty.vector_score + twenty.bm25_score)) < 1e-6
    ten = next(h for h in fused if h.record_id == 10)
    assert ten.vector_score is not None and ten.bm25_score is None
    assert all(h.source == HitSource.Fused for h in fused)


def test_rrf_legacy_is_equivalent_to_with_sources_total():
    vec_hits = [_h(10, 0.9, HitSource.Vector), _h(20, 0.8, HitSource.Vector)]
    bm_hits = [_h(20, 4.5, HitSource.Bm25), _h(30, 4.0, HitSource.Bm25)]
    legacy = rrf([vec_hits, bm_hits], 60)
    with_src = rrf_with_sources([vec_hits, bm_hits], [HitSource.Vector, HitSource.Bm25], 60)
    assert len(legacy) == len(with_src)
    for a, b in zip(legacy, with_src):
        assert a.record_id == b.record_id and abs(a.score - b.score) < 1e-6


def test_rrf_matches_restatement_bit_for_bit():
    rng = np.random.default_rng(5)
    for _ in range(50):
        va = rng.choice(40, int(rng.integers(0, 20)), replace=False).tolist()
        ba = rng.choice(40, int(rng.integers(0, 20)), replace=False).tolist()
        fused = rrf_with_sources([[_h(r, 0.0, HitSource.Vector) for r in va], [_h(r, 0.0, HitSource.Bm25) for r in ba]],
                                 [HitSource.Vector, HitSource.Bm25], 60)
        want = rrf_ref([va, ba], ["vector", "bm25"], 60)
        assert [h.record_id for h in fused] == [w[0] for w in want]
        for h, (_, tot, vs, bs, vr, br) in zip(fused, want):
            assert np.float32(h.score) == tot and (h.vector_rank, h.bm25_rank) == (vr, br)
            assert (h.vector_score is None) == (vs is None) and (h.bm25_score is None) == (bs is None)


def test_explain_cut_is_stable_and_capped():
    th = [("t%d" % i, 1.0, 1, np.float32(i % 3)) for i in range(20)]
    cut = explain_cut(th)
    assert len(cut) == 16 and [t[0] for t in cut[:3]] == ["t2", "t5", "t8"]


# ---- wire format

def test_query_request_terms_and_explain():
    r = QueryRequest.from_json({"tenant_id": 3, "modality": "Text", "terms": ["rust", "async"]})
    assert (r.terms, r.vector, r.explain, r.k) == (["rust", "async"], None, False, 10)
    r = QueryRequest.from_json({"tenant_id": 3, "modality": "Text", "terms": ["x"], "vector": [1, 0], "explain": "1"})
    assert r.terms == ["x"] and r.vector == [1.0, 0.0] and r.explain
    assert QueryRequest.from_json({"tenant_id": 1, "modality": "Image", "vector": [1]}).terms == []
    for bad in ({"tenant_id": 1, "modality": "Text", "terms": "rust"}, {"tenant_id": 1, "modality": "Text", "terms": [1]},
                {"tenant_id": 1, "modality": "Text", "terms": []}):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json(bad)


def test_bm25_and_fused_hit_json():
    h = Hit(tenant_id=1, record_id=7, score=1.5, source=HitSource.Bm25, bm25_score=1.5, bm25_rank=1,
            term_hits=[TermHit(term="rust", idf=0.5, tf=2, contribution=1.5)])
    assert json.dumps(hit_to_json(h)) == (
        '{"tenant_id": 1, "record_id": 7, "score": 1.5, "source": "bm25", "vector_score": null, "bm25_score": 1.5, '
        '"vector_rank": null, "bm25_rank": 1, "term_hits": [{"term": "rust", "idf": 0.5, "tf": 2, "contribution": 1.5}]}')
    f = Hit(tenant_id=1, record_id=7, score=0.25, source=HitSource.Fused, vector_score=0.125, bm25_score=0.125,
            vector_rank=2, bm25_rank=1)
    assert json.dumps(hit_to_json(f)) == (
        '{"tenant_id": 1, "record_id": 7, "score": 0.25, "source": "fused", "vector_score": 0.125, "bm25_score": 0.125, '
        '"vector_rank": 2, "bm25_rank": 1, "term_hits": []}')
