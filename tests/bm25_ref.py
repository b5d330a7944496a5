"""CPU restatement of the BM25 spec and of RRF (src/matcher/mod.rs:22-98), shared by the BM25 tests.

`Bm25Ref` is the numpy restatement: f32 arrays, one IEEE operation at a time in the spec's order, idf from the C
library's logf.  `search_explain_literal` transcribes the reference's `search_explain` (bm25.rs:468-628): a dict of
np.float32 scalars, for small cases.  Documents are {term: tf} dicts; terms may be strings or integer keys."""
import ctypes

import numpy as np

K1 = np.float32(1.2)
B = np.float32(0.75)
F0, F1, HALF = np.float32(0.0), np.float32(1.0), np.float32(0.5)
TERM_HITS_PER_DOC = 16

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x) -> np.float32:
    """The host C library's logf (what Rust's f32::ln calls on Linux)."""
    return np.float32(_libm.logf(float(np.float32(x))))


def idf(n_docs: int, df: int) -> np.float32:
    nf, d = np.float32(n_docs), np.float32(df)
    return logf((nf - d + HALF) / (d + HALF) + F1)


def norm(dl, avgdl: np.float32):
    dl = np.asarray(dl, np.float32)
    return K1 * ((F1 - B) + (B * dl) / np.maximum(avgdl, F1))


def contribution(w, tf, nrm):
    tf = np.asarray(tf, np.float32)
    den = tf + nrm
    return (w * (tf * (K1 + F1))) / np.maximum(den, np.float32(1e-6))


class Bm25Ref:
    """One tenant: {record_id: {term: tf}}."""

    def __init__(self, docs: dict):
        self.ids = np.array(sorted(docs), np.uint64)
        self.docs = [docs[int(i)] for i in self.ids]
        self.n = len(self.docs)
        self.dl = np.array([sum(d.values()) for d in self.docs], np.int64)
        self.avgdl = np.float32(int(self.dl.sum())) / np.float32(self.n) if self.n else F0
        self.norm = norm(self.dl, self.avgdl) if self.n else np.zeros(0, np.float32)
        self.post = {}   # term -> (ordinals ascending, tfs)
        for o, d in enumerate(self.docs):
            for t, tf in d.items():
                self.post.setdefault(t, ([], []))
                self.post[t][0].append(o)
                self.post[t][1].append(tf)
        self.post = {t: (np.array(o, np.int64), np.array(f, np.uint32)) for t, (o, f) in self.post.items()}

    def postings(self, terms) -> int:
        """V: the query's total postings."""
        return sum(self.post[t][0].size for t in terms if t in self.post)

    def search(self, terms, k: int, explain: bool = False):
        """terms: the flattened query.  -> [(record_id, score f32, [(term, idf, tf, contribution)...])], plus the idf of
        each position; term_hits hold every matched position in query order (explain=True), not yet sorted / cut."""
        idfs = [F0] * len(terms)
        if k == 0 or not terms or self.n == 0:
            return [], idfs
        score = np.zeros(self.n, np.float32)
        hit = np.zeros(self.n, bool)
        th = {}
        for j, t in enumerate(terms):
            if t not in self.post:
                continue
            o, tf = self.post[t]
            w = idf(self.n, o.size)
            idfs[j] = w
            c = contribution(w, tf, self.norm[o])
            score[o] = score[o] + c
            hit[o] = True
            if explain:
                for oo, ff, cc in zip(o.tolist(), tf.tolist(), c):
                    th.setdefault(oo, []).append((t, w, ff, np.float32(cc)))
        o = np.nonzero(hit)[0]
        order = np.lexsort((self.ids[o], -score[o]))[:k]
        return [(int(self.ids[o[i]]), score[o[i]], th.get(int(o[i]), [])) for i in order], idfs


def explain_cut(term_hits):
    """bm25.rs:562-575: stable sort by contribution, descending; the first 16."""
    return sorted(term_hits, key=lambda x: x[3], reverse=True)[:TERM_HITS_PER_DOC]


def search_explain_literal(docs: dict, terms, k: int, explain: bool = False):
    """bm25.rs search_explain, statement by statement (the accumulator map, the corpus stats, the scoring loop).
    -> {record_id: (score, term_hits)} of every hit (the reference leaves the order of equal scores open)."""
    if k == 0 or not terms or not docs:
        return {}
    doc_count = len(docs)
    total_doc_len = sum(sum(d.values()) for d in docs.values())
    avgdl = np.float32(total_doc_len) / np.float32(doc_count)
    n = np.float32(doc_count)
    accum, explain_hits = {}, {}
    for term in terms:
        entries = [(rid, d[term]) for rid, d in docs.items() if term in d]
        if not entries:
            continue
        n_with_term = np.float32(len(entries))
        w = logf((n - n_with_term + HALF) / (n_with_term + HALF) + F1)
        for doc_id, tf in entries:
            dl = np.float32(sum(docs[doc_id].values()))
            denom = np.float32(tf) + K1 * (F1 - B + B * dl / max(avgdl, F1))
            contrib = w * (np.float32(tf) * (K1 + F1)) / max(denom, np.float32(1e-6))
            accum[doc_id] = accum.get(doc_id, F0) + contrib
            if explain:
                explain_hits.setdefault(doc_id, []).append((term, w, tf, contrib))
    return {rid: (s, explain_hits.get(rid, [])) for rid, s in accum.items()}


def rrf_ref(rankings, sources, rrf_k: int = 60):
    """matcher/mod.rs rrf_with_sources on (record_id, ...) lists: -> [(record_id, total, vs, bs, vr, br)] in
    (total desc, id asc) order; absent parts are None."""
    acc = {}
    for src, ranking in zip(sources, rankings):
        for r0, rid in enumerate(ranking):
            inc = F1 / (np.float32(rrf_k) + np.float32(r0 + 1))
            e = acc.setdefault(rid, [None, None, None, None])
            i = 1 if src == "bm25" else 0
            e[i] = (F0 if e[i] is None else e[i]) + inc
            if src in ("vector", "bm25") and e[i + 2] is None:
                e[i + 2] = r0 + 1
    out = []
    for rid, (vs, bs, vr, br) in acc.items():
        total = (F0 if vs is None else vs) + (F0 if bs is None else bs)
        out.append((rid, np.float32(total), vs, bs, vr, br))
    out.sort(key=lambda x: (-x[1], x[0]))
    return out
