"""Matcher -- host-side mirror of src/matcher/mod.rs: reciprocal rank fusion (RRF, :22-98) and the query-shape dispatch
of `Matcher::search` (:140-207) over a GpuIndex.

    rrf(rankings, rrf_k)                        :22-24
    rrf_with_sources(rankings, sources, rrf_k)  :26-98   every entry adds 1 / (rrf_k + rank) in f32 to its source's part
    search(index, q)                            :140-207 vector + terms -> knn and bm25 fused by RRF; vector -> knn;
                                                         terms -> bm25; neither -> []

The reference leaves the order of equal fused scores to its HashMap; here ties go by ascending record id (DESIGN A11)."""
from typing import List, Optional, Sequence

import numpy as np

from .core import Hit, HitSource

RRF_K = 60   # Query::default (src/core/mod.rs:185)


def rrf(rankings: Sequence[Sequence[Hit]], rrf_k: int = RRF_K) -> List[Hit]:
    return rrf_with_sources(rankings, [], rrf_k)


def rrf_with_sources(rankings: Sequence[Sequence[Hit]], sources: Sequence[str], rrf_k: int = RRF_K) -> List[Hit]:
    """Fused hits (source "fused"): vector_score / bm25_score = the per-source sums of 1 / (rrf_k + rank1) in f32,
    vector_rank / bm25_rank = the first rank in each list, score = vector part + bm25 part; (score desc, id asc).
    A ranking whose source is neither vector nor bm25 folds into vector_score without a rank (matcher/mod.rs:70-75)."""
    denom = np.float32(rrf_k)
    acc = {}   # (tenant, record) -> [vs, bs, vr, br]
    for i, ranking in enumerate(rankings):
        src = sources[i] if i < len(sources) else (ranking[0].source if ranking else HitSource.Fused)
        for rank0, hit in enumerate(ranking):
            rank1 = rank0 + 1
            inc = np.float32(1.0) / (denom + np.float32(rank1))
            e = acc.setdefault((hit.tenant_id, hit.record_id), [None, None, None, None])
            if src == HitSource.Bm25:
                e[1] = (e[1] if e[1] is not None else np.float32(0.0)) + inc
                e[3] = e[3] if e[3] is not None else rank1
            else:
                e[0] = (e[0] if e[0] is not None else np.float32(0.0)) + inc
                if src == HitSource.Vector:
                    e[2] = e[2] if e[2] is not None else rank1
    out = []
    for (tenant, record), (vs, bs, vr, br) in acc.items():
        total = (vs if vs is not None else np.float32(0.0)) + (bs if bs is not None else np.float32(0.0))
        out.append(Hit(tenant_id=tenant, record_id=record, score=float(total), source=HitSource.Fused,
                       vector_score=None if vs is None else float(vs), bm25_score=None if bs is None else float(bs),
                       vector_rank=vr, bm25_rank=br))
    out.sort(key=lambda h: (-h.score, h.record_id, h.tenant_id))
    return out


def search(index, q) -> List[Hit]:
    """Matcher::search over an IndexBackend-shaped `index` (knn, bm25); the result is truncated to q.k."""
    vector: Optional[Sequence[float]] = q.vector
    terms = list(getattr(q, "terms", None) or [])
    explain = bool(getattr(q, "explain", False))
    filt = getattr(q, "filter", None)
    rrf_k = getattr(q, "rrf_k", RRF_K)
    if vector is not None and terms:
        vec_hits = index.knn(q.tenant_id, vector, q.k, filt)
        bm_hits = index.bm25(q.tenant_id, terms, q.k, filt, explain)
        fused = rrf_with_sources([vec_hits, bm_hits], [HitSource.Vector, HitSource.Bm25], rrf_k)
        if explain:
            by_id = {(h.tenant_id, h.record_id): h.term_hits for h in bm_hits if h.term_hits}
            for h in fused:
                th = by_id.pop((h.tenant_id, h.record_id), None)
                if th is not None:
                    h.term_hits = th
    elif vector is not None:
        fused = index.knn(q.tenant_id, vector, q.k, filt)
    elif terms:
        fused = index.bm25(q.tenant_id, terms, q.k, filt, explain)
    else:
        fused = []
    return fused[:q.k]
