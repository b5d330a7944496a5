"""BM25 on the device (DESIGN A11): rebuild time and queries/s over a synthetic Zipf corpus.

Corpus: n_docs documents of ~100 tokens (Poisson) drawn from a Zipf(1) law over 10^6 terms (rank r with probability
~ 1/r), generated on the device and fed through ucfp_bm25_index_upsert_dev in slices.  Queries: 1-8 terms from the
same law, so many hold stopwords.  Reported per corpus: rebuild (the first flush), queries/s at batch 1, 64 and 1024
(ucfp_bm25_index_query_dev, k = 10), the share of queries on each scoring path, and the postings bytes read per second
(sum over the batch of V x 8 B, V = the query's postings) against 8 TB/s of HBM.
CPU baseline: numpy on one core over the same postings (CSR by term), a dense f32 accumulator of N scores per query
and argpartition for the top k -- a floor for a host implementation, not the reference's redb walk.

    python tools/bench_bm25.py --docs 1000000 [--docs 10000000] [--out results.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB = 1_000_000
LDS_POSTINGS = 6144
HBM = 8e12


def zipf_terms(torch, n, gen):
    u = torch.rand(n, device="cuda", generator=gen, dtype=torch.float64)
    return torch.clamp(torch.exp(u * np.log(VOCAB)).long() - 1, 0, VOCAB - 1)


def build(torch, ix, n_docs, gen, keep=False, slice_docs=1_000_000):
    """-> df per term (host), total pairs, and with `keep` the (doc, term, tf) pairs on the host; the corpus goes in
    through upsert_dev."""
    df = torch.zeros(VOCAB, dtype=torch.int64, device="cuda")
    pairs = 0
    kept = []
    st = torch.cuda.current_stream().cuda_stream
    for d0 in range(0, n_docs, slice_docs):
        nd = min(slice_docs, n_docs - d0)
        lens = torch.poisson(torch.full((nd,), 100.0, device="cuda"), generator=gen).long().clamp_(1, 300)
        doc = torch.repeat_interleave(torch.arange(nd, device="cuda"), lens)
        term = zipf_terms(torch, doc.numel(), gen)
        key, tf = torch.unique(doc * VOCAB + term, sorted=True, return_counts=True)
        d, t = key // VOCAB, key % VOCAB
        offs = torch.zeros(nd + 1, dtype=torch.int64, device="cuda")
        offs[1:] = torch.cumsum(torch.bincount(d, minlength=nd), 0)
        ids = torch.arange(d0, d0 + nd, dtype=torch.int64, device="cuda")
        tf32 = tf.to(torch.int32)
        torch.cuda.synchronize()
        ix.upsert_dev(0, ids.data_ptr(), t.data_ptr(), tf32.data_ptr(), offs.data_ptr(), nd, st)
        df += torch.bincount(t, minlength=VOCAB)
        pairs += t.numel()
        print(f"ingested {d0 + nd} / {n_docs} documents, {pairs} postings", file=sys.stderr, flush=True)
        if keep:
            kept.append(((d + d0).cpu().numpy(), t.cpu().numpy(), tf32.cpu().numpy()))
        del lens, doc, term, key, tf, d, offs, ids, tf32
    host = tuple(np.concatenate(x) for x in zip(*kept)) if keep else None
    return df.cpu().numpy(), pairs, host


def host_postings(n_docs, host):
    """CSR by term of the kept pairs, and norm per document (A11's f32 operations)."""
    d, t, tf = host
    order = np.argsort(t, kind="stable")
    start = np.searchsorted(t[order], np.arange(VOCAB + 1))
    dl = np.bincount(d, weights=tf, minlength=n_docs)
    avgdl = np.float32(dl.sum()) / np.float32(n_docs)
    norm = np.float32(1.2) * (np.float32(0.25) + (np.float32(0.75) * dl.astype(np.float32)) / max(avgdl, np.float32(1)))
    return d[order], tf[order].astype(np.float32), start, norm, np.float32(n_docs)


def queries(rng, nq):
    out = []
    for _ in range(nq):
        m = int(rng.integers(1, 9))
        out.append(np.clip(np.exp(rng.random(m) * np.log(VOCAB)).astype(np.int64) - 1, 0, VOCAB - 1))
    return out


def run_batches(torch, ix, qs, batch, k, reps):
    n = len(qs) // batch * batch
    bufs = []
    for b0 in range(0, n, batch):
        q = qs[b0:b0 + batch]
        keys = torch.from_numpy(np.concatenate(q + [np.zeros(1, np.int64)])).cuda()
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum([x.size for x in q])]).astype(np.int64)).cuda()
        bufs.append((keys, offs))
    o_ids = torch.empty(batch * k, dtype=torch.int64, device="cuda")
    o_s = torch.empty(batch * k, dtype=torch.float32, device="cuda")
    o_n = torch.empty(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def one_pass():
        for keys, offs in bufs:
            ix.query_dev(0, keys.data_ptr(), offs.data_ptr(), batch, k, o_ids.data_ptr(), o_s.data_ptr(), o_n.data_ptr(),
                         stream=st)
        torch.cuda.synchronize()
    one_pass()   # warm-up
    t0 = time.perf_counter()
    for _ in range(reps):
        one_pass()
    return n * reps / (time.perf_counter() - t0), n


def cpu_baseline(ix_post, n_docs, qs, k):
    """numpy, one core: dense accumulator over CSR postings."""
    ords, tfs, start, norm, nf = ix_post
    t0 = time.perf_counter()
    for q in qs:
        acc = np.zeros(n_docs, np.float32)
        for t in q.tolist():
            a, b = start[t], start[t + 1]
            if a == b:
                continue
            df = np.float32(b - a)
            w = np.float32(np.log(np.float32((nf - df + 0.5) / (df + 0.5) + 1)))
            tf = tfs[a:b]
            acc[ords[a:b]] += (w * (tf * np.float32(2.2))) / (tf + norm[ords[a:b]])
        top = np.argpartition(-acc, k)[:k]
        top[np.argsort(-acc[top])]
    return len(qs) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, action="append")
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cpu-queries", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ucfp_amd import _lib
    from ucfp_amd.index import Bm25Index
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    k = 10
    for n_docs in a.docs or [1_000_000]:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(n_docs)
        ix = Bm25Index(ctx=ctx)
        t0 = time.perf_counter()
        keep = bool(a.cpu_queries) and n_docs <= 1_000_000
        df, pairs, host = build(torch, ix, n_docs, gen, keep)
        t_ingest = time.perf_counter() - t0
        t0 = time.perf_counter()
        ix.flush()
        t_rebuild = time.perf_counter() - t0
        rng = np.random.default_rng(1)
        qs = queries(rng, a.nq)
        v = np.array([int(df[q].sum()) for q in qs])
        row = {"docs": n_docs, "postings": pairs, "ingest_s": round(t_ingest, 2), "rebuild_s": round(t_rebuild, 3),
               "share_lds_path": round(float((v <= LDS_POSTINGS).mean()), 4),
               "share_range_path": round(float((v > LDS_POSTINGS).mean()), 4), "mean_V": float(v.mean()), "k": k}
        for batch, nq in ((1, 256), (64, 1024), (1024, a.nq)):
            qps, n = run_batches(torch, ix, qs[:nq], batch, k, a.reps)
            row[f"qps_b{batch}"] = round(qps, 1)
            row[f"postings_GBps_b{batch}"] = round(qps * float(v[:n].mean()) * 8 / 1e9, 1)
            row[f"hbm_frac_b{batch}"] = round(qps * float(v[:n].mean()) * 8 / HBM, 4)
        if keep:   # the same postings on the host (ordinal = doc id: ids are 0..n-1)
            row["cpu_baseline"] = "numpy, one core, CSR by term, dense f32 accumulator of N, argpartition top-k"
            row["cpu_qps"] = round(cpu_baseline(host_postings(n_docs, host), n_docs, qs[:a.cpu_queries], k), 2)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        ix.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
