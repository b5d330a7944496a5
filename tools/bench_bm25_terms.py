"""BM25 terms on the device (DESIGN A23): documents/s and tokens/s of ucfp_bm25_terms_batch_dev in both forms over resident
ASCII text, ucfp_text_simhash_batch_dev over the same bytes in the same run (the same tokenise-and-hash work without
gather, sort and count: the ratio is what counting costs), and Bm25Index(keys="hashed").upsert against the host loop of
Bm25Index().upsert on the same texts.

Corpora (the generator of tools/bench_text_utf8.py, --distinct documents from a seed, tiled): `page`, --docs documents of
--bytes bytes (100 k x 4 KiB), and `short`, --short-docs documents of --short-bytes bytes (1 M x ~90 tokens, the corpus
shape of DESIGN A11).  Every timing is a window of at least --window seconds after two warm-up calls.

    python tools/bench_bm25_terms.py [--docs 100000] [--short-docs 1000000] [--e2e-docs 100000] [--only page|short|e2e]
    rocprofv3 --kernel-trace --stats -- python tools/bench_bm25_terms.py --only page --forms counts --no-simhash   (kernel split)"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_text_utf8 import doc_ascii  # noqa: E402

FORMS = {"counts": 0, "sequence": 1}


def window(torch, call, seconds):
    """-> seconds per call: two warm-up calls, then whole calls until `seconds` have passed."""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while True:
        call()
        torch.cuda.synchronize()
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / reps, reps


def resident(torch, docs, n):
    lens = np.array([len(d) for d in docs], np.int64)[np.arange(n) % len(docs)]
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    small = torch.from_numpy(np.frombuffer(b"".join(docs), np.uint8).copy()).cuda()
    tiles = (n + len(docs) - 1) // len(docs)
    blob = torch.cat([small.repeat(tiles)[:int(offs[n])], torch.zeros(64, dtype=torch.uint8, device="cuda")])
    return blob, torch.from_numpy(offs).cuda(), int(offs[n])


def bench_entry(torch, lib, ctx, name, n, nbytes, a, rng):
    from ucfp_amd import terms
    docs = [doc_ascii(rng, nbytes).encode("ascii") for _ in range(min(a.distinct, n))]
    toks = np.array([len(terms.tokenize(d.decode("ascii"))) for d in docs], np.int64)[np.arange(n) % len(docs)]
    d_blob, d_offs, total = resident(torch, docs, n)
    cap = int(lib.ucfp_bm25_terms_max_pairs(total, n))
    d_keys = torch.zeros(cap, dtype=torch.int64, device="cuda")
    d_tfs = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_po = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_sim = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream or None
    base = {"corpus": name, "docs": n, "mean_bytes": round(total / n, 1), "tokens_per_doc": round(float(toks.mean()), 1)}
    rows = []
    for form in a.forms.split(","):
        def call(f=FORMS[form]):
            rc = lib.ucfp_bm25_terms_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, total, f, d_keys.data_ptr(),
                                               d_tfs.data_ptr(), cap, d_po.data_ptr(), d_st.data_ptr(), stream)
            assert rc == 0, lib.ucfp_last_error()
        sec, reps = window(torch, call, a.window)
        pairs = int(d_po[n].item())
        assert not bool((d_st != 0).any().item()) and (pairs == int(toks.sum()) or form == "counts")
        rows.append(dict(base, entry="bm25_terms", form=form, ms=round(sec * 1e3, 3), calls=reps, docs_per_s=round(n / sec),
                         tokens_per_s=round(int(toks.sum()) / sec), gb_per_s=round(total / sec / 1e9, 2), pairs=pairs))
    if not a.no_simhash:
        def sim():
            rc = lib.ucfp_text_simhash_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, 0, d_sim.data_ptr(), d_st.data_ptr(), stream)
            assert rc == 0, lib.ucfp_last_error()
        sec, reps = window(torch, sim, a.window)
        rows.append(dict(base, entry="text_simhash", form=None, ms=round(sec * 1e3, 3), calls=reps, docs_per_s=round(n / sec),
                         tokens_per_s=None, gb_per_s=round(total / sec / 1e9, 2)))
        for r in rows[:-1]:
            r["ms_over_simhash"] = round(r["ms"] / rows[-1]["ms"], 2)
    for r in rows:
        print(json.dumps(r), flush=True)
    del d_blob, d_keys, d_tfs
    torch.cuda.empty_cache()


def bench_e2e(torch, ctx, n, nbytes, a, rng):
    """One upsert of n texts into a fresh index per mode; the hashed route split into terms_batch and upsert_pairs."""
    from ucfp_amd import terms
    from ucfp_amd.index import Bm25Index
    distinct = [doc_ascii(rng, nbytes) for _ in range(min(a.distinct, n))]
    texts = [distinct[i % len(distinct)] for i in range(n)]
    ids = np.arange(n, dtype=np.uint64)
    terms.terms_batch(texts[:1000], "counts", ctx)                   # warm-up: library, scratch
    row = {"corpus": "e2e", "docs": n, "mean_bytes": nbytes}
    ix = Bm25Index(ctx=ctx, keys="hashed")
    t0 = time.perf_counter()
    ix.upsert(0, ids, texts)
    row["hashed_upsert_s"] = round(time.perf_counter() - t0, 3)
    size_h = ix.size(0)
    ix.close()
    t0 = time.perf_counter()
    keys, tfs, offs, _ = terms.terms_batch(texts, "counts", ctx)
    row["hashed_terms_batch_s"] = round(time.perf_counter() - t0, 3)
    ix = Bm25Index(ctx=ctx, keys="hashed")
    t0 = time.perf_counter()
    ix.upsert_pairs(0, ids, keys, tfs, offs)
    row["hashed_upsert_pairs_s"] = round(time.perf_counter() - t0, 3)     # the copy into the host document table
    ix.close()
    ix = Bm25Index(ctx=ctx)
    t0 = time.perf_counter()
    ix.upsert(0, ids, texts)
    row["numbered_upsert_s"] = round(time.perf_counter() - t0, 3)
    assert ix.size(0) == size_h, (ix.size(0), size_h)
    ix.close()
    row["speedup"] = round(row["numbered_upsert_s"] / row["hashed_upsert_s"], 2)
    row["document_table_share"] = round(row["hashed_upsert_pairs_s"] / (row["hashed_terms_batch_s"] + row["hashed_upsert_pairs_s"]), 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--short-docs", type=int, default=1_000_000)
    ap.add_argument("--short-bytes", type=int, default=560)
    ap.add_argument("--e2e-docs", type=int, default=100_000)
    ap.add_argument("--distinct", type=int, default=2048)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--forms", default="counts,sequence")
    ap.add_argument("--no-simhash", action="store_true")
    ap.add_argument("--only", default="", help="page, short or e2e")
    ap.add_argument("--seed", type=int, default=13)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no number"
    from ucfp_amd import _lib
    torch.cuda.set_device(0)
    lib, ctx = _lib.load(), _lib.default_context(0)
    rng = random.Random(a.seed)
    if a.only in ("", "page"):
        bench_entry(torch, lib, ctx, "page", a.docs, a.bytes, a, rng)
    if a.only in ("", "short"):
        bench_entry(torch, lib, ctx, "short", a.short_docs, a.short_bytes, a, rng)
    if a.only in ("", "e2e"):
        bench_e2e(torch, ctx, a.e2e_docs, a.bytes, a, rng)


if __name__ == "__main__":
    main()
