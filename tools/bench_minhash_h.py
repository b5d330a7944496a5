#!/usr/bin/env python3
"""MinHash with any slot count H: the two sweeps of DESIGN.md T10 (one GPU).

    python tools/bench_minhash_h.py [--docs 100000] [--rows 1000000]

1. Documents/s of ucfp_text_minhash_h_batch_dev (word tokeniser, RAW_ASCII, k = 5) at H = 64, 128, 256, 1024, and of the
   128-slot entry ucfp_text_minhash_batch_dev, in one process over the same --docs documents of --bytes bytes resident in
   HBM (the English-like generator of tools/bench_text_utf8.py, --distinct documents tiled).  A kernel is timed by device
   events around one call; the median of --reps calls after two warm-ups, beside (max - min) / median.  The H = 64 records
   are compared with the first 64 slots of the H = 1024 ones, and H = 128 with the old entry's.
   The model this tests: tokeniser and XXH3 do not depend on H and the fold is linear in NR = ceil(H / 64) minima per lane.
2. ms per search of ucfp_minhash_index_query_dev at nq = 1 and 1024, k = 10, over --rows rows for H = 64, 128, 256 (device
   events around stream-ordered calls, one warm-up, the median of 5 windows of 3 calls, as tools/bench_minhash_index.py);
   a sample of the answers is checked against the restatement (tests/minhash_h_ref.py).
Prints one JSON line per measurement."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_text_utf8 import doc_ascii  # noqa: E402


def timed_each(torch, call, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), (max(ms) - min(ms)) / statistics.median(ms)


def timed_windows(torch, fn, reps=3, repeats=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out), min(out), max(out)


def sweep_signatures(torch, a):
    from ucfp_amd import _lib, text
    lib, ctx = _lib.load(), _lib.current_context()
    stream = torch.cuda.current_stream().cuda_stream or None
    rng = random.Random(a.seed)
    n = a.docs
    distinct = [doc_ascii(rng, a.bytes).encode("ascii") for _ in range(min(a.distinct, n))]
    pick = np.arange(n) % len(distinct)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(np.array([len(d) for d in distinct], np.int64)[pick], out=offs[1:])
    d_small = torch.from_numpy(np.frombuffer(b"".join(distinct), np.uint8).copy()).cuda()
    tiles = (n + len(distinct) - 1) // len(distinct)
    d_blob = torch.cat([d_small.repeat(tiles)[:int(offs[n])], torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_offs = torch.from_numpy(offs).cuda()
    tokens = int(np.array([len(text._host_tokens(d.decode().lower())) for d in distinct], np.int64)[pick].sum())
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    outs, rows = {}, []

    def run(what, h, call, out):
        ms, spread = timed_each(torch, call, a.reps)
        assert int(d_st.abs().sum().item()) == 0
        r = {"bench": "minhash_h_signatures", "what": what, "h": h, "nr": -(-h // 64), "docs": n, "doc_bytes": a.bytes,
             "tokens_per_doc": round(tokens / n, 1), "ms": round(ms, 3), "spread": round(spread, 3), "docs_per_s": round(n / ms * 1e3)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        outs[what] = out

    old = torch.zeros((n, 1032), dtype=torch.uint8, device="cuda")
    run("ucfp_text_minhash_batch_dev", 128,
        lambda: _lib.check(lib.ucfp_text_minhash_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, text.RAW_ASCII, 5,
                                                           old.data_ptr(), d_st.data_ptr(), stream)), old)
    for h in a.h:
        out = torch.zeros((n, 8 + 8 * h), dtype=torch.uint8, device="cuda")
        run(f"ucfp_text_minhash_h_batch_dev h={h}", h,
            lambda out=out, h=h: _lib.check(lib.ucfp_text_minhash_h_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n,
                                                                              text.RAW_ASCII, text.TOK_WORD, 5, h, out.data_ptr(),
                                                                              d_st.data_ptr(), stream)), out)
    widest = outs[f"ucfp_text_minhash_h_batch_dev h={max(a.h)}"]
    for h in a.h:
        assert torch.equal(outs[f"ucfp_text_minhash_h_batch_dev h={h}"], widest[:, :8 + 8 * h]), f"H = {h} is not a prefix"
    if 128 in a.h:
        assert torch.equal(outs["ucfp_text_minhash_h_batch_dev h=128"], old), "H = 128 differs from the 128-slot entry"
    base = next(r for r in rows if r["what"] == "ucfp_text_minhash_batch_dev")["ms"]
    print(json.dumps({"bench": "minhash_h_signatures_vs_128", "ms_over_old_entry": {str(r["h"]): round(r["ms"] / base, 3)
                                                                                     for r in rows[1:]}}), flush=True)


def sweep_index(torch, a):
    import minhash_h_ref as ref
    from ucfp_amd import _lib, index
    dev = torch.device("cuda", 0)
    ctx = _lib.current_context()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    flips = torch.tensor([0, 1, 1 << 32, -(1 << 63)], dtype=torch.int64, device=dev)
    n, k = a.rows, 10

    def draw(m, base, h):
        """m records: slot i is base_i xor one of four masks, so agreements spread around h / 4 with ties."""
        out = torch.zeros((m, h + 1), dtype=torch.int64, device=dev)
        for lo in range(0, m, 1 << 20):
            hi = min(m, lo + (1 << 20))
            out[lo:hi, 1:] = base[None, :] ^ flips[torch.randint(0, 4, (hi - lo, h), device=dev, generator=g)]
        out[:, 0] = 1
        return out.view(torch.uint8).view(m, 8 + 8 * h)

    for h in a.index_h:
        base = (torch.randint(0, 1 << 32, (h,), dtype=torch.int64, device=dev, generator=g) << 32) \
            ^ torch.randint(0, 1 << 32, (h,), dtype=torch.int64, device=dev, generator=g)
        rows, queries = draw(n, base, h), draw(max(a.nq), base, h)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        ix = index.MinHashIndex(ctx=ctx, h=h)
        for lo in range(0, n, 1 << 20):          # in pieces: upsert_dev stages its rows on the host
            ix.upsert_dev(0, ids[lo:].data_ptr(), rows[lo:].data_ptr(), min(1 << 20, n - lo), st)
        ix.flush()                              # the rebuild is not part of a search
        for nq in a.nq:
            q = queries[:nq]
            o_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
            o_a = torch.empty((nq, k), dtype=torch.int32, device=dev)
            o_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
            o_n = torch.empty((nq,), dtype=torch.int32, device=dev)

            def go():
                ix.query_dev(0, q.data_ptr(), nq, k, 1, o_ids.data_ptr(), o_a.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)
            ms, ms_min, ms_max = timed_windows(torch, go)
            c = min(nq, 16)                     # the agreement of every returned row of the first queries, and their order
            got_rows = rows[o_ids[:c].reshape(-1)].cpu().numpy().reshape(c, k, 8 + 8 * h)
            h_a, h_q = o_a[:c].cpu().numpy(), q[:c].cpu().numpy()
            for i in range(c):
                assert np.array_equal(ref.agree_matrix(h_q[i:i + 1], got_rows[i], h)[0], h_a[i]), "a returned agreement is wrong"
                assert (np.diff(h_a[i].astype(np.int64)) <= 0).all()
            r = {"bench": "minhash_h_index_search", "h": h, "chunks": -(-h // 128), "n": n, "nq": nq, "k": k, "ms": round(ms, 4),
                 "ms_min": round(ms_min, 4), "ms_max": round(ms_max, 4), "qps": round(nq / ms * 1e3, 1),
                 "pairs_per_s": round(n * nq / ms * 1e3), "row_bytes_on_device": 1024 * -(-h // 128)}
            print(json.dumps(r), flush=True)
        ix.close()
        del rows, queries, ids, ix
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--h", type=int, nargs="+", default=[64, 128, 256, 1024])
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows of the index sweep; 0 skips it")
    ap.add_argument("--index-h", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 1024])
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no number"
    if a.docs:
        sweep_signatures(torch, a)
    if a.rows:
        sweep_index(torch, a)


if __name__ == "__main__":
    main()
