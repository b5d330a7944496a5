#!/usr/bin/env python3
"""MinHash search timing probe (one GPU).

    python tools/bench_minhash_index.py --n 1000000 10000000 --nq 1 1024

First the answers are checked against the restatement (tests/minhash_index_ref.py): every answer of an index over a
subsample of the rows, and, at each full size, the agreement of every returned row.  Then ms per search at k = 10 (device
events around stream-ordered calls, one warm-up, the median of `--repeats` windows of `--reps` calls), beside
  - for one query, the HBM time of the n x 1024 row bytes,
  - for a batch, the instruction bound of mh_keys: 3 scalar instructions per (query, row) on the one
    scalar unit of a compute unit, one per cycle.
Prints one JSON line per measurement and a last line with all of them; run it under `rocprofv3 --kernel-trace --stats`
for the per-kernel split."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 6.29e12      # measured copy rate of an MI355X (float4 copy), not the 8 TB/s of the data sheet
ROW_BYTES_STORED = 1024        # the slots of a row (minhash_index.hip)
KEY_BYTES_PER_PASS = 1 << 30   # kKeyBytes
CUS, CLOCK_HZ, SALU_PER_PAIR = 256, 2.4e9, 3
PAIRS_PER_S_BOUND = CUS * CLOCK_HZ / SALU_PER_PAIR


def timed(torch, fn, reps, repeats):
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


def draw(torch, n, base, flips, g, dev):
    """n records on the device: slot i is base_i xor one of four masks, so agreements spread around 32 with ties."""
    out = torch.zeros((n, 129), dtype=torch.int64, device=dev)
    for lo in range(0, n, 1 << 20):
        hi = min(n, lo + (1 << 20))
        out[lo:hi, 1:] = base[None, :] ^ flips[torch.randint(0, 4, (hi - lo, 128), device=dev, generator=g)]
    out[:, 0] = 1
    return out.view(torch.uint8).view(n, 1032)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--check-rows", type=int, default=20_000)
    a = ap.parse_args()
    import numpy as np
    import torch
    import minhash_index_ref as ref
    from ucfp_amd import _lib, index
    assert torch.cuda.is_available(), "no GPU: nothing to measure"
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    base = (torch.randint(0, 1 << 32, (128,), dtype=torch.int64, device=dev, generator=g) << 32) \
        ^ torch.randint(0, 1 << 32, (128,), dtype=torch.int64, device=dev, generator=g)
    flips = torch.tensor([0, 1, 1 << 32, -(1 << 63)], dtype=torch.int64, device=dev)
    nq_max = max(a.nq)
    queries = draw(torch, nq_max, base, flips, g, dev)
    h_q = queries.cpu().numpy()
    results = []

    # every answer of an index over a subsample, against the restatement
    m = min(a.check_rows, min(a.n))
    sub = draw(torch, m, base, flips, g, dev)
    h_sub = sub.cpu().numpy()
    sub_ids = np.arange(m, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ix = index.MinHashIndex(ctx=ctx)
    ix.upsert(0, sub_ids, h_sub)
    nq_c = min(nq_max, 80)
    A = ref.agree_matrix(h_q[:nq_c], h_sub)
    for ma in (0, 1, 40):
        got = ix.query(0, h_q[:nq_c], a.k, ma)
        want = ref.topk_from_agree(sub_ids, A, a.k, ma)
        for x, y in zip(got, want):
            assert x.tobytes() == y.tobytes(), "the subsample index disagrees with the restatement"
    ix.close()
    results.append({"bench": "minhash_index_check", "rows": m, "queries": nq_c, "k": a.k, "equal_to_restatement": True})
    print(json.dumps(results[-1]), flush=True)

    for n in a.n:
        rows = draw(torch, n, base, flips, g, dev)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        ix = index.MinHashIndex(ctx=ctx)
        for lo in range(0, n, 1 << 20):          # in pieces: upsert_dev stages its rows on the host
            cnt = min(1 << 20, n - lo)
            ix.upsert_dev(0, ids[lo:].data_ptr(), rows[lo:].data_ptr(), cnt, st)
        ix.flush()                              # the rebuild is not part of a search
        for nq in a.nq:
            q = queries[:nq]
            o_ids = torch.empty((nq, a.k), dtype=torch.int64, device=dev)
            o_a = torch.empty((nq, a.k), dtype=torch.int32, device=dev)
            o_s = torch.empty((nq, a.k), dtype=torch.float32, device=dev)
            o_n = torch.empty((nq,), dtype=torch.int32, device=dev)

            def go():
                ix.query_dev(0, q.data_ptr(), nq, a.k, 1, o_ids.data_ptr(), o_a.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)
            ms, ms_min, ms_max = timed(torch, go, a.reps, a.repeats)
            assert int(o_n.min().item()) == min(a.k, n)
            # the agreement of every returned row (ids are row numbers), and the order of each list
            c = min(nq, 64)
            got_rows = rows[o_ids[:c].reshape(-1)].cpu().numpy().reshape(c, a.k, 1032)
            h_a = o_a[:c].cpu().numpy()
            for i in range(c):
                assert np.array_equal(ref.agree_matrix(h_q[i:i + 1], got_rows[i])[0], h_a[i]), "a returned agreement is wrong"
                assert (np.diff(h_a[i].astype(np.int64)) <= 0).all()
            per_pass = max(1, min(nq, KEY_BYTES_PER_PASS // (4 * n)))
            passes = -(-nq // per_pass)
            rows_hbm_ms = passes * n * ROW_BYTES_STORED / HBM_BYTES_PER_S * 1e3
            pairs_per_s = n * nq / ms * 1e3
            r = {"bench": "minhash_index_search", "n": n, "nq": nq, "k": a.k, "ms": ms, "ms_min": ms_min, "ms_max": ms_max,
                 "reps": a.reps, "repeats": a.repeats, "qps": nq / ms * 1e3, "pairs_per_s": pairs_per_s, "passes": passes,
                 "queries_per_pass": per_pass, "rows_hbm_ms": rows_hbm_ms}
            if nq == 1:
                r["share_of_hbm_bound"] = rows_hbm_ms / ms
            else:
                r["instruction_bound_pairs_per_s"] = PAIRS_PER_S_BOUND
                r["share_of_instruction_bound"] = pairs_per_s / PAIRS_PER_S_BOUND
                r["key_matrix_hbm_ms"] = 2 * 4 * n * nq / HBM_BYTES_PER_S * 1e3
            results.append(r)
            print(json.dumps(r), flush=True)
        ix.close()
        del rows, ids, ix
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "minhash_index", "results": results}), flush=True)


if __name__ == "__main__":
    main()
