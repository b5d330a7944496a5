"""Multi-tenant Hamming search against the per-tenant entries (DESIGN M1 - M6; profiles/r31/README.md).

    python tools/bench_index_multi.py --cases a1,a2,b,c,d --reps 7 --out profiles/r31/bench_index_multi.jsonl

One JSON line per case.  Every figure is host wall-clock from the first enqueue to the end of a stream synchronisation --
what a caller waits -- the best of `reps` repetitions after a warm-up, with the median and the worst next to it.

  a1  1024 tenants x 10 000 codes, 1024 queries, one per tenant, k = 10: ONE ucfp_index_search_multi_dev against the only
      way there was: 1024 ucfp_index_search_dev calls of one query each, on one stream and alternating between two
  a2  the same with 4096 tenants x 1000 codes, 4096 queries
  b   64 tenants x 1 M codes, 1024 queries (16 per tenant): multi against 64 grouped ucfp_index_search_dev calls
  c   one tenant x 10 M codes, 1024 queries: multi against the one ucfp_index_search_dev call
  d   256 request threads over 1024 tenants x 10 000 codes: MultiSearchBatcher.submit against the same threads calling
      DeviceIndex.search (Python threads on both sides: the interpreter lock weighs on both alike)
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def stats(ts):
    ts = sorted(ts)
    return {"best_us": round(ts[0] * 1e6, 1), "median_us": round(ts[len(ts) // 2] * 1e6, 1), "worst_us": round(ts[-1] * 1e6, 1)}


def timed(fn, sync, reps):
    fn()
    sync()
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return stats(out)


def build_index(torch, index, ctx, tenants, rows_each, seed):
    ix = index.DeviceIndex(index.HAMMING64, flags=index.APPEND_ONLY, ctx=ctx)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    stream = torch.cuda.current_stream().cuda_stream
    ids = torch.arange(rows_each, dtype=torch.int64, device="cuda")
    for t in range(tenants):
        rows = torch.randint(-2**63, 2**63 - 1, (rows_each,), dtype=torch.int64, device="cuda", generator=g)
        ix.append_dev(t, ids.data_ptr(), rows.data_ptr(), rows_each, stream)
    torch.cuda.synchronize()
    return ix


def search_case(torch, index, lib, ctx, name, tenants, rows_each, nq, k, reps, loop_streams):
    """nq queries spread evenly over the tenants (tenant of query i = i % tenants)."""
    ix = build_index(torch, index, ctx, tenants, rows_each, 31)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    q = torch.randint(-2**63, 2**63 - 1, (nq,), dtype=torch.int64, device="cuda", generator=g)
    t_of = (np.arange(nq) % tenants).astype(np.uint32)
    order = np.argsort(t_of, kind="stable")           # the grouped baseline searches a sorted copy of the queries
    q_sorted = q[torch.from_numpy(order).cuda()].contiguous()
    o_ids = torch.zeros(nq * k, dtype=torch.int64, device="cuda")
    o_sc = torch.zeros(nq * k, dtype=torch.float32, device="cuda")
    o_d = torch.zeros(nq * k, dtype=torch.int32, device="cuda")
    o_c = torch.zeros(nq, dtype=torch.int32, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    sync = torch.cuda.synchronize
    h = ix.handle
    res = {"case": name, "tenants": tenants, "rows_per_tenant": rows_each, "queries": nq, "k": k, "reps": reps}

    def multi():
        ix.search_multi_dev(t_of, q.data_ptr(), nq, k, o_ids.data_ptr(), o_sc.data_ptr(), o_d.data_ptr(), o_c.data_ptr(),
                            streams[0].cuda_stream)
    res["multi"] = timed(multi, sync, reps)
    got_ids = o_ids.cpu().numpy().reshape(nq, k).copy()
    got_d = o_d.cpu().numpy().reshape(nq, k).copy()

    per = nq // tenants                                # queries of each tenant, contiguous in q_sorted

    def grouped(ns):
        def run():
            for t in range(tenants):
                lo = t * per
                lib.ucfp_index_search_dev(h, t, q_sorted.data_ptr() + 8 * lo, per, k, o_ids.data_ptr() + 8 * lo * k,
                                          o_sc.data_ptr() + 4 * lo * k, o_d.data_ptr() + 4 * lo * k, o_c.data_ptr() + 4 * lo,
                                          streams[t % ns].cuda_stream)
        return run
    assert nq % tenants == 0
    for ns in loop_streams:
        res[f"per_tenant_calls_{ns}_stream"] = timed(grouped(ns), sync, reps)
    # the two ways agree (rows of the grouped run are in sorted order)
    ref_ids = o_ids.cpu().numpy().reshape(nq, k)
    ref_d = o_d.cpu().numpy().reshape(nq, k)
    res["equal"] = bool(np.array_equal(got_ids[order], ref_ids) and np.array_equal(got_d[order], ref_d))
    res["calls_per_tenant_loop"] = tenants
    ix.close()
    return res


def batcher_case(torch, index, ctx, reps, threads=256, tenants=1024, rows_each=10_000, per_thread=40, k=10):
    ix = build_index(torch, index, ctx, tenants, rows_each, 41)
    rng = np.random.default_rng(3)
    plans = [(rng.integers(0, tenants, per_thread), rng.integers(0, 2**63, per_thread, dtype=np.uint64)) for _ in range(threads)]
    b = index.MultiSearchBatcher(ix, max_batch=256)

    def run(fn):
        def work(p):
            for t, q in zip(*p):
                fn(int(t), q)
        ths = [threading.Thread(target=work, args=(p,)) for p in plans]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        return threads * per_thread / (time.perf_counter() - t0)

    direct = lambda t, q: ix.search(t, np.array([q], np.uint64), k)      # noqa: E731
    batched = lambda t, q: b.submit(t, int(q), k)                          # noqa: E731
    run(direct), run(batched)
    r_direct = sorted(run(direct) for _ in range(reps))
    b0, i0 = b.stats()
    r_batched = sorted(run(batched) for _ in range(reps))
    b1, i1 = b.stats()
    b.close()
    ix.close()
    return {"case": "d", "threads": threads, "tenants": tenants, "rows_per_tenant": rows_each, "k": k, "reps": reps,
            "direct_search_qps": {"best": round(r_direct[-1]), "median": round(r_direct[len(r_direct) // 2]), "worst": round(r_direct[0])},
            "multi_batcher_qps": {"best": round(r_batched[-1]), "median": round(r_batched[len(r_batched) // 2]), "worst": round(r_batched[0])},
            "mean_batch": round((i1 - i0) / max(b1 - b0, 1), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a1,a2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 5, "at least five repetitions"
    import torch
    from ucfp_amd import _lib, index
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    lines = []
    for c in a.cases.split(","):
        if c == "a1":
            r = search_case(torch, index, lib, ctx, "a1", 1024, 10_000, 1024, 10, a.reps, (1, 2))
        elif c == "a2":
            r = search_case(torch, index, lib, ctx, "a2", 4096, 1000, 4096, 10, a.reps, (1, 2))
        elif c == "b":
            r = search_case(torch, index, lib, ctx, "b", 64, 1_000_000, 1024, 10, a.reps, (1, 2))
        elif c == "c":
            r = search_case(torch, index, lib, ctx, "c", 1, 10_000_000, 1024, 10, a.reps, (1,))
        elif c == "d":
            r = batcher_case(torch, index, ctx, a.reps)
        else:
            raise SystemExit(f"unknown case {c}")
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
