"""Corpus de-duplication on the device (DESIGN "LSH" L5-L7): time per ucfp_lsh_dedup_dev call and per kernel.

Corpora: n synthetic MinHash-128 records (BASELINE configs[3]: 1 M documents + a 16 x 8 band index), generated on the
device from slot matrices.  `dup0` / `dup10` / `dup50`: that share of the rows are copies of other rows, half of them
exact and half keeping each slot with probability 0.9; `heavy`: 10^5 identical rows among distinct ones.  Rows are
shuffled.  Per corpus and per mode (`skip`: a candidate whose rows already share a root is not verified; `noskip`:
every candidate is, UCFP_LSH_DEDUP_NO_SKIP=1) one JSON line: build ms, dedup ms per call (median of --reps, events on
the stream), the kernels' times from the profiler when it is available, the stats, and for `noskip` -- where the
verified partners are exactly `pairs` -- the link kernel's bytes per second (bands x n x 8 B of keys + 1 KiB per
partner).

--baseline adds the only route there is without this entry point, on the same corpus: LshIndex.query of every row at
k = 128, results copied to the host, a numpy union-find over the hits with agreement >= min_agree.  It answers a
slightly different question: a query sees at most cand_per_band rows per band and 1024 candidates in all.

    python tools/bench_dedup.py [--n 1000000] [--corpora dup0,dup10,dup50,heavy] [--baseline] [--out results.jsonl]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def corpus(torch, name, n, gen):
    """-> records uint8 [n, 1032] on the device."""
    slots = torch.randint(0, 1 << 62, (n, 128), device="cuda", generator=gen, dtype=torch.int64)
    if name == "heavy":
        m = min(100_000, n)
        slots[:m] = slots[0]
    else:
        d = int(n * {"dup0": 0.0, "dup10": 0.1, "dup50": 0.5}[name])
        if d:
            src = torch.randint(0, n - d, (d,), device="cuda", generator=gen)
            copy = slots[src]
            near = torch.rand((d, 128), device="cuda", generator=gen) < 0.9
            near[: d // 2] = True                                   # the first half: exact copies
            slots[n - d:] = torch.where(near, copy, slots[n - d:])
    slots = slots[torch.randperm(n, device="cuda", generator=gen)]
    rec = torch.zeros((n, 1032), dtype=torch.uint8, device="cuda")
    rec[:, 0] = 1
    rec[:, 8:] = slots.view(torch.uint8).reshape(n, 1024)
    return rec


def kernel_times(torch, fn):
    """{kernel: microseconds} of one call, from the profiler; None when it is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            m = re.search(r"dedup_\w+", e.name)
            if m:
                out[m.group(0)] = out.get(m.group(0), 0.0) + float(e.device_time)
        return out or None
    except Exception as ex:       # the profiler is optional equipment
        print(f"profiler unavailable: {ex}", file=sys.stderr)
        return None


def timed(torch, fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms))


def union_find_numpy(n, a, b):
    lab = np.arange(n, dtype=np.int64)
    while True:
        la, lb = lab[a], lab[b]
        m = la != lb
        if not m.any():
            return lab
        np.minimum.at(lab, np.maximum(la[m], lb[m]), np.minimum(la[m], lb[m]))
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def baseline(torch, idx, rec, n, min_agree, chunk=65536, k=128):
    """query every row, copy the hits to the host, union-find there.  ids are the row numbers."""
    st = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    ea, eb = [], []
    t_query = t_copy = 0.0
    for q0 in range(0, n, chunk):
        nq = min(chunk, n - q0)
        o_ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        o_sc = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        o_ct = torch.empty(nq, dtype=torch.int32, device="cuda")
        t = time.perf_counter()
        idx.query_dev(rec[q0:].data_ptr(), nq, k, o_ids.data_ptr(), o_sc.data_ptr(), o_ct.data_ptr(), st)
        torch.cuda.synchronize()
        t_query += time.perf_counter() - t
        t = time.perf_counter()
        h_ids, h_sc = o_ids.cpu().numpy(), o_sc.cpu().numpy()
        t_copy += time.perf_counter() - t
        hit = h_sc >= np.float32(min_agree) / np.float32(128)
        r, c = np.nonzero(hit)
        ea.append(r + q0)
        eb.append(h_ids[r, c])
    t = time.perf_counter()
    lab = union_find_numpy(n, np.concatenate(ea), np.concatenate(eb))
    t_uf = time.perf_counter() - t
    return {"total_s": time.perf_counter() - t0, "query_s": t_query, "copy_s": t_copy, "union_find_s": t_uf,
            "clusters": int((lab == np.arange(n)).sum()), "k": k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--corpora", default="dup0,dup10,dup50,heavy")
    ap.add_argument("--bands", type=int, default=16)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--span", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--modes", default="skip,noskip")
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from ucfp_amd import _lib, text
    assert torch.cuda.is_available(), "needs a GPU"
    ctx = _lib.default_context(0)
    n, min_agree = args.n, text.min_agree_for(args.threshold)
    st = torch.cuda.current_stream().cuda_stream
    out = open(args.out, "a") if args.out else None
    for name in args.corpora.split(","):
        gen = torch.Generator(device="cuda").manual_seed(1234)
        rec = corpus(torch, name, n, gen)
        ids = torch.arange(n, dtype=torch.int64, device="cuda")
        idx = text.LshIndex(args.bands, args.rows, ctx=ctx)
        torch.cuda.synchronize()
        build_ms = timed(torch, lambda: idx.build_dev(ids.data_ptr(), rec.data_ptr(), n, st), 3)[0]
        lab = torch.empty(n, dtype=torch.int32, device="cuda")
        rep = torch.empty(n, dtype=torch.int64, device="cuda")
        keep = torch.empty(n, dtype=torch.uint8, device="cuda")
        stats = torch.zeros(4, dtype=torch.int64, device="cuda")

        def call():
            idx.dedup_dev(min_agree, args.span, lab.data_ptr(), rep.data_ptr(), keep.data_ptr(), stats.data_ptr(), st)

        for mode in args.modes.split(","):
            if mode == "noskip":
                os.environ["UCFP_LSH_DEDUP_NO_SKIP"] = "1"
            else:
                os.environ.pop("UCFP_LSH_DEDUP_NO_SKIP", None)
            call()
            torch.cuda.synchronize()
            med, best = timed(torch, call, args.reps)
            s = [int(x) for x in stats.cpu().numpy().view(np.uint64)]
            kern = kernel_times(torch, call)
            line = {"corpus": name, "mode": mode, "n": n, "bands": args.bands, "rows": args.rows, "min_agree": min_agree,
                    "span": args.span, "build_ms": round(build_ms, 3), "dedup_ms": round(med, 4),
                    "dedup_ms_best": round(best, 4), "rows_per_s": round(n / (med * 1e-3)), "kernels_us": kern,
                    "pairs": s[0], "clusters": s[1], "duplicates": s[2], "largest": s[3]}
            if mode == "noskip" and kern and kern.get("dedup_link_kernel"):
                b = args.bands * n * 8 + s[0] * 1024
                line["link_bytes"] = b
                line["link_TBps"] = round(b / (kern["dedup_link_kernel"] * 1e-6) / 1e12, 3)
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
        os.environ.pop("UCFP_LSH_DEDUP_NO_SKIP", None)
        if args.baseline and name != "heavy":
            line = {"corpus": name, "mode": "baseline_query_all_rows", "n": n, **baseline(torch, idx, rec, n, min_agree)}
            line = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in line.items()}
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
        idx.close()
        del rec, ids, lab, rep, keep
    if out:
        out.close()


if __name__ == "__main__":
    main()
