#!/usr/bin/env python3
"""Filtered search timing probe (one GPU).

    python tools/bench_index_filter.py [--out profiles/r30] [--hamming-rows 10000000] [--cosine-rows 1000000] [--shares 0.1]

Two things are measured, each as the median of `--repeats` runs with their minimum and maximum:

  view build   ucfp_index_filter_create (host clock: parse + copies + probe + scan + read-back + gather) and
               ucfp_index_filter_refresh followed by a device synchronise (the same without the first allocation), at
               0.1 / 1 / 10 / 50 / 100 % of the rows allowed, for ascending and for shuffled ids; beside them the HBM time
               of the id bytes the probe must read and of the bytes the gather must read and write.  Each refresh is
               also split into its stages by the device events the library keeps (ucfp_index_filter_build_ms): probe,
               scan, read-back (the row count's copy, the host's wake-up, the allocation of the view) and gather.
  search       ucfp_index_search_filtered_dev on a view against ucfp_index_search_dev on a dedicated index of the same
               allowed rows, in the same run, the two alternating; the answers are compared bit for bit first.

Writes bench_index_filter.json and README.md (the tables) into --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.29e12      # measured copy rate of an MI355X (float4 copy), not the 8 TB/s of the data sheet
SHARES = (0.001, 0.01, 0.1, 0.5, 1.0)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "runs": len(xs)}


def time_build(torch, ix, data, repeats):
    """create (host clock) once per repeat on a fresh view; refresh + synchronise on the last one, with its stages."""
    create, refresh = [], []
    stages = {"probe": [], "scan": [], "readback": [], "gather": []}
    view = None
    for _ in range(repeats):
        if view is not None:
            view.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        view = ix.filter(0, data)
        torch.cuda.synchronize()
        create.append((time.perf_counter() - t0) * 1e3)
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        view.refresh()
        torch.cuda.synchronize()
        refresh.append((time.perf_counter() - t0) * 1e3)
        for name, ms in view.build_ms().items():
            stages[name].append(ms)
    return view, spread(create), spread(refresh), {name: spread(v) for name, v in stages.items()}


def time_pair(torch, fa, fb, reps, repeats):
    """Two stream-ordered calls timed alternately with device events: ms per call of each."""
    fa()
    fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(repeats):
        for j, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[j].append(e0.elapsed_time(e1) / reps)
    return spread(out[0]), spread(out[1])


def outputs(torch, nq, k, dev):
    return (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
            torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq,), dtype=torch.int32, device=dev))


def run_kind(torch, np, index, ctx, a, kind, results):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(30)
    hamming = kind == "hamming"
    n = a.hamming_rows if hamming else a.cosine_rows
    dim = 0 if hamming else a.dim
    row_bytes = 8 if hamming else 4 * dim
    nqs = (1, 256, 4096) if hamming else (1, 16, 256)
    if hamming:
        rows = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)
        queries = torch.randint(-2**63, 2**63 - 1, (max(nqs),), dtype=torch.int64, device=dev, generator=g)
    else:
        rows = torch.randn((n, dim), dtype=torch.float32, device=dev, generator=g)
        queries = torch.randn((max(nqs), dim), dtype=torch.float32, device=dev, generator=g)
    rng = np.random.default_rng(30)
    base_ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    for order in (("ascending", "shuffled") if hamming else ("ascending",)):
        ids_np = base_ids if order == "ascending" else rng.permutation(base_ids)
        ids = torch.from_numpy(ids_np.view(np.int64)).to(dev)
        ix = index.DeviceIndex(index.HAMMING64 if hamming else index.COSINE_F32, dim, index.APPEND_ONLY, ctx)
        ix.append_dev(0, ids.data_ptr(), rows.data_ptr(), n, st)
        ix.flush()
        for share in a.shares:
            mask = np.ones(n, bool) if share == 1.0 else rng.random(n) < share
            allowed = int(mask.sum())
            t0 = time.perf_counter()
            data = index.filter_bytes(ids_np[mask])
            write_ms = (time.perf_counter() - t0) * 1e3
            view, create, refresh, stages = time_build(torch, ix, data, a.repeats)
            stats = view.stats()
            assert stats["rows_allowed"] == allowed and stats["rows_seen"] == n
            r = {"bench": "filter_view_build", "kind": kind, "ids": order, "rows": n, "dim": dim, "share": share, "allowed": allowed,
                 "filter_bytes": len(data), "containers": stats["containers"], "device_bytes": stats["device_bytes"],
                 "filter_bytes_write_ms": write_ms, "create_ms": create, "refresh_ms": refresh, "stages_ms": stages,
                 "ids_hbm_ms": n * 8 / HBM_BYTES_PER_S * 1e3,
                 "gather_hbm_ms": 2 * allowed * (8 + row_bytes + (0 if hamming else 4)) / HBM_BYTES_PER_S * 1e3}
            r["refresh_over_hbm_bound"] = refresh["median"] / (r["ids_hbm_ms"] + r["gather_hbm_ms"])
            results.append(r)
            print(json.dumps(r), flush=True)
            if order == "ascending" and share in a.search_shares:
                t_mask = torch.from_numpy(mask).to(dev)
                d = index.DeviceIndex(ix.kind, dim, index.APPEND_ONLY, ctx)
                d_rows, d_ids = rows[t_mask].contiguous(), ids[t_mask].contiguous()
                d.append_dev(0, d_ids.data_ptr(), d_rows.data_ptr(), allowed, st)
                d.flush()
                for nq in nqs:
                    q = queries[:nq]
                    ov, od = outputs(torch, nq, a.k, dev), outputs(torch, nq, a.k, dev)

                    def on_view():
                        ix.search_dev(0, q.data_ptr(), nq, a.k, ov[0].data_ptr(), ov[1].data_ptr(), ov[2].data_ptr(),
                                      ov[3].data_ptr(), st, view)

                    def on_dedicated():
                        d.search_dev(0, q.data_ptr(), nq, a.k, od[0].data_ptr(), od[1].data_ptr(), od[2].data_ptr(),
                                     od[3].data_ptr(), st)
                    on_view()
                    on_dedicated()
                    torch.cuda.synchronize()
                    equal = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                            y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(ov, od))
                    assert equal, "a view and the dedicated index of its rows disagree"
                    reps = max(1, min(20, 2000 // nq))
                    tv, td = time_pair(torch, on_view, on_dedicated, reps, a.repeats)
                    s = {"bench": "filter_view_search", "kind": kind, "rows": n, "dim": dim, "share": share, "allowed": allowed,
                         "nq": nq, "k": a.k, "reps": reps, "view_ms": tv, "dedicated_ms": td, "bit_equal": True,
                         "view_over_dedicated": tv["median"] / td["median"]}
                    results.append(s)
                    print(json.dumps(s), flush=True)
                d.close()
                del d_rows, d_ids, d
            view.close()
        ix.close()
        del ids, ix
        torch.cuda.empty_cache()


def fmt(s):
    return f"{s['median']:.3f} ({s['min']:.3f} – {s['max']:.3f})"


def write_readme(path, results, a):
    out = ["# Filtered search: view build and search on a view (`tools/bench_index_filter.py`)", "",
           f"One MI355X; every figure is the median of {a.repeats} runs with (minimum – maximum), in milliseconds.  `create` is "
           "`ucfp_index_filter_create` on the host clock (parse, copies, probe, scan, the one read-back, allocation, gather, "
           "synchronised), `refresh` is `ucfp_index_filter_refresh` + a device synchronise.  `ids HBM` / `gather HBM` are the times "
           f"the id bytes and the gathered bytes (read + write) take at {HBM_BYTES_PER_S / 1e12:.2f} TB/s.", "",
           "## View build", "",
           "| kind | ids | rows | allowed | containers | filter bytes | create | refresh | ids HBM | gather HBM | refresh / (ids + gather HBM) |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    stage_rows = ["", "## Stages of a refresh on the device (events around each stage; `read-back` = the copy of the row count, the host's "
                  "wake-up and the allocation of the view; what `refresh` has beyond their sum is host work: parsing, copies up, "
                  "freeing the old view)", "",
                  "| kind | ids | allowed | probe | scan | read-back | gather | probe / ids HBM |", "|---|---|---|---|---|---|---|---|"]
    for r in results:
        if r["bench"] == "filter_view_build":
            out.append(f"| {r['kind']}{' dim ' + str(r['dim']) if r['dim'] else ''} | {r['ids']} | {r['rows']} | {r['allowed']} "
                       f"({100 * r['share']:g} %) | {r['containers']} | {r['filter_bytes']} | {fmt(r['create_ms'])} | "
                       f"{fmt(r['refresh_ms'])} | {r['ids_hbm_ms']:.4f} | {r['gather_hbm_ms']:.4f} | {r['refresh_over_hbm_bound']:.1f} |")
            g = r["stages_ms"]
            stage_rows.append(f"| {r['kind']}{' dim ' + str(r['dim']) if r['dim'] else ''} | {r['ids']} | {r['allowed']} ({100 * r['share']:g} %) | "
                              f"{fmt(g['probe'])} | {fmt(g['scan'])} | {fmt(g['readback'])} | {fmt(g['gather'])} | "
                              f"{g['probe']['median'] / r['ids_hbm_ms']:.1f} |")
    out += stage_rows
    out += ["", "## Search on a view against a dedicated index of the same rows (same run, alternating; answers bit-equal)", "",
            "| kind | rows | allowed | queries | view | dedicated | view / dedicated |", "|---|---|---|---|---|---|---|"]
    for r in results:
        if r["bench"] == "filter_view_search":
            out.append(f"| {r['kind']}{' dim ' + str(r['dim']) if r['dim'] else ''} | {r['rows']} | {r['allowed']} ({100 * r['share']:g} %) | "
                       f"{r['nq']} | {fmt(r['view_ms'])} | {fmt(r['dedicated_ms'])} | {r['view_over_dedicated']:.3f} |")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30"))
    ap.add_argument("--hamming-rows", type=int, default=10_000_000)
    ap.add_argument("--cosine-rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shares", type=float, nargs="+", default=list(SHARES), help="shares of the rows the filters allow")
    ap.add_argument("--search-shares", type=float, nargs="*", default=[0.1, 1.0])
    a = ap.parse_args()
    assert a.repeats >= 7, "medians of at least 7 runs"
    import numpy as np
    import torch
    from ucfp_amd import _lib, index
    assert torch.cuda.is_available(), "no GPU: nothing to measure"
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    results = []
    if a.hamming_rows:
        run_kind(torch, np, index, ctx, a, "hamming", results)
    if a.cosine_rows:
        run_kind(torch, np, index, ctx, a, "cosine", results)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "bench_index_filter.json"), "w") as f:
        json.dump({"bench": "index_filter", "hbm_bytes_per_s": HBM_BYTES_PER_S, "results": results}, f, indent=1)
    write_readme(os.path.join(a.out, "README.md"), results, a)
    print(json.dumps({"bench": "index_filter", "written": a.out, "measurements": len(results)}), flush=True)


if __name__ == "__main__":
    main()
