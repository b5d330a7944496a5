#!/usr/bin/env python3
"""Image match timing probe (one GPU).

    python tools/bench_image_match.py --n 1000000 10000000 --nq 1 16 256 1024
        ms per search at k = 10 over random records, bundles (536 bytes) and single-algorithm records (168), beside the
        HBM time of the stored code planes (408 or 136 bytes per row, read once per pass of the query batch) and the
        time the instruction count predicts (397 or 134 vector instructions per (query, row))

Every index answers a sample of its queries against the restatement (tests/image_match_ref.py): the scores of the ids
it returned, bit for bit, and no row of a random sample of the stored rows may beat the last hit.
Prints one JSON line per measurement; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 6.29e12        # measured copy rate of an MI355X (float4 copy), not the 8 TB/s of the data sheet
LANE_OPS_PER_S = 39.3e12         # 256 CUs x 64 lanes x 2.4 GHz: one vector instruction per lane and clock
KEY_BYTES_PER_PASS = 1 << 30     # kKeyBytes
ALGO = {536: 7, 168: 2}          # UCFP_IMG_MULTI, UCFP_IMG_PHASH
PLANE_BYTES = {536: 408, 168: 136}
INSTR_PER_PAIR = {536: 397, 168: 134}   # vector instructions in the query loop of im_keys<3> / im_keys<1> as compiled for gfx950


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def check_sample(torch, np, ref, rows, q, o_ids, o_s, o_n, k, n, g):
    """The first two queries against the restatement; ids are row numbers here."""
    dev = rows.device
    sample = torch.randint(0, n, (min(n, 100_000),), device=dev, generator=g)
    h_sample = rows[sample].cpu().numpy()
    for qi in range(min(2, q.shape[0])):
        cnt = int(o_n[qi].item())
        assert cnt == min(k, n), (cnt, k, n)
        ids = o_ids[qi, :cnt].cpu().numpy()
        got = o_s[qi, :cnt].cpu().numpy()
        hq = q[qi:qi + 1].cpu().numpy()
        want = ref.score_matrix(hq, rows[torch.from_numpy(ids).to(dev)].cpu().numpy())[0]
        assert got.tobytes() == want.tobytes(), "a returned score differs from the restatement"
        key = list(zip((-got.astype(np.float64)).tolist(), ids.tolist()))
        assert key == sorted(key), "hits are not ordered (score desc, id asc)"
        s = ref.score_matrix(hq, h_sample)[0]
        better = (s > got[-1]) | ((s == got[-1]) & (sample.cpu().numpy() < ids[-1]))
        missing = set(sample.cpu().numpy()[better].tolist()) - set(ids.tolist())
        assert not missing, f"rows that beat the last hit are missing: {sorted(missing)[:4]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--sizes", type=int, nargs="+", default=[536, 168], choices=[536, 168])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    import image_match_ref as ref
    from ucfp_amd import _lib, index
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    st = torch.cuda.current_stream().cuda_stream
    for size in a.sizes:
        for n in a.n:
            g = torch.Generator(device=dev)
            g.manual_seed(1)
            rows = torch.randint(0, 256, (n, size), dtype=torch.uint8, device=dev, generator=g)
            ids = torch.arange(n, dtype=torch.int64, device=dev)
            ix = index.ImageMatchIndex(ALGO[size], 0, ctx)
            step = 1 << 20                          # the row table is built on the host: ingest in pieces
            for lo in range(0, n, step):
                m = min(step, n - lo)
                ix.upsert_dev(0, ids[lo:].data_ptr(), rows[lo:].data_ptr(), m, st)
            ix.flush()                              # the rebuild is not part of a search
            for nq in a.nq:
                q = rows[torch.randint(0, n, (nq,), device=dev, generator=g)].clone()
                # a local edit: two blocks of every algorithm replaced, as a caption or a logo would
                for s0 in ([32] if size == 168 else [64, 232, 400]):
                    q[:, s0 + 8:s0 + 24] = torch.randint(0, 256, (nq, 16), dtype=torch.uint8, device=dev, generator=g)
                o_ids = torch.empty((nq, a.k), dtype=torch.int64, device=dev)
                o_s = torch.empty((nq, a.k), dtype=torch.float32, device=dev)
                o_n = torch.empty((nq,), dtype=torch.int32, device=dev)

                def go():
                    ix.query_dev(0, q.data_ptr(), nq, a.k, None, o_ids.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)
                ms = timed(torch, go, a.reps)
                check_sample(torch, np, ref, rows, q, o_ids, o_s, o_n, a.k, n, g)
                per_pass = max(1, min(nq, KEY_BYTES_PER_PASS // (4 * n)))
                passes = -(-nq // per_pass)
                hbm_ms = passes * n * PLANE_BYTES[size] / HBM_BYTES_PER_S * 1e3
                alu_ms = n * nq * INSTR_PER_PAIR[size] / LANE_OPS_PER_S * 1e3
                print(json.dumps({"bench": "image_match_search", "record_bytes": size, "n": n, "nq": nq, "k": a.k, "ms": ms,
                                  "qps": nq / ms * 1e3, "G_pairs_per_s": n * nq / ms / 1e6, "passes": passes,
                                  "rows_hbm_ms": hbm_ms, "share_of_rows_hbm_bound": hbm_ms / ms,
                                  "instruction_count_ms": alu_ms, "share_of_instruction_bound": alu_ms / ms,
                                  "key_matrix_hbm_ms": 2 * 4 * n * nq / HBM_BYTES_PER_S * 1e3,
                                  "sample_checked": True}), flush=True)
            ix.close()
            del rows, ids


if __name__ == "__main__":
    main()
