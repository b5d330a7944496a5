#!/usr/bin/env python3
"""TLSH timing probe (one GPU).

    python tools/bench_tlsh.py digest --docs 1000000
        TLSH digests/s over the synthetic 4 KiB documents of bench.py's text leg, beside the
        MinHash kernel's rate on the same blob in the same run and the HBM time of the bytes (4096 + 35 per document)
    python tools/bench_tlsh.py search --n 1000000 10000000 --nq 1 64 1024
        ms per search at k = 10 over random rows, beside the HBM time of the stored rows (52 bytes each, read once
        per pass of the query batch)

Prints one JSON line per measurement; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12     # measured copy rate of an MI355X (float4 copy), not the 8 TB/s of the data sheet
ROW_BYTES_STORED = 52         # 13 dword planes per row (tlsh_index.hip)
KEY_BYTES_PER_PASS = 1 << 30  # kKeyBytes


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


def digest(a):
    import torch
    import bench
    from ucfp_amd import _lib
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    lib = _lib.load()
    n, doc_len = a.docs, 4096
    blob = bench.synth_docs_dev(n, doc_len, dev, 0xD0C5)
    offs = (torch.arange(n + 1, dtype=torch.int64, device=dev) * doc_len).contiguous()
    st = torch.empty((n,), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    out_t = torch.empty((n, 35), dtype=torch.uint8, device=dev)
    out_m = torch.empty((n, 1032), dtype=torch.uint8, device=dev)

    def tlsh():
        _lib.check(lib.ucfp_text_tlsh_batch_dev(ctx.handle, blob.data_ptr(), offs.data_ptr(), n, out_t.data_ptr(), st.data_ptr(), s))

    def minhash():
        _lib.check(lib.ucfp_text_minhash_batch_dev(ctx.handle, blob.data_ptr(), offs.data_ptr(), n, 0, 5, out_m.data_ptr(),
                                                   st.data_ptr(), s))
    ms_t = timed(torch, tlsh, a.reps)
    assert int(st.abs().sum().item()) == 0, "a synthetic document was refused"
    ms_m = timed(torch, minhash, a.reps)
    ms_t2 = timed(torch, tlsh, a.reps)        # again after the other kernel: the spread of the same code in one run
    # the other form of the checksum chain (table registers walked with v_readlane), alternating with the default
    ref_out = out_t.clone()
    os.environ["UCFP_TLSH_CHAIN"] = "readlane"
    ms_r = timed(torch, tlsh, a.reps)
    same = bool(torch.equal(ref_out, out_t))
    del os.environ["UCFP_TLSH_CHAIN"]
    ms_t3 = timed(torch, tlsh, a.reps)
    os.environ["UCFP_TLSH_CHAIN"] = "readlane"
    ms_r2 = timed(torch, tlsh, a.reps)
    del os.environ["UCFP_TLSH_CHAIN"]
    hbm_ms = n * (doc_len + 35) / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"bench": "tlsh_digest", "docs": n, "doc_bytes": doc_len, "ms": ms_t, "ms_repeat": ms_t2,
                      "docs_per_s": n / ms_t * 1e3, "GB_per_s": n * (doc_len + 35) / ms_t / 1e6, "hbm_ms": hbm_ms,
                      "share_of_hbm_bound": hbm_ms / ms_t, "ms_third": ms_t3, "readlane_chain_ms": ms_r, "readlane_chain_ms_repeat": ms_r2, "readlane_chain_same_digests": same,
                      "minhash_ms": ms_m, "minhash_docs_per_s": n / ms_m * 1e3,
                      "digest_sample": bytes(out_t[0].cpu().numpy()).hex()}), flush=True)


def search(a):
    import torch
    from ucfp_amd import _lib, index
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    st = torch.cuda.current_stream().cuda_stream
    for n in a.n:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        rows = torch.randint(0, 256, (n, 35), dtype=torch.uint8, device=dev, generator=g)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        ix = index.TlshIndex(ctx=ctx)
        ix.upsert_dev(0, ids.data_ptr(), rows.data_ptr(), n, st)
        ix.flush()                              # the rebuild is not part of a search
        for nq in a.nq:
            q = rows[torch.randint(0, n, (nq,), device=dev, generator=g)].clone()
            q[:, 3:8] = torch.randint(0, 256, (nq, 5), dtype=torch.uint8, device=dev, generator=g)   # near a stored row, not equal
            o_ids = torch.empty((nq, a.k), dtype=torch.int64, device=dev)
            o_d = torch.empty((nq, a.k), dtype=torch.int32, device=dev)
            o_s = torch.empty((nq, a.k), dtype=torch.float32, device=dev)
            o_n = torch.empty((nq,), dtype=torch.int32, device=dev)

            def go():
                ix.query_dev(0, q.data_ptr(), nq, a.k, 0xFFFFFFFF, o_ids.data_ptr(), o_d.data_ptr(), o_s.data_ptr(),
                             o_n.data_ptr(), st)
            ms = timed(torch, go, a.reps)
            assert int(o_n.min().item()) == min(a.k, n)
            per_pass = max(1, min(nq, KEY_BYTES_PER_PASS // (4 * n)))
            passes = -(-nq // per_pass)
            hbm_ms = passes * n * ROW_BYTES_STORED / HBM_BYTES_PER_S * 1e3
            print(json.dumps({"bench": "tlsh_search", "n": n, "nq": nq, "k": a.k, "ms": ms, "qps": nq / ms * 1e3,
                              "G_pairs_per_s": n * nq / ms / 1e6, "passes": passes, "rows_hbm_ms": hbm_ms,
                              "key_matrix_hbm_ms": 2 * 4 * n * nq / HBM_BYTES_PER_S * 1e3}), flush=True)
        ix.close()
        del rows, ids


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("digest")
    d.add_argument("--docs", type=int, default=1_000_000)
    d.add_argument("--reps", type=int, default=3)
    s = sub.add_parser("search")
    s.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    s.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    s.add_argument("--k", type=int, default=10)
    s.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    {"digest": digest, "search": search}[a.cmd](a)


if __name__ == "__main__":
    main()
