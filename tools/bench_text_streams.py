"""Streaming MinHash: rate of ucfp_text_streams_push_dev over S live streams, each advanced by one chunk
(default 4 KiB) of bench.py's synthetic ASCII documents per push, over P pushes; in the same run the offline yardstick,
ucfp_text_minhash_batch_dev over the same bytes taken as S * P documents.  Times come from device events around the P
pushes.  One JSON line on stdout.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats with a small --pushes."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ucfp_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--pushes", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    S, P, chunk = a.streams, a.pushes, a.chunk
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    # push p carries document p * S + i for stream i: the chunks of one push are contiguous
    blob = bench.synth_docs_dev(S * P, chunk, dev, 0xD0C5)
    n_bytes = np.full(S, chunk, np.uint64)
    d_status = torch.zeros(S, dtype=torch.int32, device=dev)
    d_out = torch.zeros((S, 1032), dtype=torch.uint8, device=dev)
    h = C.c_void_p()
    _lib.check(lib.ucfp_text_streams_create(ctx.handle, 5, S, C.byref(h)))

    def run_streams():
        slots = np.zeros(S, np.uint32)
        for i in range(S):
            s = C.c_uint32(0)
            _lib.check(lib.ucfp_text_streams_open(h, 0, C.byref(s)))
            slots[i] = s.value
        none, last = np.zeros(S, np.uint8), np.ones(S, np.uint8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for p in range(P):
            fin = last if p == P - 1 else none
            _lib.check(lib.ucfp_text_streams_push_dev(h, slots.ctypes.data, n_bytes.ctypes.data, fin.ctypes.data, S,
                                                      blob[p * S].data_ptr(), d_out.data_ptr(), d_status.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        assert int(d_status.abs().sum().item()) == 0
        return e0.elapsed_time(e1)

    run_streams()                                             # warm-up: every slot is used and freed once
    ms = min(run_streams() for _ in range(a.repeats))

    offs = (torch.arange(S * P + 1, dtype=torch.int64, device=dev) * chunk).contiguous()
    bout = torch.empty((S * P, 1032), dtype=torch.uint8, device=dev)
    bst = torch.empty(S * P, dtype=torch.int32, device=dev)

    def run_offline():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.ucfp_text_minhash_batch_dev(ctx.handle, blob.data_ptr(), offs.data_ptr(), S * P, 0, 5,
                                                   bout.data_ptr(), bst.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    run_offline()
    bms = min(run_offline() for _ in range(a.repeats))
    lib.ucfp_text_streams_destroy(h)
    total = S * P * chunk
    print(json.dumps({"case": "text_streams_push", "streams": S, "pushes": P, "chunk_bytes": chunk,
                      "state_bytes": int(lib.ucfp_text_streams_state_bytes()), "repeats": a.repeats,
                      "stream_ms": round(ms, 3), "stream_GBs": round(total / (ms / 1e3) / 1e9, 3),
                      "pushes_per_s": round(P / (ms / 1e3), 1), "stream_pushes_per_s": round(S * P / (ms / 1e3), 1),
                      "offline_ms": round(bms, 3), "offline_GBs": round(total / (bms / 1e3) / 1e9, 3),
                      "offline_docs_per_s": round(S * P / (bms / 1e3), 1),
                      "stream_over_offline_rate": round(bms / ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
