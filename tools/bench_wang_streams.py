"""Streaming Wang: steady-state cost of one ucfp_wang_streams_push_dev over S live streams that each
already hold 10 s of history, for chunks of 0.25 s and 1 s per stream per push; in the same run the offline yardstick,
ucfp_audio_wang_batch_dev over the same chunks taken as S clips.  Times come from device events over --steps pushes.
One JSON line per case on stdout.  Per-kernel times and launches per push: run it under rocprofv3 --kernel-trace --stats
with one --sizes value and a small --steps."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucfp_amd import _lib  # noqa: E402


def synth(n, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32, device=dev) / 8000.0
    x = torch.zeros(n, dtype=torch.float32, device=dev)
    for i in range(8):
        f0 = 110.0 * (1.6 ** i)
        x += 0.06 * torch.sin(2 * np.pi * (f0 * t + 3.0 * torch.sin(0.05 * (i + 1) * t)))
    del t
    x += 0.0158 * torch.randn(n, dtype=torch.float32, device=dev, generator=g)
    return x.clamp_(-0.5, 0.5)


def events_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,4096")
    ap.add_argument("--chunks", default="2000,8000")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--history", type=float, default=10.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for S in [int(v) for v in a.sizes.split(",")]:
        for chunk in [int(v) for v in a.chunks.split(",")]:
            h = C.c_void_p()
            _lib.check(lib.ucfp_wang_streams_create(ctx.handle, 8000, None, S, C.byref(h)))
            slots = np.zeros(S, np.uint32)
            for i in range(S):
                s = C.c_uint32(0)
                _lib.check(lib.ucfp_wang_streams_open(h, C.byref(s)))
                slots[i] = s.value
            fin = np.zeros(S, np.uint8)
            hist = int(a.history * 8000)
            x = synth(S * max(hist, chunk), dev, seed=S * 7 + chunk)
            oo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

            def push(n, cap, out):
                ns = np.full(S, n, np.uint64)
                _lib.check(lib.ucfp_wang_streams_push_dev(h, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S,
                                                          x.data_ptr(), out.data_ptr(), cap, oo.data_ptr(), st))

            ns = np.full(S, hist, np.uint64)
            cap = int(lib.ucfp_wang_streams_max_hashes(h, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S))
            out = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev)
            push(hist, cap, out)                              # the 10 s of history
            ns = np.full(S, chunk, np.uint64)
            cap = 2 * int(lib.ucfp_wang_streams_max_hashes(h, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S)) + 4096
            out = torch.empty((cap, 2), dtype=torch.int32, device=dev)
            for _ in range(5):
                push(chunk, cap, out)
            torch.cuda.synchronize()
            ms = events_ms(lambda: push(chunk, cap, out), a.steps)
            hashes = int(oo[-1].item())
            # the yardstick: the same S chunks as S clips of one offline batch
            offs = torch.arange(S + 1, dtype=torch.int64, device=dev) * chunk
            bcap = int(lib.ucfp_audio_wang_batch_max_hashes(S * chunk, S, 8000, None))
            bout = torch.empty((max(bcap, 1), 2), dtype=torch.int32, device=dev)
            boo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

            def batch():
                _lib.check(lib.ucfp_audio_wang_batch_dev(ctx.handle, x.data_ptr(), offs.data_ptr(), S * chunk, S, 8000,
                                                         None, bout.data_ptr(), bcap, boo.data_ptr(), st))

            for _ in range(5):
                batch()
            torch.cuda.synchronize()
            bms = events_ms(batch, a.steps)
            lib.ucfp_wang_streams_destroy(h)
            audio_s = S * chunk / 8000.0
            print(json.dumps({"case": "wang_streams_push", "streams": S, "chunk_s": chunk / 8000.0, "steps": a.steps,
                              "push_ms": round(ms, 4), "audio_s_per_s": round(audio_s / (ms / 1e3), 1),
                              "hashes_last_push": hashes, "offline_batch_ms": round(bms, 4),
                              "offline_audio_s_per_s": round(audio_s / (bms / 1e3), 1),
                              "push_over_offline": round(ms / bms, 3)}), flush=True)
            del x, out, bout


if __name__ == "__main__":
    main()
