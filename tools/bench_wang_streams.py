"""Streaming Wang: steady-state cost of one ucfp_wang_streams_push_dev over S live streams that each
already hold 10 s of history, for chunks of 0.25 s and 1 s per stream per push; in the same run the offline yardstick,
ucfp_audio_wang_batch_dev over the same chunks taken as S clips.  Times come from device events over --steps pushes.
One JSON line per case on stdout.  Per-kernel times and launches per push: run it under rocprofv3 --kernel-trace --stats
with one --sizes value and a small --steps.
--chunks and --history stay in 8 kHz samples and seconds; with --sample-rate other than 8000 the set comes
from ucfp_wang_streams_create_sr and takes the same seconds of audio at that rate, the offline batch runs at that rate,
and a second set at 8 kHz is pushed over the same seconds in the same run (`push_8k_ms`)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucfp_amd import _lib  # noqa: E402


def synth(n, dev, seed, sr=8000):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32, device=dev) / float(sr)
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
    ap.add_argument("--sample-rate", type=int, default=8000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    sr = a.sample_rate
    for S in [int(v) for v in a.sizes.split(",")]:
        for chunk8 in [int(v) for v in a.chunks.split(",")]:
            h, h8 = C.c_void_p(), C.c_void_p()
            if sr == 8000:
                _lib.check(lib.ucfp_wang_streams_create(ctx.handle, 8000, None, S, C.byref(h)))
            else:
                _lib.check(lib.ucfp_wang_streams_create_sr(ctx.handle, sr, None, S, 0, C.byref(h)))
                _lib.check(lib.ucfp_wang_streams_create(ctx.handle, 8000, None, S, C.byref(h8)))
            slots = np.zeros(S, np.uint32)
            for i in range(S):
                s = C.c_uint32(0)
                _lib.check(lib.ucfp_wang_streams_open(h, C.byref(s)))
                slots[i] = s.value
                if h8:
                    _lib.check(lib.ucfp_wang_streams_open(h8, C.byref(s)))
                    assert slots[i] == s.value
            fin = np.zeros(S, np.uint8)
            chunk, hist = chunk8 * sr // 8000, int(a.history * sr)
            x = synth(S * max(hist, chunk), dev, seed=S * 7 + chunk8, sr=sr)
            oo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

            def push(n, cap, out, hh=None, xx=None):
                ns = np.full(S, n, np.uint64)
                _lib.check(lib.ucfp_wang_streams_push_dev(hh or h, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S,
                                                          (x if xx is None else xx).data_ptr(), out.data_ptr(), cap,
                                                          oo.data_ptr(), st))

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
            # the host's share: one plan of all S entries (max_hashes plans a push and changes nothing)
            ns = np.full(S, chunk, np.uint64)
            t0 = time.perf_counter()
            for _ in range(50):
                lib.ucfp_wang_streams_max_hashes(h, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S)
            plan_ms = (time.perf_counter() - t0) / 50 * 1e3
            extra = {}
            if h8:                                            # the same seconds of audio through a set at 8 kHz
                hist8 = int(a.history * 8000)
                x8 = synth(S * max(hist8, chunk8), dev, seed=S * 7 + chunk8)
                ns = np.full(S, hist8, np.uint64)
                hcap = int(lib.ucfp_wang_streams_max_hashes(h8, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S))
                hout = torch.empty((max(hcap, 1), 2), dtype=torch.int32, device=dev)
                push(hist8, hcap, hout, h8, x8)
                del hout
                for _ in range(5):
                    push(chunk8, cap, out, h8, x8)
                torch.cuda.synchronize()
                ms8 = events_ms(lambda: push(chunk8, cap, out, h8, x8), a.steps)
                extra = {"rate": sr, "push_8k_ms": round(ms8, 4), "push_over_push_8k": round(ms / ms8, 3)}
                lib.ucfp_wang_streams_destroy(h8)
                del x8
            # the yardstick: the same S chunks as S clips of one offline batch
            offs = torch.arange(S + 1, dtype=torch.int64, device=dev) * chunk
            bcap = int(lib.ucfp_audio_wang_batch_max_hashes(S * chunk, S, sr, None))
            bout = torch.empty((max(bcap, 1), 2), dtype=torch.int32, device=dev)
            boo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

            def batch():
                _lib.check(lib.ucfp_audio_wang_batch_dev(ctx.handle, x.data_ptr(), offs.data_ptr(), S * chunk, S, sr,
                                                         None, bout.data_ptr(), bcap, boo.data_ptr(), st))

            for _ in range(5):
                batch()
            torch.cuda.synchronize()
            bms = events_ms(batch, a.steps)
            lib.ucfp_wang_streams_destroy(h)
            audio_s = S * chunk8 / 8000.0
            print(json.dumps({"case": "wang_streams_push", "streams": S, "chunk_s": chunk8 / 8000.0, "steps": a.steps,
                              "push_ms": round(ms, 4), "audio_s_per_s": round(audio_s / (ms / 1e3), 1),
                              "hashes_last_push": hashes, "offline_batch_ms": round(bms, 4),
                              "offline_audio_s_per_s": round(audio_s / (bms / 1e3), 1),
                              "push_over_offline": round(ms / bms, 3), "plan_host_ms": round(plan_ms, 4), **extra}),
                  flush=True)
            del x, out, bout


if __name__ == "__main__":
    main()
