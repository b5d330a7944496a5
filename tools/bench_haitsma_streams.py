"""Streaming Haitsma: steady-state cost of ucfp_haitsma_streams_push_dev over S live streams that each
receive one chunk per push (default 4096 streams, 32 pushes of one second at 44.1 kHz); in the same run the offline
yardstick, ucfp_audio_haitsma_batch_dev over the same samples taken as S clips.  A one-second clip holds 47 frames, a
stream emits 78 per second (it keeps its tail), so the comparison is given per second of audio and per frame.  Times
come from device events over the pushes of a round; rounds of the two alternate.  One JSON line on stdout.  Per-kernel
times and launches per push: run it under rocprofv3 --kernel-trace --stats with --rounds 1."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucfp_amd import _lib  # noqa: E402


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
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--pushes", type=int, default=32)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--chunk-s", type=float, default=1.0)
    ap.add_argument("--block-frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S, sr, chunk = a.streams, a.rate, int(a.chunk_s * a.rate)
    h = C.c_void_p()
    _lib.check(lib.ucfp_haitsma_streams_create(ctx.handle, sr, None, S, a.block_frames, C.byref(h)))
    slots = np.zeros(S, np.uint32)
    for i in range(S):
        s = C.c_uint32(0)
        _lib.check(lib.ucfp_haitsma_streams_open(h, C.byref(s)))
        slots[i] = s.value
    fin = np.zeros(S, np.uint8)
    ns = np.full(S, chunk, np.uint64)
    g = torch.Generator(device=dev)
    g.manual_seed(18)
    x = 0.3 * torch.randn(S * chunk, dtype=torch.float32, device=dev, generator=g)
    cap = S * (int(a.chunk_s * 5000) // 64 + 2)
    out = torch.empty(cap, dtype=torch.int32, device=dev)
    oo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

    def push():
        _lib.check(lib.ucfp_haitsma_streams_push_dev(h, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S, x.data_ptr(),
                                                     out.data_ptr(), cap, oo.data_ptr(), st))

    offs = torch.arange(S + 1, dtype=torch.int64, device=dev) * chunk
    bcap = int(lib.ucfp_audio_haitsma_batch_max_frames(S * chunk, S, sr))
    bout = torch.empty(max(bcap, 1), dtype=torch.int32, device=dev)
    boo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

    def batch():
        _lib.check(lib.ucfp_audio_haitsma_batch_dev(ctx.handle, x.data_ptr(), offs.data_ptr(), S * chunk, S, sr, None,
                                                    bout.data_ptr(), bcap, boo.data_ptr(), st))

    for _ in range(3):                       # the streams reach their steady state (a full tail) with the first push
        push()
        batch()
    torch.cuda.synchronize()
    push_ms, batch_ms = [], []
    for _ in range(a.rounds):
        push_ms.append(events_ms(push, a.pushes))
        batch_ms.append(events_ms(batch, a.pushes))
    frames = int(oo[-1].item())
    bframes = int(boo[-1].item())
    lib.ucfp_haitsma_streams_destroy(h)
    p, b = statistics.median(push_ms), statistics.median(batch_ms)
    audio_s = S * chunk / sr
    print(json.dumps({
        "case": "haitsma_streams_push", "streams": S, "rate": sr, "chunk_s": a.chunk_s, "pushes_per_round": a.pushes,
        "rounds": a.rounds, "block_frames": a.block_frames,
        "state_bytes_per_stream": int(lib.ucfp_haitsma_streams_state_bytes(sr, a.block_frames)),
        "push_ms": round(p, 4), "push_ms_min_max": [round(min(push_ms), 4), round(max(push_ms), 4)],
        "x_real_time": round(audio_s / (p / 1e3), 1), "stream_chunks_per_s": round(S / (p / 1e3), 1),
        "frames_per_push": frames, "push_us_per_kframe": round(p * 1e6 / max(frames, 1), 3),
        "offline_batch_ms": round(b, 4), "offline_ms_min_max": [round(min(batch_ms), 4), round(max(batch_ms), 4)],
        "offline_x_real_time": round(audio_s / (b / 1e3), 1), "offline_frames_per_batch": bframes,
        "offline_us_per_kframe": round(b * 1e6 / max(bframes, 1), 3),
        "stream_over_offline_rate": round(b / p, 3),
        "stream_over_offline_rate_per_frame": round((b / max(bframes, 1)) / (p / max(frames, 1)), 3)}), flush=True)


if __name__ == "__main__":
    main()
