"""Streaming Panako: steady-state cost of ucfp_panako_streams_push_dev over S live streams that each
receive one chunk per push (default 4096 streams, 32 pushes of one second at 8 kHz, windows of W = 625 frames).  In the
same run, over the same samples: ucfp_wang_streams_push_dev (the same front end with pairs behind it),
ucfp_audio_panako_batch_dev (the samples taken as S offline clips) and ucfp_panako_streams_windows_dev for all S slots.
Times come from device events over the calls of a round; rounds of the four alternate.  One JSON line on stdout.
Per-kernel times and launches per push: run it under rocprofv3 --kernel-trace --stats with --rounds 1.
With --sample-rate other than 8000 the two sets come from the _sr entries and resample on the device, the
offline batch runs at that rate, and a second Panako set at 8 kHz is pushed over the same seconds of audio in the same
rounds (`push_8k_ms`)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--chunk-s", type=float, default=1.0)
    ap.add_argument("--window-frames", type=int, default=625)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sample-rate", type=int, default=8000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S, sr, chunk, W = a.streams, a.sample_rate, int(a.chunk_s * a.sample_rate), a.window_frames
    pc, wc = _lib.PanakoConfig(5, 96, 96, 30, -50.0), _lib.WangConfig(10, 63, 64, 30, -50.0)
    hp, hw, h8 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    if sr == 8000:
        _lib.check(lib.ucfp_panako_streams_create(ctx.handle, sr, C.byref(pc), S, W, C.byref(hp)))
        _lib.check(lib.ucfp_wang_streams_create(ctx.handle, sr, C.byref(wc), S, C.byref(hw)))
    else:
        _lib.check(lib.ucfp_panako_streams_create_sr(ctx.handle, sr, C.byref(pc), S, W, C.byref(hp)))
        _lib.check(lib.ucfp_wang_streams_create_sr(ctx.handle, sr, C.byref(wc), S, 0, C.byref(hw)))
        _lib.check(lib.ucfp_panako_streams_create(ctx.handle, 8000, C.byref(pc), S, W, C.byref(h8)))
    slots = np.zeros(S, np.uint32)
    for i in range(S):
        s, t = C.c_uint32(0), C.c_uint32(0)
        _lib.check(lib.ucfp_panako_streams_open(hp, C.byref(s)))
        _lib.check(lib.ucfp_wang_streams_open(hw, C.byref(t)))
        assert s.value == t.value
        slots[i] = s.value
        if h8:
            _lib.check(lib.ucfp_panako_streams_open(h8, C.byref(t)))
            assert s.value == t.value
    fin = np.zeros(S, np.uint8)
    ns = np.full(S, chunk, np.uint64)
    g = torch.Generator(device=dev)
    g.manual_seed(19)
    x = 0.3 * torch.randn(S * chunk, dtype=torch.float32, device=dev, generator=g)
    secs = int(a.chunk_s) + 2                     # seconds of anchors one push can emit
    pcap, wcap = S * secs * 30 * 5, S * secs * 30 * 10
    pout = torch.empty((pcap, 4), dtype=torch.int32, device=dev)
    wout = torch.empty((wcap, 2), dtype=torch.int32, device=dev)
    poo = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    woo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

    def push():
        _lib.check(lib.ucfp_panako_streams_push_dev(hp, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S, x.data_ptr(),
                                                    pout.data_ptr(), pcap, poo.data_ptr(), st))

    def wang_push():
        _lib.check(lib.ucfp_wang_streams_push_dev(hw, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S, x.data_ptr(),
                                                  wout.data_ptr(), wcap, woo.data_ptr(), st))

    chunk8 = int(a.chunk_s * 8000)                # the same seconds of audio at 8 kHz
    ns8 = np.full(S, chunk8, np.uint64)
    x8 = 0.3 * torch.randn(S * chunk8, dtype=torch.float32, device=dev, generator=g) if h8 else None

    def push_8k():
        _lib.check(lib.ucfp_panako_streams_push_dev(h8, slots.ctypes.data, ns8.ctypes.data, fin.ctypes.data, S,
                                                    x8.data_ptr(), pout.data_ptr(), pcap, poo.data_ptr(), st))

    offs = torch.arange(S + 1, dtype=torch.int64, device=dev) * chunk
    bcap = int(lib.ucfp_audio_panako_batch_max_hashes(S * chunk, S, sr, C.byref(pc)))
    bout = torch.empty((max(bcap, 1), 4), dtype=torch.int32, device=dev)
    boo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

    def batch():
        _lib.check(lib.ucfp_audio_panako_batch_dev(ctx.handle, x.data_ptr(), offs.data_ptr(), S * chunk, S, sr, C.byref(pc),
                                                   bout.data_ptr(), bcap, boo.data_ptr(), st))

    wrec = int(lib.ucfp_panako_streams_window_cap(C.byref(pc), W))
    win = torch.empty((max(S * wrec, 1), 4), dtype=torch.int32, device=dev)
    win_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    win_org = torch.zeros(S, dtype=torch.int32, device=dev)

    def windows():
        _lib.check(lib.ucfp_panako_streams_windows_dev(hp, slots.ctypes.data, S, win.data_ptr(), S * wrec,
                                                       win_off.data_ptr(), win_org.data_ptr(), st))

    warm = max(3, -(-W // 62) + 3)               # the streams reach their steady state once the windows are full
    for _ in range(warm):
        push()
        wang_push()
        if h8:
            push_8k()
    batch()
    if W:
        windows()
    torch.cuda.synchronize()
    push_ms, wang_ms, batch_ms, win_ms, push8_ms = [], [], [], [], []
    for _ in range(a.rounds):
        if h8:
            push8_ms.append(events_ms(push_8k, a.pushes))
        push_ms.append(events_ms(push, a.pushes))
        wang_ms.append(events_ms(wang_push, a.pushes))
        batch_ms.append(events_ms(batch, a.pushes))
        if W:
            win_ms.append(events_ms(windows, a.pushes))
    # the host's share: one plan of all S entries (max_hashes plans a push and changes nothing; a push plans once more)
    t0 = time.perf_counter()
    for _ in range(50):
        lib.ucfp_panako_streams_max_hashes(hp, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S)
    plan_ms = (time.perf_counter() - t0) / 50 * 1e3
    recs, pairs, brecs = int(poo[-1].item()), int(woo[-1].item()), int(boo[-1].item())
    wrecs = int(win_off[-1].item()) // 16 if W else 0
    lib.ucfp_panako_streams_destroy(hp)
    if h8:
        lib.ucfp_panako_streams_destroy(h8)
    lib.ucfp_wang_streams_destroy(hw)
    p, w, b = statistics.median(push_ms), statistics.median(wang_ms), statistics.median(batch_ms)
    v = statistics.median(win_ms) if W else 0.0
    audio_s = S * chunk / sr
    mm = lambda xs: [round(min(xs), 4), round(max(xs), 4)] if xs else []   # noqa: E731
    extra = {}
    if h8:
        p8 = statistics.median(push8_ms)
        extra = {"push_8k_ms": round(p8, 4), "push_8k_ms_min_max": mm(push8_ms), "push_over_push_8k": round(p / p8, 3)}
        sb = int(lib.ucfp_panako_streams_state_bytes_sr(C.byref(pc), W, sr))
    else:
        sb = int(lib.ucfp_panako_streams_state_bytes(C.byref(pc), W))
    print(json.dumps({
        "case": "panako_streams_push", "streams": S, "rate": sr, "chunk_s": a.chunk_s, "pushes_per_round": a.pushes,
        "rounds": a.rounds, "window_frames": W,
        "state_bytes_per_stream": sb,
        "push_ms": round(p, 4), "push_ms_min_max": mm(push_ms), "x_real_time": round(audio_s / (p / 1e3), 1),
        "stream_chunks_per_s": round(S / (p / 1e3), 1), "records_per_push": recs,
        "wang_push_ms": round(w, 4), "wang_push_ms_min_max": mm(wang_ms), "wang_hashes_per_push": pairs,
        "push_over_wang_push": round(p / w, 3),
        "offline_batch_ms": round(b, 4), "offline_ms_min_max": mm(batch_ms), "offline_records_per_batch": brecs,
        "offline_x_real_time": round(audio_s / (b / 1e3), 1), "push_over_offline_batch": round(p / b, 3),
        "windows_ms": round(v, 4), "windows_ms_min_max": mm(win_ms), "window_records": wrecs,
        "windows_over_push": round(v / p, 3), "plan_host_ms": round(plan_ms, 4), **extra}), flush=True)


if __name__ == "__main__":
    main()
