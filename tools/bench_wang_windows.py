"""Live Wang windows: what the ring costs a push and what the windows calls cost.  S live streams
(default 4096) receive one chunk of one second per push; feed i plays clip i mod R of R distinct one-second noise clips
over and over.  In the same run, rounds alternating: ucfp_wang_streams_push_dev on a set without windows (W = 0) and on
one with W = 625, ucfp_wang_streams_windows_dev for all S slots, and for Q feeds (default 1024) windows_dev ->
ucfp_landmark_index_query_dev against an index of the R clips, each tiled to --record-s seconds.  Times come from device
events over the calls of a round (the query chain synchronises inside the index, so its time is wall time between the
events).  One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucfp_amd import _lib, audio, index  # noqa: E402


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
    ap.add_argument("--window-frames", type=int, default=625)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--query-feeds", type=int, default=1024)
    ap.add_argument("--records", type=int, default=256)
    ap.add_argument("--record-s", type=int, default=12)
    ap.add_argument("--k", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    S, sr, chunk, W, Q, R, k = a.streams, 8000, 8000, a.window_frames, min(a.query_feeds, a.streams), a.records, a.k
    assert S % R == 0 and W > 0
    sets = {}
    for name, w in (("w0", 0), ("win", W)):
        h = C.c_void_p()
        _lib.check(lib.ucfp_wang_streams_create_ex(ctx.handle, sr, None, S, w, C.byref(h)))
        for i in range(S):
            s = C.c_uint32(0)
            _lib.check(lib.ucfp_wang_streams_open(h, C.byref(s)))
            assert s.value == i
        sets[name] = h
    slots = np.arange(S, dtype=np.uint32)
    fin = np.zeros(S, np.uint8)
    ns = np.full(S, chunk, np.uint64)
    g = torch.Generator(device=dev)
    g.manual_seed(22)
    clips = 0.3 * torch.randn((R, chunk), dtype=torch.float32, device=dev, generator=g)
    x = clips.repeat(S // R, 1).reshape(-1).contiguous()          # feed i plays clip i mod R
    cap = S * 3 * 30 * 10                                          # a push of one second emits anchors of <= 3 seconds
    out = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    oo = torch.zeros(S + 1, dtype=torch.int64, device=dev)

    def push(h):
        _lib.check(lib.ucfp_wang_streams_push_dev(h, slots.ctypes.data, ns.ctypes.data, fin.ctypes.data, S, x.data_ptr(),
                                                  out.data_ptr(), cap, oo.data_ptr(), st))

    wcap = int(lib.ucfp_wang_streams_window_cap(None, W))
    win = torch.empty((S * wcap, 2), dtype=torch.int32, device=dev)
    win_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    win_org = torch.zeros(S, dtype=torch.int32, device=dev)

    def windows(n):
        _lib.check(lib.ucfp_wang_streams_windows_dev(sets["win"], slots.ctypes.data, n, win.data_ptr(), n * wcap,
                                                     win_off.data_ptr(), win_org.data_ptr(), st))

    ix = index.LandmarkIndex(ctx=ctx)
    recs = audio.wang_hashes_batch([c.repeat(a.record_s).cpu().numpy() for c in clips], sr, ctx=ctx)
    ix.upsert(0, np.arange(R, dtype=np.uint64) + 1, recs)
    ix.flush()
    postings = ix.size(0)[1]
    o_ids = torch.zeros((Q, k), dtype=torch.int64, device=dev)
    o_v, o_o = (torch.zeros((Q, k), dtype=torch.int32, device=dev) for _ in range(2))
    o_s = torch.zeros((Q, k), dtype=torch.float32, device=dev)
    o_n = torch.zeros(Q, dtype=torch.int32, device=dev)

    def identify():
        windows(Q)
        ix.query_dev(0, win.data_ptr(), win_off.data_ptr(), Q, k, 2, o_ids.data_ptr(), o_v.data_ptr(), o_o.data_ptr(),
                     o_s.data_ptr(), o_n.data_ptr(), st)

    for _ in range(-(-W // 62) + 3):             # the streams reach their steady state once the windows are full
        push(sets["w0"])
        push(sets["win"])
    windows(S)
    identify()
    torch.cuda.synchronize()
    top = int((o_ids[:, 0].cpu().numpy() == (np.arange(Q) % R) + 1).sum())
    t = {"w0": [], "win": [], "windows": [], "identify": []}
    for _ in range(a.rounds):
        t["w0"].append(events_ms(lambda: push(sets["w0"]), a.pushes))
        t["win"].append(events_ms(lambda: push(sets["win"]), a.pushes))
        t["windows"].append(events_ms(lambda: windows(S), a.pushes))
        t["identify"].append(events_ms(identify, 4))
    hashes = int(oo[-1].item())
    windows(S)
    torch.cuda.synchronize()
    held = int(win_off[-1].item()) // 8
    for h in sets.values():
        lib.ucfp_wang_streams_destroy(h)
    med = {n: statistics.median(v) for n, v in t.items()}
    series = {n + "_ms_series": [round(v, 4) for v in vs] for n, vs in t.items()}
    print(json.dumps({
        "case": "wang_windows", "streams": S, "pushes_per_round": a.pushes, "rounds": a.rounds, "window_frames": W,
        "window_cap": wcap, "state_bytes_w0": int(lib.ucfp_wang_streams_state_bytes_ex(None, 0)),
        "state_bytes_win": int(lib.ucfp_wang_streams_state_bytes_ex(None, W)),
        "push_w0_ms": round(med["w0"], 4), "push_win_ms": round(med["win"], 4),
        "win_over_w0": round(med["win"] / med["w0"], 4), "hashes_per_push": hashes,
        "windows_ms": round(med["windows"], 4), "window_hashes": held,
        "identify_feeds": Q, "index_records": R, "index_record_s": a.record_s, "index_postings": postings, "k": k,
        "identify_ms": round(med["identify"], 4), "identify_top_hits_right": top, **series}), flush=True)


if __name__ == "__main__":
    main()
