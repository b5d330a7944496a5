"""Streaming MinHash: rate of ucfp_text_streams_push_dev over S live streams, each advanced by one chunk
(default 4 KiB) of bench.py's synthetic ASCII documents per push, over P pushes; in the same run the offline yardstick,
ucfp_text_minhash_batch_dev over the same bytes taken as S * P documents.  Times come from device events around the P
pushes.  One JSON line on stdout.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats with a small --pushes.

UTF-8 legs (`utf8` in the result, skipped with --no-utf8): the same S x P shape over RAW_UTF8 streams of a set created
with UCFP_TEXT_STREAMS_UTF8, once on Latin prose with diacritics and once on Han / kana text (the generators of
tools/bench_text_utf8.py; every chunk is a valid UTF-8 document of `chunk` bytes, so the offline call can take the same
bytes as S x P documents), with, in the same run, (a) ucfp_text_minhash_batch_dev in mode RAW_UTF8 over the same bytes,
(b) the ASCII stream leg above and (c) StreamingMinHashSession on its host route (decode, canonicalise and tokenise on
the host, cut at ASCII whitespace) and on its device route over --session-docs of the same chunks, wall clock."""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from ucfp_amd import _lib  # noqa: E402


def utf8_leg(kind, a, ctx, lib, dev, st, ascii_ratio):
    """One UTF-8 kind: RAW_UTF8 streams against the offline call in mode 2 over the same bytes, and the session routes."""
    import bench_text_utf8 as gen
    from ucfp_amd import text as T
    S, P, chunk = a.streams, a.pushes, a.chunk
    rng = random.Random(0xC0DE + len(kind))
    make = {"latin": gen.doc_latin, "cjk": gen.doc_cjk}[kind]
    pool = [make(rng, chunk).encode("utf-8").ljust(chunk, b" ") for _ in range(a.pool)]
    assert all(len(d) == chunk for d in pool)
    d_pool = torch.from_numpy(np.frombuffer(b"".join(pool), np.uint8).reshape(a.pool, chunk).copy()).to(dev)
    pick = (torch.arange(S * P, device=dev) * 7 + 3) % a.pool        # push p carries chunk p * S + i for stream i
    blob = d_pool[pick].contiguous()
    n_bytes = np.full(S, chunk, np.uint64)
    d_status = torch.zeros(S, dtype=torch.int32, device=dev)
    d_out = torch.zeros((S, 1032), dtype=torch.uint8, device=dev)
    h = C.c_void_p()
    _lib.check(lib.ucfp_text_streams_create_ex(ctx.handle, 5, S, T.STREAMS_UTF8, S * chunk, C.byref(h)))

    def run_streams():
        slots = np.zeros(S, np.uint32)
        for i in range(S):
            s = C.c_uint32(0)
            _lib.check(lib.ucfp_text_streams_open(h, T.RAW_UTF8, C.byref(s)))
            slots[i] = s.value
        none, last = np.zeros(S, np.uint8), np.ones(S, np.uint8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for p in range(P):
            _lib.check(lib.ucfp_text_streams_push_dev(h, slots.ctypes.data, n_bytes.ctypes.data,
                                                      (last if p == P - 1 else none).ctypes.data, S, blob[p * S].data_ptr(),
                                                      d_out.data_ptr(), d_status.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        assert int(d_status.abs().sum().item()) == 0
        return e0.elapsed_time(e1)

    run_streams()
    ms = min(run_streams() for _ in range(a.repeats))
    lib.ucfp_text_streams_destroy(h)

    offs = (torch.arange(S * P + 1, dtype=torch.int64, device=dev) * chunk).contiguous()
    bout = torch.empty((S * P, 1032), dtype=torch.uint8, device=dev)
    bst = torch.empty(S * P, dtype=torch.int32, device=dev)

    def run_offline():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.ucfp_text_minhash_batch_dev(ctx.handle, blob.data_ptr(), offs.data_ptr(), S * P, T.RAW_UTF8, 5,
                                                   bout.data_ptr(), bst.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        assert int(bst.abs().sum().item()) == 0
        return e0.elapsed_time(e1)

    run_offline()
    bms = min(run_offline() for _ in range(a.repeats))

    def run_sessions(host: bool):
        """--session-docs chunks through sessions of P pushes each, wall clock; -> (chunks per second, routes seen)."""
        routes, n = set(), 0
        t0 = time.perf_counter()
        while n < a.session_docs:
            sess = T.StreamingMinHashSession(T.TextOpts(), 1, n)
            if host:
                sess._utf8_ok = False                     # the route every non-ASCII stream took before UTF-8 streams
            for p in range(P):
                sess.push(pool[(n * 7 + 3) % a.pool])
                n += 1
            sess.finalize()
            routes.add(sess.route)
        return n / (time.perf_counter() - t0), sorted(routes)

    run_sessions(False)
    host_rate, host_routes = run_sessions(True)
    dev_rate, dev_routes = run_sessions(False)
    total = S * P * chunk
    ratio = bms / ms
    return {"state_bytes": int(lib.ucfp_text_streams_state_bytes_ex(T.STREAMS_UTF8)),
            "stream_ms": round(ms, 3), "stream_GBs": round(total / (ms / 1e3) / 1e9, 3),
            "stream_pushes_per_s": round(S * P / (ms / 1e3), 1),
            "offline_mode2_ms": round(bms, 3), "offline_mode2_docs_per_s": round(S * P / (bms / 1e3), 1),
            "stream_over_offline_rate": round(ratio, 3), "ascii_stream_over_offline_rate": round(ascii_ratio, 3),
            "session_chunks": a.session_docs, "session_host_route_chunks_per_s": round(host_rate, 1),
            "session_host_routes": host_routes, "session_device_route_chunks_per_s": round(dev_rate, 1),
            "session_device_routes": dev_routes,
            "stream_over_session_host_route": round(S * P / (ms / 1e3) / host_rate, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--pushes", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-utf8", action="store_true")
    ap.add_argument("--pool", type=int, default=512, help="distinct chunk documents per UTF-8 kind")
    ap.add_argument("--session-docs", type=int, default=256, help="chunks pushed through sessions, 32 per session")
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
    del blob
    utf8 = {} if a.no_utf8 else {kind: utf8_leg(kind, a, ctx, lib, dev, st, bms / ms) for kind in ("latin", "cjk")}
    print(json.dumps({"case": "text_streams_push", "streams": S, "pushes": P, "chunk_bytes": chunk,
                      "state_bytes": int(lib.ucfp_text_streams_state_bytes()), "repeats": a.repeats,
                      "stream_ms": round(ms, 3), "stream_GBs": round(total / (ms / 1e3) / 1e9, 3),
                      "pushes_per_s": round(P / (ms / 1e3), 1), "stream_pushes_per_s": round(S * P / (ms / 1e3), 1),
                      "offline_ms": round(bms, 3), "offline_GBs": round(total / (bms / 1e3) / 1e9, 3),
                      "offline_docs_per_s": round(S * P / (bms / 1e3), 1),
                      "stream_over_offline_rate": round(bms / ms, 3), "utf8": utf8}), flush=True)


if __name__ == "__main__":
    main()
