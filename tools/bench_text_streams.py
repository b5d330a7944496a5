"""Streaming MinHash: rate of ucfp_text_streams_push_dev over S live streams, each advanced by one chunk
(default 4 KiB) of bench.py's synthetic ASCII documents per push, over P pushes; in the same run the offline yardstick,
ucfp_text_minhash_batch_dev over the same bytes taken as S * P documents.  Times come from device events around the P
pushes.  One JSON line on stdout.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats with a small --pushes.

UTF-8 legs (`utf8` in the result, skipped with --no-utf8): the same S x P shape over RAW_UTF8 streams of a set created
with UCFP_TEXT_STREAMS_UTF8, once on Latin prose with diacritics and once on Han / kana text (the generators of
tools/bench_text_utf8.py; every chunk is a valid UTF-8 document of `chunk` bytes, so the offline call can take the same
bytes as S x P documents), with, in the same run, (a) ucfp_text_minhash_batch_dev in mode RAW_UTF8 over the same bytes,
(b) the ASCII stream leg above and (c) StreamingMinHashSession on its host route (decode, canonicalise and tokenise on
the host, cut at ASCII whitespace) and on its device route over --session-docs of the same chunks, wall clock.

SimHash legs (`simhash` in the result, skipped with --no-simhash): the same S x P shape over sets of
ucfp_text_streams_create_sim, TF and weighted by a table fitted to the leg's own documents, on the ASCII prose above, on
the two UTF-8 corpora and (weighted only) on ASCII documents over a 200 k-word Zipf-like vocabulary; each against
ucfp_text_simhash_batch_dev / ucfp_text_simhash_idf_batch_dev over the same bytes in the same run, after the streams'
records have been compared with the offline records of the concatenated documents."""
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


def simhash_leg(a, ctx, lib, st, rows, mode, table):
    """One SimHash leg: S streams advanced by P pushes of one row of `rows` (uint8 [S * P, chunk] on the
    device; push p carries rows p * S + i for stream i) in mode `mode`, TF or weighted by `table`, against the offline
    entry over the same bytes taken as S * P documents, in the same run.  Before anything is timed the streams' final
    records are compared with the offline records of the S concatenated documents."""
    from ucfp_amd import text as T
    S, P, chunk = a.streams, a.pushes, a.chunk
    dev = rows.device
    utf8 = mode == T.RAW_UTF8
    th = table.handle if table is not None else None
    n_bytes = np.full(S, chunk, np.uint64)
    d_status = torch.zeros(S, dtype=torch.int32, device=dev)
    d_out = torch.zeros((S, 8), dtype=torch.uint8, device=dev)
    h = C.c_void_p()
    _lib.check(lib.ucfp_text_streams_create_sim(ctx.handle, S, T.STREAMS_UTF8 if utf8 else 0, S * chunk if utf8 else 0, th,
                                                C.byref(h)))
    assert lib.ucfp_text_streams_record_bytes(h) == 8

    def offline(blob, offs, n, out, status):
        if table is None:
            _lib.check(lib.ucfp_text_simhash_batch_dev(ctx.handle, blob.data_ptr(), offs.data_ptr(), n, mode, out.data_ptr(),
                                                       status.data_ptr(), st))
        else:
            _lib.check(lib.ucfp_text_simhash_idf_batch_dev(ctx.handle, th, blob.data_ptr(), offs.data_ptr(), n, mode, T.TOK_WORD,
                                                           out.data_ptr(), status.data_ptr(), st))

    def run_streams():
        slots = np.zeros(S, np.uint32)
        for i in range(S):
            s = C.c_uint32(0)
            _lib.check(lib.ucfp_text_streams_open(h, mode, C.byref(s)))
            slots[i] = s.value
        none, last = np.zeros(S, np.uint8), np.ones(S, np.uint8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for p in range(P):
            _lib.check(lib.ucfp_text_streams_push_dev(h, slots.ctypes.data, n_bytes.ctypes.data,
                                                      (last if p == P - 1 else none).ctypes.data, S, rows[p * S].data_ptr(),
                                                      d_out.data_ptr(), d_status.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        assert int(d_status.abs().sum().item()) == 0
        return e0.elapsed_time(e1)

    # the records first: entry i of every push is the stream that carried rows i, S + i, 2 S + i, ...
    pad = torch.zeros(64, dtype=torch.uint8, device=dev)
    whole = torch.cat([rows.view(P, S, chunk).permute(1, 0, 2).reshape(-1), pad])
    woffs = (torch.arange(S + 1, dtype=torch.int64, device=dev) * (P * chunk)).contiguous()
    wout = torch.zeros((S, 8), dtype=torch.uint8, device=dev)
    wst = torch.zeros(S, dtype=torch.int32, device=dev)
    offline(whole, woffs, S, wout, wst)
    run_streams()
    assert int(wst.abs().sum().item()) == 0 and torch.equal(d_out, wout), \
        "stream records differ from the offline records of the concatenated documents"
    del whole
    ms = min(run_streams() for _ in range(a.repeats))
    lib.ucfp_text_streams_destroy(h)

    flat = torch.cat([rows.reshape(-1), pad])
    offs = (torch.arange(S * P + 1, dtype=torch.int64, device=dev) * chunk).contiguous()
    bout = torch.empty((S * P, 8), dtype=torch.uint8, device=dev)
    bst = torch.empty(S * P, dtype=torch.int32, device=dev)

    def run_offline():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        offline(flat, offs, S * P, bout, bst)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    run_offline()
    bms = min(run_offline() for _ in range(a.repeats))
    total = S * P * chunk
    return {"state_bytes": int(lib.ucfp_text_streams_state_bytes_sim(T.STREAMS_UTF8 if utf8 else 0, 1 if table is not None else 0)),
            "records_equal_offline": True, "table_keys": len(table) if table is not None else 0,
            "stream_ms": round(ms, 3), "ms_per_push": round(ms / P, 4), "stream_GBs": round(total / (ms / 1e3) / 1e9, 3),
            "offline_ms": round(bms, 3), "offline_GBs": round(total / (bms / 1e3) / 1e9, 3),
            "stream_over_offline_rate": round(bms / ms, 3)}


def simhash_legs(a, ctx, lib, dev, st, ascii_rows):
    """TF and weighted legs over ASCII prose (the MinHash leg's own documents) and the two UTF-8 corpora, each weighted by a
    table fitted to the leg's own documents, and a weighted ASCII leg over a 200 k-word Zipf-like vocabulary (the corpus of
    tools/bench_simhash_idf.py --vocab 200000), whose table the tokens really probe."""
    import bench_text_utf8 as gen
    from ucfp_amd import text as T
    S, P, chunk = a.streams, a.pushes, a.chunk
    pick = (torch.arange(S * P, device=dev) * 7 + 3) % a.pool

    def pooled(docs):
        assert all(len(d) == chunk for d in docs)
        d_pool = torch.from_numpy(np.frombuffer(b"".join(docs), np.uint8).reshape(len(docs), chunk).copy()).to(dev)
        return d_pool[pick].contiguous()

    def fitted(rows, mode):
        t = T.IdfTable(ctx=ctx)
        flat = torch.cat([rows.reshape(-1), torch.zeros(64, dtype=torch.uint8, device=dev)])
        offs = (torch.arange(S * P + 1, dtype=torch.int64, device=dev) * chunk).contiguous()
        _lib.check(lib.ucfp_idf_table_add_batch_dev(t.handle, flat.data_ptr(), offs.data_ptr(), S * P, mode, T.TOK_WORD, None, st))
        _lib.check(lib.ucfp_idf_table_finalize(t.handle, st))
        return t

    out = {}
    corpora = [("ascii", T.RAW_ASCII, lambda: ascii_rows)]
    if not a.no_utf8:
        for kind, make in (("latin", gen.doc_latin), ("cjk", gen.doc_cjk)):
            rng = random.Random(0xC0DE + len(kind))
            corpora.append((kind, T.RAW_UTF8, lambda make=make, rng=rng: pooled(
                [make(rng, chunk).encode("utf-8").ljust(chunk, b" ") for _ in range(a.pool)])))
    nrng = np.random.default_rng(13)

    def zipf_doc():
        ranks = np.floor(200_000 ** nrng.random(chunk // 2)).astype(np.int64)
        return " ".join(f"w{r}" for r in ranks)[:chunk].rsplit(" ", 1)[0].ljust(chunk).encode("ascii")

    corpora.append(("zipf200k", T.RAW_ASCII, lambda: pooled([zipf_doc() for _ in range(a.pool)])))
    for name, mode, make in corpora:
        rows = make()
        table = fitted(rows, mode)
        if name != "zipf200k":
            out[f"{name}_tf"] = simhash_leg(a, ctx, lib, st, rows, mode, None)
        out[f"{name}_idf"] = simhash_leg(a, ctx, lib, st, rows, mode, table)
        table.close()
        del rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--pushes", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-utf8", action="store_true")
    ap.add_argument("--no-simhash", action="store_true", help="skip the SimHash stream legs (DESIGN.md T11)")
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
    simhash = {} if a.no_simhash else simhash_legs(a, ctx, lib, dev, st, blob)
    del blob
    utf8 = {} if a.no_utf8 else {kind: utf8_leg(kind, a, ctx, lib, dev, st, bms / ms) for kind in ("latin", "cjk")}
    print(json.dumps({"case": "text_streams_push", "streams": S, "pushes": P, "chunk_bytes": chunk,
                      "state_bytes": int(lib.ucfp_text_streams_state_bytes()), "repeats": a.repeats,
                      "stream_ms": round(ms, 3), "stream_GBs": round(total / (ms / 1e3) / 1e9, 3),
                      "pushes_per_s": round(P / (ms / 1e3), 1), "stream_pushes_per_s": round(S * P / (ms / 1e3), 1),
                      "offline_ms": round(bms, 3), "offline_GBs": round(total / (bms / 1e3) / 1e9, 3),
                      "offline_docs_per_s": round(S * P / (bms / 1e3), 1),
                      "stream_over_offline_rate": round(bms / ms, 3), "utf8": utf8, "simhash": simhash}), flush=True)


if __name__ == "__main__":
    main()
