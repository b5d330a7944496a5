"""TF.IDF SimHash against TF SimHash over the same bytes, and the fit of the table.

    python tools/bench_simhash_idf.py [--docs 100000] [--bytes 4096] [--distinct 2048] [--reps 7] [--piece-tokens 0] [--pad-keys 0] [--vocab 0]

One corpus of --bytes-sized English-like ASCII documents resident in HBM (the generator of tools/bench_text_utf8.py;
--distinct documents from a seed, tiled to --docs), mode RAW_ASCII, the word tokeniser.  Three measurements in one run,
one JSON line each:
    tf        ucfp_text_simhash_batch_dev: the control
    idf       ucfp_text_simhash_idf_batch_dev against the table fitted below (one table gather per token)
    fit       ucfp_idf_table_add_batch_dev + ucfp_idf_table_finalize into a fresh table: documents/s, distinct keys
and a last line with the idf / tf ratio and the table's size.  The generator's vocabulary is small, so the fitted table is
too: --pad-keys K adds a line `idf_padded`, the same documents against the fitted weights plus K random keys that no
token has (a table of the size a real corpus makes; the records are the same and are compared).  --vocab V replaces the
prose by documents over V words `w<rank>` with log-uniform ranks (Zipf-like, exponent 1): a vocabulary whose tail the
tokens really look up.  The two record kernels are timed with device events around
one call, median of --reps after a warm-up; the fit synchronises the stream itself (it reads counters back per piece), so
it is timed on the host around the call and the synchronisation that follows it.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_text_utf8 import doc_ascii  # noqa: E402


def timed(torch, call, reps):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e-3, (max(ms) - min(ms)) / statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=13)
    ap.add_argument("--piece-tokens", type=int, default=0)
    ap.add_argument("--pad-keys", type=int, default=0)
    ap.add_argument("--vocab", type=int, default=0)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no number"
    from ucfp_amd import _lib, text
    lib, ctx = _lib.load(), _lib.current_context()
    stream = torch.cuda.current_stream().cuda_stream or None
    rng = random.Random(a.seed)
    n = a.docs
    if a.vocab:
        nrng = np.random.default_rng(a.seed)

        def doc_vocab():
            ranks = np.floor(a.vocab ** nrng.random(a.bytes // 2)).astype(np.int64)
            return " ".join(f"w{r}" for r in ranks)[:a.bytes].rsplit(" ", 1)[0].ljust(a.bytes).encode("ascii")
        distinct = [doc_vocab() for _ in range(min(a.distinct, n))]
    else:
        distinct = [doc_ascii(rng, a.bytes).encode("ascii") for _ in range(min(a.distinct, n))]
    pick = np.arange(n) % len(distinct)
    lens = np.array([len(d) for d in distinct], np.int64)[pick]
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    d_small = torch.from_numpy(np.frombuffer(b"".join(distinct), np.uint8).copy()).cuda()
    tiles = (n + len(distinct) - 1) // len(distinct)
    d_blob = torch.cat([d_small.repeat(tiles)[:int(offs[n])], torch.zeros(64, dtype=torch.uint8, device="cuda")])
    d_offs = torch.from_numpy(offs).cuda()
    src_bytes = int(offs[n])
    tokens = int(np.array([len(text._host_tokens(d.decode().lower())) for d in distinct], np.int64)[pick].sum())
    d_out = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    mode, tok = text.RAW_ASCII, text.TOK_WORD

    def row(what, sec, spread, **more):
        r = {"what": what, "docs": n, "mean_bytes": round(src_bytes / n, 1), "tokens_per_doc": round(tokens / n, 1),
             "ms": round(sec * 1e3, 3), "spread": round(spread, 3), "docs_per_s": round(n / sec), "tokens_per_s": round(tokens / sec),
             "gb_per_s": round(src_bytes / sec / 1e9, 2), "vocab": a.vocab or "prose"}
        r.update(more)
        print(json.dumps(r), flush=True)
        return r

    def fit_once():
        t = text.IdfTable(ctx=ctx, piece_tokens=a.piece_tokens)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.ucfp_idf_table_add_batch_dev(t.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, tok, d_st.data_ptr(), stream))
        _lib.check(lib.ucfp_idf_table_finalize(t.handle, stream))
        torch.cuda.synchronize()
        return t, time.perf_counter() - t0

    fit_once()[0].close()                                  # warm-up: scratch sizes, rocPRIM's first launch
    fits = [fit_once() for _ in range(max(3, a.reps // 2))]
    secs = [s for _, s in fits]
    table = fits[0][0]
    for t, _ in fits[1:]:
        t.close()
    assert int((d_st != 0).sum().item()) == 0
    n_keys = len(table)

    tf_call = lambda: lib.ucfp_text_simhash_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, d_out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
    idf_call = lambda: lib.ucfp_text_simhash_idf_batch_dev(ctx.handle, table.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, tok, d_out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
    assert tf_call() == 0 and idf_call() == 0, lib.ucfp_last_error()
    tf = row("tf", *timed(torch, tf_call, a.reps))
    idf = row("idf", *timed(torch, idf_call, a.reps), status_nonzero=int((d_st != 0).sum().item()))
    tf2 = row("tf", *timed(torch, tf_call, a.reps))        # the control again: the run's own spread
    row("fit", statistics.median(secs), (max(secs) - min(secs)) / statistics.median(secs), distinct_keys=n_keys, n_docs=table.n_docs,
        piece_tokens=a.piece_tokens or 1 << 22)
    if a.pad_keys:
        e = table.export()
        assert idf_call() == 0, lib.ucfp_last_error()
        torch.cuda.synchronize()
        ref_out = d_out.clone()
        extra = np.random.default_rng(a.seed).integers(1, 1 << 63, a.pad_keys, dtype=np.uint64) | np.uint64(1 << 63)
        extra = np.setdiff1d(extra, e["keys"])
        e["keys"] = np.concatenate([e["keys"], extra])
        e["weights"] = np.concatenate([e["weights"], np.full(extra.size, 0x10000, np.uint32)])
        big = text.IdfTable.load(e, ctx=ctx)
        big_call = lambda: lib.ucfp_text_simhash_idf_batch_dev(ctx.handle, big.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, tok, d_out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
        assert big_call() == 0, lib.ucfp_last_error()
        pslots = 16
        while pslots < 2 * len(big):
            pslots *= 2
        row("idf_padded", *timed(torch, big_call, a.reps), table_keys=len(big), table_slots=pslots, table_bytes=(pslots + 1) * 16,
            equals_idf=bool(torch.equal(ref_out, d_out)))
        big.close()
    slots = 1 << 17                                        # IdfTable's default capacity_hint of 2^16 keys, at most half full
    while slots < 2 * n_keys:
        slots *= 2
    print(json.dumps({"what": "summary", "idf_over_tf": round(idf["docs_per_s"] / max(tf["docs_per_s"], tf2["docs_per_s"]), 3),
                      "distinct_keys": n_keys, "table_slots": slots, "table_bytes": (slots + 1) * 16}), flush=True)
    table.close()


if __name__ == "__main__":
    main()
