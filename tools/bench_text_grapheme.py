"""The grapheme tokeniser and the caller-segmented token entries against the word tokeniser over the same bytes.

    python tools/bench_text_grapheme.py [--docs 100000] [--bytes 4096] [--distinct 2048] [--reps 7] [--only CORPUS] [--no-k1]

Three corpora of --bytes-sized documents resident in HBM (the generators of tools/bench_text_utf8.py; --distinct documents
from a seed, tiled to --docs):
    ascii   English-like prose, mode RAW_ASCII
    latin   prose with diacritics, mode RAW_UTF8
    cjk     Han and kana, mode RAW_UTF8
For each, one JSON line per measurement, all in the same run: the WORD tokeniser (the control: ucfp_text_*_batch_dev, the
entry that existed before), the GRAPHEME tokeniser (ucfp_text_*_batch_ex_dev) and the TOKEN form over the same clusters
(ucfp_text_*_tokens_batch_dev: the canonical bytes with one table entry per cluster), MinHash (k = 5, and k = 1 on the
ascii corpus: as many hashes as SimHash, with the 128-slot fold) and SimHash.  Times are device events around one call,
median of --reps after a warm-up; documents/s, shingles/s (MinHash: max(tokens - k + 1, 1) per document; SimHash: tokens)
and GB/s of source bytes.  The grapheme and token records are compared.  --only restricts the run to one corpus and --no-k1
leaves the k = 1 lines out, so that in a profiler's per-kernel statistics every kernel name is one measurement.
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_text_utf8 import doc_ascii, doc_cjk, doc_latin  # noqa: E402


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
    ap.add_argument("--only", default="", help="one corpus: ascii, latin or cjk")
    ap.add_argument("--no-k1", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no number"
    from ucfp_amd import _lib, text
    lib, ctx = _lib.load(), _lib.current_context()
    stream = torch.cuda.current_stream().cuda_stream or None
    rng = random.Random(a.seed)
    canon = text.Canonicalizer()
    n = a.docs

    for name, fn, mode in (("ascii", doc_ascii, text.RAW_ASCII), ("latin", doc_latin, text.RAW_UTF8), ("cjk", doc_cjk, text.RAW_UTF8)):
        if a.only and a.only != name:
            continue
        distinct = [fn(rng, a.bytes) for _ in range(min(a.distinct, n))]
        pick = np.arange(n) % len(distinct)

        def resident(docs):
            lens = np.array([len(d) for d in docs], np.int64)[pick]
            offs = np.zeros(n + 1, np.int64)
            np.cumsum(lens, out=offs[1:])
            blob = np.frombuffer(b"".join(docs), np.uint8)
            d_small = torch.from_numpy(blob.copy()).cuda()
            tiles = (n + len(docs) - 1) // len(docs)       # document i is distinct document i mod len(docs): the blob, repeated
            d_blob = torch.cat([d_small.repeat(tiles)[:int(offs[n])], torch.zeros(64, dtype=torch.uint8, device="cuda")])
            return d_blob, torch.from_numpy(offs).cuda(), int(offs[n])

        src = [t.encode("utf-8") for t in distinct]
        assert not any(b"\r" in d for d in src)
        d_blob, d_offs, src_bytes = resident(src)
        # the token form: the canonical bytes, one table entry per cluster (no CR in the corpora: a cluster = a code point)
        can = [canon.apply(t).encode("utf-8") for t in distinct]
        d_can, d_can_offs, _ = resident(can)
        lead = (d_can[:-64] & 0xC0) != 0x80
        d_tok = torch.cat([torch.nonzero(lead).flatten(), d_can_offs[-1:]]).contiguous()
        d_doc_tok = torch.searchsorted(d_tok, d_can_offs).contiguous()
        clusters = (d_doc_tok[1:] - d_doc_tok[:-1]).cpu().numpy()
        words = np.array([len(text._host_tokens(c.decode("utf-8"))) for c in can], np.int64)[pick]
        del lead
        d_rec = {"minhash": torch.zeros((n, 1032), dtype=torch.uint8, device="cuda"), "simhash": torch.zeros((n, 8), dtype=torch.uint8, device="cuda")}
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        keep = {}

        def measure(route, kind, k):
            out = d_rec[kind]
            if route == "word":
                if kind == "minhash":
                    call = lambda: lib.ucfp_text_minhash_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, k, out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
                else:
                    call = lambda: lib.ucfp_text_simhash_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
            elif route == "grapheme":
                if kind == "minhash":
                    call = lambda: lib.ucfp_text_minhash_batch_ex_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, text.TOK_GRAPHEME, k, out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
                else:
                    call = lambda: lib.ucfp_text_simhash_batch_ex_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, text.TOK_GRAPHEME, out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
            else:
                if kind == "minhash":
                    call = lambda: lib.ucfp_text_minhash_tokens_batch_dev(ctx.handle, d_can.data_ptr(), d_tok.data_ptr(), d_doc_tok.data_ptr(), n, k, out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
                else:
                    call = lambda: lib.ucfp_text_simhash_tokens_batch_dev(ctx.handle, d_can.data_ptr(), d_tok.data_ptr(), d_doc_tok.data_ptr(), n, out.data_ptr(), d_st.data_ptr(), stream)  # noqa: E731,E501
            assert call() == 0, lib.ucfp_last_error()
            sec, spread = timed(torch, call, a.reps)
            toks = words if route == "word" else clusters
            items = int(toks.sum()) if kind == "simhash" else int(np.maximum(toks - k + 1, 1).sum())
            row = {"corpus": name, "route": route, "kind": kind, "k": k if kind == "minhash" else None, "docs": n,
                   "mean_bytes": round(src_bytes / n, 1), "tokens_per_doc": round(float(toks.mean()), 1), "ms": round(sec * 1e3, 3),
                   "spread": round(spread, 3), "docs_per_s": round(n / sec), "shingles_per_s": round(items / sec),
                   "gb_per_s": round(src_bytes / sec / 1e9, 2), "status_nonzero": int((d_st != 0).sum().item())}
            if route != "word":
                mine = out[:len(distinct)].cpu().numpy().copy()
                other = keep.get((kind, k))
                if other is not None:
                    row["equals_other_cluster_route"] = bool(np.array_equal(mine, other))
                keep[(kind, k)] = mine
            print(json.dumps(row), flush=True)

        for route in ("word", "grapheme", "tokens"):
            measure(route, "minhash", 5)
            measure(route, "simhash", 0)
            if name == "ascii" and route != "word" and not a.no_k1:
                measure(route, "minhash", 1)
        if not a.only:
            measure("word", "minhash", 5)        # the control again, at the end of the corpus: the run's own spread
        del d_blob, d_can, d_tok, d_doc_tok
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
