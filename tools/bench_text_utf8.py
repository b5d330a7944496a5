"""Text route on non-ASCII documents: mode RAW_UTF8 (canonicalise + tokenise on the GPU) against the host path it replaces.

    python tools/bench_text_utf8.py [--docs 4096] [--bytes 4096] [--host-docs 1024] [--reps 7]

Three corpora of --bytes-sized documents, generated from a seed:
    ascii   English-like words and punctuation (no `_`, no `'`: modes 0 and 2 give the same records, DESIGN U6)
    latin   prose with about 5 % two-byte code points, curly quotes and dashes
    cjk     Han and kana with full-width punctuation

Two kinds of figures, one JSON line each:
    "device"  the C ABI's _dev calls on documents resident on the GPU, timed with device events (median of --reps after a
              warm-up): mode 0 (ascii only), mode 2, and PRETOKENIZED over the host-made tokens (the hash pass alone)
    "python"  text.minhash_batch as a user calls it (host clock; the call ends in a synchronise) beside `host_path`, the
              minhash_batch of the commit before mode 2 existed: every non-ASCII document through `_prepare`
              (unicodedata + regex) in a Python loop, then one PRETOKENIZED launch.  Records are compared.
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

WORDS = ("the quick brown fox jumps over lazy dog and then a small river runs past old mill where nobody has been since "
         "winter of 1987 with 3.14 or 1,000 reasons e.g. U.S.A. x:y ab12cd HELLO World").split()
ACCENTED = "é è ê à ç ü ö ä ñ ó í ú ß ø å œ É Ü".split()
HAN = [chr(c) for c in range(0x4E00, 0x4E00 + 3000)]
HIRA = [chr(c) for c in range(0x3041, 0x3097)]
KATA = [chr(c) for c in range(0x30A1, 0x30FB)]


def _cut(s: str, nbytes: int) -> str:
    b = s.encode("utf-8")[:nbytes]
    return b.decode("utf-8", "ignore")


def doc_ascii(rng, nbytes):
    out, size = [], 0
    while size < nbytes:
        out.append(rng.choice(WORDS) + rng.choice([" ", " ", " ", ", ", ". ", "\n", "; ", " - "]))
        size += len(out[-1])
    return _cut("".join(out), nbytes)


def doc_latin(rng, nbytes):
    out, size = [], 0
    while size < nbytes:
        w = rng.choice(WORDS)
        if rng.random() < 0.22:                      # about one letter in twenty is a two-byte code point
            i = rng.randrange(len(w) + 1)
            w = w[:i] + rng.choice(ACCENTED) + w[i:]
        r = rng.random()
        if r < 0.03:
            w = "“" + w + "”"
        elif r < 0.06:
            w = w + "’s"
        elif r < 0.08:
            w = w + " —"
        out.append(w + rng.choice([" ", " ", " ", ", ", ". ", "\n"]))
        size += len(out[-1].encode("utf-8"))
    return _cut("".join(out), nbytes)


def doc_cjk(rng, nbytes):
    out, size = [], 0
    while size < nbytes:
        r = rng.random()
        if r < 0.55:
            w = "".join(rng.choice(HAN) for _ in range(rng.randint(1, 4)))
        elif r < 0.8:
            w = "".join(rng.choice(HIRA) for _ in range(rng.randint(1, 5)))
        elif r < 0.95:
            w = "".join(rng.choice(KATA) for _ in range(rng.randint(2, 6)))
        else:
            w = rng.choice(["。", "、", " ", "１２３", "ABC"])
        out.append(w)
        size += len(w.encode("utf-8"))
    return _cut("".join(out), nbytes)


def host_path(text, texts, k=5):
    """minhash_batch as it was before mode RAW_UTF8: `_prepare` every document, one launch per mode."""
    opts = text.TextOpts()
    prepared = [text._prepare(t, opts) for t in texts]
    out = np.zeros((len(texts), text.MINHASH_BYTES), np.uint8)
    status = np.zeros(len(texts), np.int32)
    for mode in (text.RAW_ASCII, text.PRETOKENIZED):
        idx = [i for i, (_, m) in enumerate(prepared) if m == mode]
        if idx:
            o, s = text._run("minhash", [prepared[i][0] for i in idx], mode, k)
            out[idx], status[idx] = o, s
    return out, status


def device_rate(torch, lib, ctx, docs, mode, reps):
    """documents/s of ucfp_text_minhash_batch_dev on device-resident documents (device events, median)."""
    n = len(docs)
    blob = np.frombuffer(b"".join(docs) + b"\0" * 64, np.uint8)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    d_blob, d_offs = torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(offs).cuda()
    d_rec = torch.zeros((n, 1032), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream or None

    def call():
        rc = lib.ucfp_text_minhash_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode, 5, d_rec.data_ptr(),
                                             d_st.data_ptr(), stream)
        assert rc == 0, lib.ucfp_last_error()
    for _ in range(3):
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
    return n / (statistics.median(ms) * 1e-3), int((d_st != 0).sum().item()), d_rec.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--bytes", type=int, default=4096)
    ap.add_argument("--host-docs", type=int, default=1024, help="documents of the python comparison (the host path is slow)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=13)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no number"
    from ucfp_amd import _lib, text
    lib, ctx = _lib.load(), _lib.current_context()
    rng = random.Random(a.seed)
    corpora = {name: [fn(rng, a.bytes) for _ in range(a.docs)]
               for name, fn in (("ascii", doc_ascii), ("latin", doc_latin), ("cjk", doc_cjk))}
    for name, texts in corpora.items():
        docs = [t.encode("utf-8") for t in texts]
        row = {"kind": "device", "corpus": name, "docs": len(docs), "mean_bytes": round(sum(map(len, docs)) / len(docs), 1),
               "two_plus_byte_share": round(sum(ord(c) >= 0x80 for t in texts[:64] for c in t) / sum(map(len, texts[:64])), 3)}
        r2, nz2, rec2 = device_rate(torch, lib, ctx, docs, text.RAW_UTF8, a.reps)
        row["mode2_docs_per_s"], row["mode2_status_nonzero"] = round(r2), nz2
        if name == "ascii":
            r0, nz0, rec0 = device_rate(torch, lib, ctx, docs, text.RAW_ASCII, a.reps)
            row["mode0_docs_per_s"], row["mode0_equals_mode2"] = round(r0), bool(np.array_equal(rec0, rec2))
        else:
            toks = [text._prepare(t, text.TextOpts())[0] for t in texts[:a.host_docs]]
            tiled = (toks * (len(docs) // len(toks) + 1))[:len(docs)]       # the same number of waves as the mode 2 launch
            r1, _, rec1 = device_rate(torch, lib, ctx, tiled, text.PRETOKENIZED, a.reps)
            row["hash_pass_alone_docs_per_s"] = round(r1)
            row["mode2_equals_host_tokens_hash"] = bool(np.array_equal(rec1[:len(toks)], rec2[:len(toks)]))
        print(json.dumps(row), flush=True)
    for name, texts in corpora.items():
        texts = texts[:a.host_docs]
        text.minhash_batch(texts[:8])
        t0 = time.perf_counter()
        new, new_st = text.minhash_batch(texts)
        t1 = time.perf_counter()
        old, old_st = host_path(text, texts)
        t2 = time.perf_counter()
        print(json.dumps({"kind": "python", "corpus": name, "docs": len(texts), "minhash_batch_docs_per_s": round(len(texts) / (t1 - t0)),
                          "host_path_docs_per_s": round(len(texts) / (t2 - t1)), "ratio": round((t2 - t1) / (t1 - t0), 1),
                          "records_equal": bool(np.array_equal(new, old) and np.array_equal(new_st, old_st))}), flush=True)


if __name__ == "__main__":
    main()
