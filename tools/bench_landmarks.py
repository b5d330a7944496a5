"""Landmark index at corpus scale: postings, rebuild time, queries/s for batches of 5-second clips, the
posting bytes gathered per query, and a single-threaded CPU hash-map restatement of the spec on a sample, checked
against the GPU answers.  Prints one JSON line per measurement.

    python tools/bench_landmarks.py [--tracks 10000] [--seconds 180]

The corpus is synthetic (notes of 300 .. 1000 samples, three random tones each, at 8 kHz): its hash distribution is
not music's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucfp_amd import _lib, audio  # noqa: E402
from ucfp_amd.index import LandmarkIndex  # noqa: E402

SR, HOP = 8000, 128


def synth(seeds, n, dev):
    """Tracks on the device: one row per seed."""
    g = torch.Generator(device=dev)
    out = torch.empty((len(seeds), n), dtype=torch.float32, device=dev)
    for r, s in enumerate(seeds):
        g.manual_seed(int(s))
        lens = torch.randint(300, 1001, (n // 300 + 1,), generator=g, device=dev)
        idx = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens)[:n]
        f = (150.0 + 3350.0 * torch.rand((3, lens.numel()), generator=g, device=dev))[:, idx].double()
        a = (0.1 + 0.2 * torch.rand((3, lens.numel()), generator=g, device=dev))[:, idx]
        ph = torch.remainder(torch.cumsum(f, 1) / SR, 1.0).float()
        out[r] = (a * torch.sin(2 * np.pi * ph)).sum(0) + 0.01 * torch.randn(n, generator=g, device=dev)
    return out


def fingerprint(pcm, ctx, stream):
    """pcm [m, n] device tracks -> list of uint32 [h, 2] arrays (one ragged batch launch)."""
    m, n = pcm.shape
    offs = torch.arange(m + 1, dtype=torch.int64, device=pcm.device) * n
    cap = int(_lib.load().ucfp_audio_wang_batch_max_hashes(m * n, m, SR, None))
    out = torch.empty((cap, 2), dtype=torch.int32, device=pcm.device)
    oo = torch.empty(m + 1, dtype=torch.int64, device=pcm.device)
    audio.wang_hashes_batch_dev(pcm.data_ptr(), offs.data_ptr(), m * n, m, SR, out.data_ptr(), cap, oo.data_ptr(),
                                stream=stream, ctx=ctx)
    o = oo.cpu().numpy()
    h = out[: int(o[-1])].cpu().numpy().view(np.uint32)
    return [h[o[i]:o[i + 1]] for i in range(m)]


def cpu_query(table, q, k):
    """The spec with a hash map (dict: hash -> list of (record, t)), one thread."""
    qs = {(int(h), int(t)) for h, t in q}
    cnt = {}
    for h, t in qs:
        for r, tr in table.get(h, ()):
            key = (r, tr - t)
            cnt[key] = cnt.get(key, 0) + 1
    best = {}
    for (r, d), c in cnt.items():
        b = best.get(r)
        if b is None or c > b[0] or (c == b[0] and d < b[1]):
            best[r] = (c, d)
    hits = sorted(((-c, r, d) for r, (c, d) in best.items()))[:k]
    return [(r, -c, d) for c, r, d in hits]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10000)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--chunk", type=int, default=250)
    ap.add_argument("--cpu-sample", type=int, default=16)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = "cuda:0"
    ctx = _lib.default_context(0)
    stream = torch.cuda.current_stream().cuda_stream
    n = a.seconds * SR
    ix = LandmarkIndex(0, ctx=ctx)
    fp_s, total_h, cpu_table = 0.0, 0, {}
    sample_tracks = set(range(0, a.tracks, max(1, a.tracks // 200)))
    for c0 in range(0, a.tracks, a.chunk):
        seeds = list(range(c0, min(a.tracks, c0 + a.chunk)))
        pcm = synth(seeds, n, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fps = fingerprint(pcm, ctx, stream)
        fp_s += time.perf_counter() - t0
        del pcm
        total_h += sum(f.shape[0] for f in fps)
        ix.upsert(0, np.array(seeds, np.uint64), fps)
        for s, f in zip(seeds, fps):
            if s in sample_tracks:
                for h, t in {(int(h), int(t)) for h, t in f}:
                    cpu_table.setdefault(h, []).append((s, t))
    t0 = time.perf_counter()
    ix.flush()
    rebuild_s = time.perf_counter() - t0
    recs, postings = ix.size(0)
    print(json.dumps({"bench": "landmark_corpus", "tracks": a.tracks, "seconds_per_track": a.seconds,
                      "audio_hours": a.tracks * a.seconds / 3600, "wang_fingerprint_s": round(fp_s, 3),
                      "landmarks": total_h, "records": recs, "postings": postings,
                      "posting_bytes": postings * 12, "rebuild_s": round(rebuild_s, 3)}), flush=True)
    # queries: 5-second clips at hop-aligned offsets, fingerprinted on the device
    rng = np.random.default_rng(1)
    nclip = 1024
    src = rng.integers(0, a.tracks, nclip)
    m = rng.integers(0, (n - 5 * SR) // HOP, nclip)
    clips = []
    for c0 in range(0, nclip, 256):
        pcm = synth(src[c0:c0 + 256].tolist(), n, dev)
        cut = torch.stack([pcm[i, HOP * int(m[c0 + i]): HOP * int(m[c0 + i]) + 5 * SR] for i in range(pcm.shape[0])])
        clips += fingerprint(cut.contiguous(), ctx, stream)
        del pcm
    for nq in (1, 64, 1024):
        qs = clips[:nq]
        ix.query(0, qs, 10)                      # warm
        reps = max(3, 256 // nq)
        t0 = time.perf_counter()
        for _ in range(reps):
            got = ix.query(0, qs, 10)
        dt = (time.perf_counter() - t0) / reps
        ok = float(np.mean([(int(got[0][i, 0]) == src[i]) and (int(got[2][i, 0]) == m[i]) for i in range(nq)]))
        # gathered posting bytes: 12 B (hash + entry) per vote, over the query's unique landmarks
        qlm = sum(len({(int(h), int(t)) for h, t in q}) for q in qs)
        print(json.dumps({"bench": "landmark_query", "batch": nq, "ms_per_batch": round(dt * 1e3, 3),
                          "queries_per_s": round(nq / dt, 1), "query_landmarks": qlm, "top1_correct": ok}), flush=True)
    # CPU baseline on the sampled tracks: the same spec over a sub-corpus, one thread, checked against a GPU index of it
    sub = LandmarkIndex(0, ctx=ctx)
    sample = sorted(sample_tracks)
    qi = [i for i in range(nclip) if src[i] in sample_tracks][: a.cpu_sample] or list(range(a.cpu_sample))
    per = {}
    for h, lst in cpu_table.items():
        for r, t in lst:
            per.setdefault(r, []).append((h, t))
    sub.upsert(0, np.array(sample, np.uint64), [np.array(per.get(r, []), np.uint32).reshape(-1, 2) for r in sample])
    t0 = time.perf_counter()
    cpu = [cpu_query(cpu_table, clips[i], 10) for i in qi]
    cpu_s = (time.perf_counter() - t0) / len(qi)
    g = sub.query(0, [clips[i] for i in qi], 10)
    agree = all([(int(g[0][j, x]), int(g[1][j, x]), int(g[2][j, x])) for x in range(int(g[4][j]))] == cpu[j]
                for j in range(len(qi)))
    print(json.dumps({"bench": "landmark_cpu_baseline", "threads": 1, "sub_corpus_tracks": len(sample),
                      "queries": len(qi), "cpu_ms_per_query": round(cpu_s * 1e3, 3), "gpu_agrees": bool(agree)}),
          flush=True)
    sub.close()
    ix.close()


if __name__ == "__main__":
    main()
