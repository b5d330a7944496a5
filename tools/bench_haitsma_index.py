"""Haitsma sub-fingerprint index at corpus scale: frames, rebuild time, queries/s for batches of
256-frame excerpts (clean and with noise) at every flip_bits, the seeds / candidates / candidate bytes per query (so
that the verify kernels' GB/s can be read off a kernel trace), and a single-threaded numpy restatement of the spec over
a sub-corpus, checked against the GPU answers.  Prints one JSON line per measurement.

    python tools/bench_haitsma_index.py [--tracks 10000] [--seconds 180]

Every clean excerpt's first hit must be its source track at its offset: the tool exits with an error otherwise.
The corpus is synthetic (four random tones per 0.25 s over a noise floor, at 5 kHz): its value distribution is not
music's."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucfp_amd import _lib, audio  # noqa: E402
from ucfp_amd.index import HaitsmaIndex  # noqa: E402

SR, HOP, WIN = 5000, 64, 2048
M = 256                                  # frames per excerpt
CLIP = WIN + HOP * (M - 1)
SEG = SR // 4


def synth(seeds, n, dev):
    """Tracks on the device, one row per seed: per 0.25-s segment four tones (200 .. 2200 Hz, amplitude 0.2 .. 1) over
    a noise floor, scaled to a peak of 0.8."""
    g = torch.Generator(device=dev)
    nseg = (n + SEG - 1) // SEG
    t = torch.arange(n, device=dev, dtype=torch.float64) / SR      # f64: the phase of 2200 Hz after minutes
    seg = (torch.arange(n, device=dev) // SEG)
    out = torch.empty((len(seeds), n), dtype=torch.float32, device=dev)
    for r, s in enumerate(seeds):
        g.manual_seed(int(s))
        f = 200.0 + 2000.0 * torch.rand((4, nseg), generator=g, device=dev)
        a = 0.2 + 0.8 * torch.rand((4, nseg), generator=g, device=dev)
        ph = 6.28 * torch.rand((4, nseg), generator=g, device=dev)
        x = (a[:, seg] * torch.sin(2 * np.pi * torch.remainder(f.double()[:, seg] * t, 1.0).float() + ph[:, seg])).sum(0)
        x = x + 0.05 * torch.randn(n, generator=g, device=dev)
        out[r] = x * (0.8 / x.abs().max())
    return out


def fingerprint_dev(pcm, ctx, stream):
    """pcm [m, n] device clips -> (device frames i32 [total], device offsets i64 [m + 1]): one ragged batch launch."""
    lib = _lib.load()
    m, n = pcm.shape
    offs = torch.arange(m + 1, dtype=torch.int64, device=pcm.device) * n
    cap = max(1, int(lib.ucfp_audio_haitsma_batch_max_frames(m * n, m, SR)))
    out = torch.empty(cap, dtype=torch.int32, device=pcm.device)
    oo = torch.empty(m + 1, dtype=torch.int64, device=pcm.device)
    cfg = audio.HaitsmaConfig()._c()
    _lib.check(lib.ucfp_audio_haitsma_batch_dev(ctx.handle, pcm.data_ptr(), offs.data_ptr(), m * n, m, SR, C.byref(cfg),
                                                out.data_ptr(), cap, oo.data_ptr(), stream or None))
    return out, oo


POP16 = np.array([bin(i).count("1") for i in range(65536)], np.int64)


def masks(flip_bits):
    m = [0]
    if flip_bits >= 1:
        m += [1 << b for b in range(32)]
    if flip_bits >= 2:
        m += [(1 << a) | (1 << b) for a in range(32) for b in range(a + 1, 32)]
    return np.array(m, np.uint32)


class CpuIndex:
    """The spec in numpy, one thread: sorted values + positions, searchsorted, unique, popcount table."""

    def __init__(self, frames):
        self.len = np.array([f.size for f in frames], np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.len)]).astype(np.int64)
        self.flat = np.concatenate(frames)
        self.pos = np.argsort(self.flat, kind="stable")
        self.val = self.flat[self.pos]

    def candidates(self, q, flip_bits):
        """-> (seeds looked at, ordinals, offsets of the distinct admissible ones)."""
        mk = masks(flip_bits)
        pr = (q[:, None] ^ mk[None, :]).ravel()
        lo = np.searchsorted(self.val, pr, "left")
        ln = np.searchsorted(self.val, pr, "right") - lo
        tot = int(ln.sum())
        p = self.pos[np.repeat(lo - (np.cumsum(ln) - ln), ln) + np.arange(tot)]
        o = np.searchsorted(self.start, p, "right") - 1
        d = p - self.start[o] - np.repeat(np.repeat(np.arange(q.size), mk.size), ln)
        ok = (d >= 0) & (d + q.size <= self.len[o])
        key = np.unique((o[ok] << 32) | d[ok])
        return tot, key >> 32, key & 0xFFFFFFFF

    def query(self, q, k, flip_bits, ppm):
        _, o, d = self.candidates(q, flip_bits)
        if not o.size:
            return []
        x = self.flat[(self.start[o] + d)[:, None] + np.arange(q.size)[None, :]] ^ q[None, :]
        dist = (POP16[x & np.uint32(0xFFFF)] + POP16[x >> np.uint32(16)]).sum(1)
        best = np.lexsort((d, dist, o))
        o, d, dist = o[best], d[best], dist[best]
        first = np.ones(o.size, bool)
        first[1:] = o[1:] != o[:-1]
        o, d, dist = o[first], d[first], dist[first]
        keep = dist * 1_000_000 <= ppm * 32 * q.size
        o, d, dist = o[keep], d[keep], dist[keep]
        order = np.lexsort((o, dist))[:k]
        return [(int(o[i]), int(dist[i]), int(d[i])) for i in order]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=10000)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--chunk", type=int, default=250)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--snr", type=float, default=20.0)
    ap.add_argument("--stat-sample", type=int, default=16)
    ap.add_argument("--cpu-tracks", type=int, default=200)
    ap.add_argument("--cpu-sample", type=int, default=8)
    ap.add_argument("--reps", type=int, default=0, help="timed repetitions per case (0: 256 / batch, at least 3)")
    ap.add_argument("--flip-bits", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--sets", nargs="+", default=["clean", "noisy"], help="a kernel trace of ONE case: --sets noisy "
                    "--flip-bits 2 --batches 1024 --cpu-tracks 0")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = "cuda:0"
    ctx = _lib.default_context(0)
    stream = torch.cuda.current_stream().cuda_stream
    n = a.seconds * SR
    ix = HaitsmaIndex(0, ctx=ctx)
    fp_s, host_frames = 0.0, []
    for c0 in range(0, a.tracks, a.chunk):
        seeds = list(range(c0, min(a.tracks, c0 + a.chunk)))
        pcm = synth(seeds, n, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_fr, d_oo = fingerprint_dev(pcm, ctx, stream)
        torch.cuda.synchronize()
        fp_s += time.perf_counter() - t0
        del pcm
        d_ids = torch.tensor(seeds, dtype=torch.int64, device=dev)
        ix.upsert_dev(0, d_ids.data_ptr(), d_fr.data_ptr(), d_oo.data_ptr(), len(seeds), stream)   # device to index
        oo = d_oo.cpu().numpy()
        fr = d_fr[: int(oo[-1])].cpu().numpy().view(np.uint32)
        host_frames += [fr[oo[i]:oo[i + 1]].copy() for i in range(len(seeds))]
    t0 = time.perf_counter()
    ix.flush()
    rebuild_s = time.perf_counter() - t0
    recs, frames = ix.size(0)
    print(json.dumps({"bench": "haitsma_corpus", "tracks": a.tracks, "seconds_per_track": a.seconds,
                      "audio_hours": a.tracks * a.seconds / 3600, "haitsma_fingerprint_s": round(fp_s, 3), "records": recs,
                      "frames": frames, "frame_bytes": frames * 4, "posting_bytes": frames * 8,
                      "rebuild_s": round(rebuild_s, 3), "rebuild_s_per_million_postings": round(rebuild_s / max(frames, 1) * 1e6, 5)}),
          flush=True)
    # excerpts: 256 frames cut at an arbitrary sample, clean and with white noise, fingerprinted on the device
    rng = np.random.default_rng(1)
    src = rng.integers(0, a.tracks, a.queries)
    s0 = rng.integers(0, n - CLIP, a.queries)
    sets = {"clean": [], "noisy": []}
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    for c0 in range(0, a.queries, 256):
        pcm = synth(src[c0:c0 + 256].tolist(), n, dev)
        cut = torch.stack([pcm[i, int(s0[c0 + i]): int(s0[c0 + i]) + CLIP] for i in range(pcm.shape[0])]).contiguous()
        del pcm
        p = (cut.double() ** 2).mean(1, keepdim=True)
        noise = torch.randn(cut.shape, generator=g, device=dev, dtype=torch.float64) * torch.sqrt(p / 10 ** (a.snr / 10))
        for name, x in (("clean", cut), ("noisy", (cut.double() + noise).float().contiguous())):
            d_fr, d_oo = fingerprint_dev(x, ctx, stream)
            oo = d_oo.cpu().numpy()
            fr = d_fr[: int(oo[-1])].cpu().numpy().view(np.uint32)
            sets[name] += [fr[oo[i]:oo[i + 1]].copy() for i in range(x.shape[0])]
    assert all(q.size == M for qs in sets.values() for q in qs)
    cpu_full = CpuIndex(host_frames)        # for the seeds / candidates of a sample of queries
    bad = 0
    for name, qs_all in sets.items():
        if name not in a.sets:
            continue
        for flip_bits in a.flip_bits:
            stat = [cpu_full.candidates(q, flip_bits) for q in qs_all[: a.stat_sample]]
            seeds_q = float(np.mean([s[0] for s in stat]))
            cands_q = float(np.mean([s[1].size for s in stat]))
            for nq in a.batches:
                if nq > a.queries:
                    continue
                qs = qs_all[:nq]
                ix.query(0, qs, 10, flip_bits)           # warm
                reps = a.reps or max(3, 256 // nq)
                times = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    got = ix.query(0, qs, 10, flip_bits)
                    times.append(time.perf_counter() - t0)
                dt = float(np.median(times))
                ok = [int(got[4][i]) >= 1 and int(got[0][i, 0]) == src[i] and abs(int(got[2][i, 0]) - s0[i] / HOP) <= 1
                      for i in range(nq)]
                if name == "clean":
                    bad += nq - sum(ok)
                print(json.dumps({"bench": "haitsma_query", "excerpts": name, "snr_db": None if name == "clean" else a.snr,
                                  "flip_bits": flip_bits, "batch": nq, "reps": reps, "ms_per_batch": round(dt * 1e3, 3),
                                  "ms_min": round(min(times) * 1e3, 3), "ms_max": round(max(times) * 1e3, 3),
                                  "queries_per_s": round(nq / dt, 1), "top1_correct": float(np.mean(ok)),
                                  "seeds_per_query": round(seeds_q, 1), "candidates_per_query": round(cands_q, 1),
                                  "candidate_bytes_per_query": round(cands_q * M * 4, 1)}), flush=True)
    del cpu_full
    # CPU baseline: the same spec over a sub-corpus, one thread, checked against a GPU index of it
    if not a.cpu_tracks:
        ix.close()
        if bad:
            sys.exit(f"{bad} clean excerpts were not identified at their offset")
        return
    sample = list(range(0, a.tracks, max(1, a.tracks // a.cpu_tracks)))[: a.cpu_tracks]
    sub = HaitsmaIndex(0, ctx=ctx)
    sub.upsert(0, np.array(sample, np.uint64), [host_frames[i] for i in sample])
    cpu = CpuIndex([host_frames[i] for i in sample])
    in_sample = set(sample)
    qi = ([i for i in range(a.queries) if int(src[i]) in in_sample] + list(range(a.queries)))[: a.cpu_sample]
    for flip_bits in a.flip_bits:
        qs = [sets["noisy"][i] for i in qi]
        t0 = time.perf_counter()
        want = [cpu.query(q, 10, flip_bits, 350_000) for q in qs]
        cpu_s = (time.perf_counter() - t0) / len(qs)
        gq = sub.query(0, qs, 10, flip_bits)
        agree = all([(int(gq[0][j, x]), int(gq[1][j, x]), int(gq[2][j, x])) for x in range(int(gq[4][j]))]
                    == [(sample[o], ds, d) for o, ds, d in want[j]] for j in range(len(qs)))
        bad += 0 if agree else 1
        print(json.dumps({"bench": "haitsma_cpu_baseline", "threads": 1, "sub_corpus_tracks": len(sample), "queries": len(qs),
                          "flip_bits": flip_bits, "cpu_ms_per_query": round(cpu_s * 1e3, 3), "gpu_agrees": bool(agree)}),
              flush=True)
    sub.close()
    ix.close()
    if bad:
        sys.exit(f"{bad} clean excerpts were not identified at their offset, or CPU / GPU disagreements")


if __name__ == "__main__":
    main()
