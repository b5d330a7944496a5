"""Panako index with the (scale, offset) vote against A10's rigid-offset vote over the (hash, t_anchor)
projection of the same records (DESIGN A13 P7, the code path of the parent commit): queries/s at batch sizes 1, 64 and
1024 for unstretched 8 s excerpts through both, and for excerpts re-rendered at speeds 0.85 ... 1.2 through the new one,
with the share of queries whose expanded votes exceed ucfp_panako_index_lds_votes() (the global path), counted in numpy
over a sample.  A third set, `resampled`, is the same excerpts played at those speeds through a resampler (frequencies
multiplied by the speed) and answered with bins="scaled" (DESIGN A22, ucfp_panako_index_query_ex).  Prints one JSON
line per measurement.

    python tools/bench_panako_index.py [--tracks 500] [--seconds 60] [--sets unstretched stretched resampled]

Every unstretched excerpt's first hit must be its source track through both indexes, every stretched one through the new
index and every resampled one through its scaled mode: the tool exits with an error otherwise.  The corpus is synthetic (tone bursts at seeded onsets, the
generator of tests/panako_match_ref.py restated): its hash distribution is not music's."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ucfp_amd import _lib, audio  # noqa: E402
from ucfp_amd.index import PANAKO_MATCH_DEFAULTS, LandmarkIndex, PanakoIndex  # noqa: E402

SR = 8000
EXCERPT_S = 8.0
SPEEDS = (0.85, 0.9, 0.96, 1.03, 1.1, 1.2)


def make_score(seed, seconds, per_second=9.0):
    rng = np.random.default_rng(seed)
    n = int(seconds * per_second)
    return np.stack([np.sort(rng.uniform(0.0, seconds - 0.2, n)), rng.uniform(0.10, 0.16, n),
                     rng.integers(40, 440, n) * (SR / 1024.0), rng.uniform(0.08, 0.25, n)], axis=1)


def render(score, t0, t1, speed=1.0, pitch=1.0):
    """The excerpt [t0, t1) of the score at `speed`: onsets and durations divided by it, frequencies multiplied by `pitch`
    (1.0: a time stretch; `speed`: a resampled copy, whose tones past SR / 2 alias and are left in)."""
    n = int(round((t1 - t0) / speed * SR))
    x = np.zeros(n)
    for onset, dur, freq, amp in score[(score[:, 0] + score[:, 1] > t0) & (score[:, 0] < t1)] * np.array([1.0, 1.0, pitch, 1.0]):
        a, m = int(round((onset - t0) / speed * SR)), int(round(dur / speed * SR))
        lo, hi = max(a, 0), min(a + m, n)
        if hi > lo and m >= 2:
            i = np.arange(lo, hi) - a
            x[lo:hi] += amp * np.hanning(m)[i] * np.sin(2 * np.pi * freq * i / SR)
    return x.astype(np.float32)


def expanded_votes(h, a, d, q, lds_match):
    """Expanded votes of one query over the sorted postings (h, a, d): matches x supported hypotheses (A14)."""
    m = lds_match
    scales = np.arange(m["scale_min"], m["scale_max"] + 1, m["scale_step"], dtype=np.int64)
    t = np.unique(np.stack([q[:, 0], q[:, 1], q[:, 3] - q[:, 1]], axis=1).astype(np.int64), axis=0)
    total = 0
    for dr in range(-m["r_slack"], m["r_slack"] + 1):
        r = (t[:, 0] & 31) + dr
        hp = (t[:, 0] & ~np.int64(31)) | np.clip(r, 0, 31)
        lo = np.searchsorted(h, hp, "left")
        ln = np.where((r >= 0) & (r <= 31), np.searchsorted(h, hp, "right") - lo, 0)
        if not ln.sum():
            continue
        p = np.repeat(lo - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum()))
        dq = np.repeat(t[:, 2], ln)
        total += int((np.abs(256 * d[p][:, None] - scales[None, :] * dq[:, None]) <= 256 * m["slack"]).sum())
    return total


def timed(fn, reps):
    fn()                                     # warm
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=500)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--sets", nargs="+", default=["unstretched", "stretched", "resampled"],
                    choices=["unstretched", "stretched", "resampled"])
    ap.add_argument("--path-sample", type=int, default=128)
    ap.add_argument("--reps", type=int, default=0, help="timed repetitions per case (0: 256 / batch, at least 3)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    scores = [make_score(5000 + i, a.seconds) for i in range(a.tracks)]
    t0 = time.perf_counter()
    recs = []
    for c0 in range(0, a.tracks, 64):
        recs += audio.panako_hashes_batch([render(s, 0.0, a.seconds) for s in scores[c0:c0 + 64]], SR, ctx=ctx)
    fp_s = time.perf_counter() - t0
    ids = np.arange(a.tracks, dtype=np.uint64)
    new, old = PanakoIndex(0, ctx=ctx), LandmarkIndex(0, ctx=ctx)
    new.upsert(0, ids, recs)
    old.upsert(0, ids, [audio.panako_landmarks(r.tobytes()) for r in recs])
    t0 = time.perf_counter()
    new.flush()
    t_new = time.perf_counter() - t0
    t0 = time.perf_counter()
    old.flush()
    t_old = time.perf_counter() - t0
    print(json.dumps({"bench": "panako_corpus", "tracks": a.tracks, "seconds_per_track": a.seconds,
                      "synth_and_fingerprint_s": round(fp_s, 2), "triples": int(sum(r.shape[0] for r in recs)),
                      "a14_postings": new.size(0)[1], "a10_postings": old.size(0)[1], "a14_rebuild_s": round(t_new, 4),
                      "a10_rebuild_s": round(t_old, 4)}), flush=True)
    rng = np.random.default_rng(1)
    src = rng.integers(0, a.tracks, a.queries)
    start = rng.integers(0, int(a.seconds - EXCERPT_S - 1), a.queries).astype(float)
    speed = np.array(SPEEDS)[rng.integers(0, len(SPEEDS), a.queries)]
    sets = {}
    for name, sp, pitch in (("unstretched", np.ones(a.queries), np.ones(a.queries)), ("stretched", speed, np.ones(a.queries)),
                            ("resampled", speed, speed)):
        if name not in a.sets:
            continue
        qs = []
        for c0 in range(0, a.queries, 64):
            qs += audio.panako_hashes_batch([render(scores[src[i]], start[i], start[i] + EXCERPT_S, sp[i], pitch[i])
                                             for i in range(c0, min(a.queries, c0 + 64))], SR, ctx=ctx)
        sets[name] = qs
    # the share of queries on the global path, from a sample
    flat = np.concatenate(recs).astype(np.int64)
    flat = flat[np.argsort(flat[:, 0], kind="stable")]
    ph, pa, pd = flat[:, 0], flat[:, 1], flat[:, 3] - flat[:, 1]
    lds = PanakoIndex.lds_votes()
    bad = 0
    for name, qs_all in sets.items():
        if name == "resampled":                  # the kept-bins count says nothing about scaled mode: not sampled
            v_mean = share = None
        else:
            v = np.array([expanded_votes(ph, pa, pd, q, PANAKO_MATCH_DEFAULTS) for q in qs_all[: a.path_sample]])
            v_mean, share = round(float(v.mean()), 1), round(float((v > lds).mean()), 3)
        for nq in a.batches:
            if nq > a.queries:
                continue
            qs = qs_all[:nq]
            reps = a.reps or max(3, 256 // nq)
            legs = [("a14_scale_offset_vote", lambda: new.query(0, qs, 10))]
            if name == "resampled":
                legs = [("a22_scaled_bins_vote", lambda: new.query(0, qs, 10, bins="scaled"))]
            if name == "unstretched":
                lm = [audio.panako_landmarks(q.tobytes()) for q in qs]
                legs.append(("a10_projection_baseline", lambda: old.query(0, lm, 10)))
            for leg, fn in legs:
                got, dt, lo, hi = timed(fn, reps)
                ok = [int(got[-1][i]) >= 1 and int(got[0][i, 0]) == src[i] for i in range(nq)]
                bad += nq - sum(ok)
                print(json.dumps({"bench": "panako_query", "excerpts": name, "leg": leg, "batch": nq, "reps": reps,
                                  "ms_per_batch": round(dt * 1e3, 3), "ms_min": round(lo * 1e3, 3), "ms_max": round(hi * 1e3, 3),
                                  "queries_per_s": round(nq / dt, 1), "top1_correct": float(np.mean(ok)),
                                  "triples_per_query": round(float(np.mean([q.shape[0] for q in qs])), 1),
                                  "expanded_votes_per_query_sampled": v_mean, "global_path_share_sampled": share}),
                      flush=True)
    new.close()
    old.close()
    if bad:
        sys.exit(f"{bad} excerpts were not identified")


if __name__ == "__main__":
    main()
