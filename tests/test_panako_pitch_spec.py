"""The Panako vote whose bins follow the scale on the CPU: the numpy reference against the literal
reading of the definition, the closed-form hypothesis interval of a bin against the literal scan, the new integer pieces
of ucfp_amd/csrc/panako_match.h (compiled with g++ into a stand-alone program) against the reference, and the property
that justifies the feature: a resampled excerpt, whose every hash differs from the record's, still finds its recording."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import panako_match_ref as pm
import panako_pitch_ref as pp
import panako_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))


def _random_case(rng):
    """<= 5 records of <= 30 triples over a few base bins; the query's bins are the stored ones mapped through a scale
    with jitter, so true matches and near misses are dense.  Every parameter is drawn; both modes, f_slack 0 ... 3."""
    base = rng.integers(0, 512, (4, 3))
    base[0] = [0, 1, 2]                                             # small bins: clamps at 0, k = 0
    base[1] = [511, 509, 500]                                       # and at 511

    def hashes(n, s, jitter):
        b = base[rng.integers(0, 4, n)] + rng.integers(-2, 3, (n, 3)) * (rng.random((n, 3)) < 0.5)
        b = np.clip(b, 0, 511)
        k = np.clip((512 * b + s) // (2 * s) + rng.integers(-jitter, jitter + 1, (n, 3)), 0, 511) if s else b
        return (k[:, 0] << 23) | (k[:, 1] << 14) | (k[:, 2] << 5) | rng.integers(0, 3, n)

    def item(n, s=0, jitter=0):
        a = rng.integers(0, 60, n)
        d = rng.integers(1, 40, n)
        return np.stack([hashes(n, s, jitter), a, a, a + d], axis=1).astype(np.uint32)

    records = {int(i): item(int(rng.integers(0, 31))) for i in rng.choice(50, int(rng.integers(1, 6)), replace=False)}
    bins = int(rng.integers(0, 4) > 0)
    smin = int(rng.integers(64, 400))
    nh = int(rng.integers(1, 65))
    step = int(rng.integers(1, 9))
    match = dict(scale_min=smin, scale_max=min(1024, smin + (nh - 1) * step), scale_step=step,
                 window=int(rng.choice([1, 2, 5, 16, 256])), slack=int(rng.integers(0, 9)), r_slack=int(rng.integers(0, 2)),
                 bins=bins, f_slack=int(rng.integers(0, 4)) if bins else 0)
    # half of the query is stored triples as a copy played at s_true / 256 has them (record bin = B_s(query bin), so
    # query bin = record bin * s / 256; d likewise), with jitter; the rest is noise
    s_true = int(rng.integers(smin, match["scale_max"] + 1))
    q = item(int(rng.integers(0, 12)), 65536 // s_true if bins else 0, 2)
    stored = np.concatenate([r for r in records.values()] + [np.zeros((0, 4), np.uint32)]).astype(np.int64)
    if stored.shape[0]:
        t = stored[rng.integers(0, stored.shape[0], int(rng.integers(0, 14)))]
        kb = np.stack([(t[:, 0] >> 23) & 511, (t[:, 0] >> 14) & 511, (t[:, 0] >> 5) & 511], axis=1)
        if bins:
            kb = np.clip((kb * s_true + 128) // 256 + rng.integers(-1, 2, kb.shape) * (rng.random(kb.shape) < 0.3), 0, 511)
        h = (kb[:, 0] << 23) | (kb[:, 1] << 14) | (kb[:, 2] << 5) | (t[:, 0] & 31)
        d = np.clip(((t[:, 3] - t[:, 1]) * 256 + s_true // 2) // s_true + rng.integers(-1, 2, t.shape[0]), 1, 1023)
        a = rng.integers(0, 60, t.shape[0])
        q = np.concatenate([q, np.stack([h, a, a, a + d], axis=1).astype(np.uint32)])
    return (records, q, int(rng.choice([1, 2, 10])), int(rng.choice([0, 1, 2])), int(rng.choice([0, 0, 1, 3, 10])), match)


def test_reference_matches_brute_force_on_random_cases():
    rng = np.random.default_rng(2201)
    nonempty = {0: 0, 1: 0}
    capped = 0
    slacks = set()
    for i in range(360):
        records, q, k, min_votes, max_postings, match = _random_case(rng)
        got = pp.PanakoPitchRef(records, max_postings).query(q, k, min_votes, **match)
        want = pp.brute_force(records, q, k, min_votes, max_postings, **match)
        assert got == want, (i, match, max_postings)
        nonempty[match["bins"]] += bool(got)
        if got and match["bins"]:
            slacks.add(match["f_slack"])
        capped += bool(max_postings) and bool(match["bins"]) and got != pp.PanakoPitchRef(records).query(q, k, min_votes, **match)
    assert nonempty[0] >= 20 and nonempty[1] >= 100 and capped >= 5 and slacks == {0, 1, 2, 3}, (nonempty, capped, slacks)


def test_kept_mode_of_the_new_reference_is_the_old_reference():
    rng = np.random.default_rng(2202)
    for _ in range(40):
        records, q, k, min_votes, max_postings, match = _random_case(rng)
        match.update(bins=0, f_slack=0)
        old = {n: v for n, v in match.items() if n not in ("bins", "f_slack")}
        assert pp.PanakoPitchRef(records, max_postings).query(q, k, min_votes, **match) == \
            pm.PanakoMatchRef(records, max_postings).query(q, k, min_votes, **old)


def test_closed_form_interval_against_the_literal_scan():
    """For every k, k' in 0 ... 511 and f in 0 ... 3: {s in 64 ... 1024 : |k' - B_s(k)| <= f} is s_lo ... s_hi of the
    closed form, cut to 64 ... 1024."""
    s = np.arange(64, 1025, dtype=np.int32)
    kp = np.arange(512, dtype=np.int32)
    for k in range(512):
        dist = np.abs(kp[:, None] - pp.bin_map(s, k)[None, :])          # [k', s]
        for f in range(4):
            ok = dist <= f
            s_lo = (512 * k) // (2 * kp + 2 * f + 1) + 1
            den = 2 * (kp - f) - 1
            s_hi = np.where(kp - f >= 1, (512 * k) // np.maximum(den, 1), 1 << 20)
            want = (s[None, :] >= s_lo[:, None]) & (s[None, :] <= s_hi[:, None])
            assert np.array_equal(ok, want), (k, f)
    assert pp.bin_interval(1, 1, 0) == (171, 512) and pp.bin_interval(0, 2, 3) == (1, None)
    assert all(pp.bin_map(256, k) == k for k in range(512))
    assert all(pp.bin_map(s0 + 1, k) <= pp.bin_map(s0, k) for s0 in range(64, 1024) for k in (0, 1, 7, 255, 511))


@pytest.mark.parametrize("case", pp.corners(), ids=lambda c: c[0])
def test_fixed_corners(case):
    _, records, q, kw, want = case
    kw = dict(kw)
    max_postings = kw.pop("max_postings", 0)
    got = pp.PanakoPitchRef(records, max_postings).query(q, 5, **kw)
    assert got == pp.brute_force(records, q, 5, 1, max_postings, **kw)
    if want is not None:
        assert [h[:4] for h in got] == want
    if case[0].startswith("bins = 1, f_slack = 0, s = 256"):
        old = {n: v for n, v in kw.items() if n not in ("bins", "f_slack")}
        assert got == pm.PanakoMatchRef(records).query(q, 5, **old)
    if case[0].startswith("one posting votes under two"):
        assert pp.PanakoPitchRef(records).votes(q, **kw)[1].size == 3       # 254, 256 and 258


def test_invalid_configs():
    good = pm.rec((pm.H0, 1, 5))
    for match in pp.INVALID_CONFIGS + [dict(bins=1, f_slack=1, **m) for m in pm.INVALID_CONFIGS]:
        with pytest.raises(pp.Invalid):
            pp.PanakoPitchRef({1: good}).query(good, 1, **match)
        with pytest.raises(pp.Invalid):
            pp.brute_force({1: good}, good, 1, **match)
    pp.PanakoPitchRef({1: good}).query(good, 1, bins=1, f_slack=3)
    pp.PanakoPitchRef({1: good}).query(good, 1, bins=1, f_slack=0)


def _header_cases(rng, n):
    rows = []
    for i in range(n):
        smin = int(rng.integers(64, 1025))
        step = int(rng.choice([1, 2, 4, 7, 16, 100, 1 << 20]))
        smax = min(1024, smin + int(rng.integers(0, 64)) * step + int(rng.integers(0, min(step, 1024))))
        bins = int(i % 5 != 0)
        cfg = [smin, smax, step, int(rng.integers(1, 257)), int(rng.integers(0, 9)), int(rng.integers(0, 2)), bins,
               int(rng.integers(0, 4)) if bins else 0]
        if i % 40 == 0:                                # an invalid one now and then
            cfg = [cfg[:6] + [2, 0], cfg[:6] + [1, 4], cfg[:6] + [0, 1], [63] + cfg[1:], cfg[:5] + [2] + cfg[6:]][int(rng.integers(0, 5))]
        nh = (cfg[1] - cfg[0]) // cfg[2] + 1
        s = cfg[0] + int(rng.integers(0, max(1, min(nh, 64)))) * cfg[2]
        kq = rng.integers(0, 512, 3) if i % 7 else np.array([0, 511, int(rng.integers(0, 4))])
        kpost = np.clip((512 * kq + s) // (2 * s) + rng.integers(-cfg[7] - 1, cfg[7] + 2, 3), 0, 511)   # near a supported pair
        if i % 6 == 0:
            kpost = rng.integers(0, 512, 3)
        r = int(rng.integers(0, 32))
        h = (int(kq[0]) << 23) | (int(kq[1]) << 14) | (int(kq[2]) << 5) | r
        hp = (int(kpost[0]) << 23) | (int(kpost[1]) << 14) | (int(kpost[2]) << 5) | int(np.clip(r + rng.integers(-2, 3), 0, 31))
        d = int(rng.integers(1, max(2, min(1024, 1023 * 256 // s))))
        dp = int(np.clip(d * s // 256 + rng.integers(-cfg[4] - 1, cfg[4] + 2), 1, 1023))
        x = int(rng.integers(0, 3))
        rows.append(cfg + [h, d, hp, dp, int(kq[x]), int(kpost[x]), int(rng.integers(64, 1025))])
    return rows


def test_header_arithmetic_against_reference(tmp_path):
    """pk_plan_ex, pk_bin, pk_bin_interval, pk_interval_scaled and pk_bin_range of panako_match.h on 12 000 random
    (query triple, posting, config) cases, against the literal definition."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "panako_pitch_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "native", "panako_pitch_check.cpp"),
                    "-o", exe], check=True)
    rows = _header_cases(np.random.default_rng(2203), 12000)
    r = subprocess.run([exe], input="".join(" ".join(map(str, row)) + "\n" for row in rows), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    n_bad = n_support = n_bin = 0
    for row, line in zip(rows, lines):
        smin, smax, step, win, slack, rs, bins, f, h, d, hp, dp, k, kp, s = row
        try:
            c = pp.config(bins, f, scale_min=smin, scale_max=smax, scale_step=step, window=win, slack=slack, r_slack=rs)
        except pp.Invalid:
            assert line == "0", row
            n_bad += 1
            continue
        sc = c["scales"]
        got = [int(x) for x in line.split()]
        assert got[:3] == [1, len(sc), pp.bin_map(s, k)], row
        on_bin = [j for j, t in enumerate(sc) if abs(kp - pp.bin_map(t, k)) <= f]
        qb, pb = pp.bins_of(h), pp.bins_of(hp)
        sup = [j for j, t in enumerate(sc)
               if all(abs(pb[x] - pp.bin_map(t, qb[x])) <= f for x in range(3)) and abs(pb[3] - qb[3]) <= rs
               and abs(256 * dp - t * d) <= 256 * slack]
        for want, (lo, hi) in ((on_bin, got[3:5]), (sup, got[5:7])):
            if want:
                assert want == list(range(want[0], want[-1] + 1)) and [lo, hi] == [want[0], want[-1]], (row, want, lo, hi)
            else:
                assert lo > hi, (row, lo, hi)
        bm = [pp.bin_map(t, k) for t in sc]             # every bin some hypothesis reaches lies in the range
        assert got[7] == max(0, min(bm) - f) and got[8] == min(511, max(bm) + f), row
        n_support += bool(sup)
        n_bin += bool(on_bin)
    assert n_bad >= 100 and n_support >= 800 and n_bin >= 4000, (n_bad, n_support, n_bin)


@pytest.fixture(scope="module")
def recordings(oracle):
    return {100 + i: pr.panako_ref(oracle, pm.recording(i)) for i in range(pm.N_RECORDINGS)}


def test_a_resampled_excerpt_finds_its_recording(oracle, recordings):
    """Eight recordings of 20 s of tone bursts; the excerpt [4 s, 12 s) of recording 3 re-rendered at seven speeds with
    its frequencies multiplied by the speed, under bins = "scaled" and the Python defaults (scale_step 2, f_slack 1).
    The reference's votes for the true record and for any other, the offset (true value 250) and the scale:

        speed            0.85  0.9  0.96  1.0  1.03  1.1  1.2
        scaled, true      148  163   196  279   190  163  117
        scaled, other       0    0     0    1     1    0    0
        offset            248  249   248  248   249  249  249
        scale             218  230   246  256   264  282  308
        kept (A14), true    0    0     0  279     0    0    0
    """
    ref = pp.PanakoPitchRef(recordings)
    for speed in pm.SPEEDS:
        q = pr.panako_ref(oracle, pp.resampled_excerpt(3, speed))
        hits = ref.query(q, 8, bins=1, **pp.SCALED_DEFAULTS)
        kept = {h[0]: h[1] for h in ref.query(q, 8)}.get(103, 0)
        others = max([h[1] for h in hits[1:]], default=0)
        print(f"speed {speed}: {hits[:1]}, any other record {others}, kept mode {kept}")
        assert hits and hits[0][0] == 103, (speed, hits)
        assert hits[0][1] >= 3 * others and hits[0][1] >= 50, (speed, hits)
        assert abs(hits[0][2] - 250) <= pm.DEFAULTS["window"], (speed, hits[0])
        assert abs(hits[0][3] - 256 * speed) <= 6, (speed, hits[0])
        if speed != 1.0:
            assert kept == 0, (speed, kept)             # what A14 alone answers: nothing
