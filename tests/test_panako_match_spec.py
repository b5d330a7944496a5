"""The Panako (scale, offset) vote on the CPU: the numpy reference against the literal reading of the
definitions, the integer pieces of ucfp_amd/csrc/panako_match.h (compiled with g++ into a stand-alone program) against
the reference, and the property that justifies the feature: a time-stretched excerpt still finds its recording."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import panako_match_ref as pm
import panako_ref as pr
from landmark_ref import LandmarkRef

HERE = os.path.dirname(os.path.abspath(__file__))


def _random_case(rng):
    """<= 6 records of <= 40 triples, hashes from few values (with neighbours in r), every parameter drawn."""
    bases = rng.integers(0, 1 << 27, 3) << 5
    pool = np.concatenate([bases | r for r in (0, 1, 2, 30, 31)])

    def item(n):
        h = rng.choice(pool, n)
        a = rng.integers(0, 60, n)
        d = rng.integers(1, 40, n)
        return np.stack([h, a, a, a + d], axis=1).astype(np.uint32)

    records = {int(i): item(int(rng.integers(0, 41))) for i in rng.choice(50, int(rng.integers(1, 7)), replace=False)}
    smin = int(rng.integers(64, 400))
    nh = int(rng.integers(1, 65))
    step = int(rng.integers(1, 40))
    match = dict(scale_min=smin, scale_max=min(1024, smin + (nh - 1) * step + int(rng.integers(0, step))), scale_step=step,
                 window=int(rng.choice([1, 2, 5, 16, 256])), slack=int(rng.integers(0, 9)), r_slack=int(rng.integers(0, 2)))
    if (match["scale_max"] - smin) // step + 1 > 64:
        match["scale_max"] = smin + 63 * step
    return (records, item(int(rng.integers(0, 30))), int(rng.choice([1, 2, 10])), int(rng.choice([0, 1, 2, 4])),
            int(rng.choice([0, 0, 1, 3, 10])), match)


def test_reference_matches_brute_force_on_random_cases():
    rng = np.random.default_rng(1401)
    nonempty = capped = 0
    for i in range(320):
        records, q, k, min_votes, max_postings, match = _random_case(rng)
        got = pm.PanakoMatchRef(records, max_postings).query(q, k, min_votes, **match)
        want = pm.brute_force(records, q, k, min_votes, max_postings, **match)
        assert got == want, (i, match, max_postings)
        nonempty += bool(got)
        capped += bool(max_postings) and got != pm.PanakoMatchRef(records).query(q, k, min_votes, **match)
    assert nonempty >= 150 and capped >= 10, (nonempty, capped)     # the cases are not vacuous


@pytest.mark.parametrize("case", pm.corners(), ids=lambda c: c[0])
def test_fixed_corners(case):
    _, records, q, match, want = case
    got = pm.PanakoMatchRef(records).query(q, 5, **match)
    assert got == pm.brute_force(records, q, 5, **match)
    if want is not None:
        assert [h[:4] for h in got] == want
    if case[0].startswith("pairs are counted"):
        assert got[0][4] == 3.0


def test_invalid_inputs():
    good = pm.rec((pm.H0, 1, 5))
    for name, item, bad_record, bad_query in pm.invalid_items():
        for bad, run in ((bad_record, lambda: pm.PanakoMatchRef({1: item})), (bad_query, lambda: pm.PanakoMatchRef({1: good}).query(item, 1))):
            if bad:
                with pytest.raises(pm.Invalid):
                    run()
            else:
                run()
    for match in pm.INVALID_CONFIGS:
        with pytest.raises(pm.Invalid):
            pm.PanakoMatchRef({1: good}).query(good, 1, **match)
        with pytest.raises(pm.Invalid):
            pm.brute_force({1: good}, good, 1, **match)
    assert len(pm.config(scale_min=200, scale_max=263, scale_step=1)["scales"]) == 64     # 64 hypotheses are allowed


def _header_cases(rng, n):
    rows = []
    for i in range(n):
        smin = int(rng.integers(64, 1025))
        step = int(rng.choice([1, 2, 4, 7, 16, 100, 1 << 20]))
        smax = min(1024, smin + int(rng.integers(0, 64)) * step + int(rng.integers(0, min(step, 1024))))
        cfg = [smin, smax, step, int(rng.integers(1, 257)), int(rng.integers(0, 9)), int(rng.integers(0, 2))]
        if i % 50 == 0:                                # an invalid one now and then
            cfg = [[63, smax, step] + cfg[3:], cfg[:3] + [257] + cfg[4:], cfg[:4] + [9, 0], cfg[:5] + [2],
                   [smin, min(1024, smin + 64), 1] + cfg[3:]][int(rng.integers(0, 5))]
        nh = (cfg[1] - cfg[0]) // cfg[2] + 1 if cfg[2] else 0
        s = cfg[0] + int(rng.integers(0, max(1, min(nh, 64)))) * cfg[2]
        d = int(rng.integers(1, max(2, min(1024, 1023 * 256 // s))))      # mostly near a supported pair
        dp = int(np.clip(d * s // 256 + rng.integers(-cfg[4] - 1, cfg[4] + 2), 1, 1023)) if i % 4 else int(rng.integers(1, 1024))
        a = int(rng.choice([0, 1, (1 << 28) - 1, int(rng.integers(0, 1 << 28)), int(rng.integers(0, 5000))]))
        ap = int(rng.choice([0, (1 << 31) - 1, int(rng.integers(0, 1 << 31)), int(rng.integers(0, 5000))]))
        h = int(rng.integers(0, 1 << 32)) if i % 3 else (int(rng.integers(0, 1 << 27)) << 5) | int(rng.choice([0, 31]))
        jmax = max(1, min(nh, 64))
        pair = []
        for _ in range(2):
            pair += [int(rng.integers(0, 1 << 23)), int(rng.integers(0, 1 << 26)), int(rng.integers(0, jmax)),
                     int(rng.choice([-(1 << 30), (1 << 31) - 1, int(rng.integers(-(1 << 30), 1 << 31)), int(rng.integers(-300, 300))]))]
        if i % 3 == 0:                                  # ties and near ties: same ordinal, count and hypothesis
            pair[4:7] = pair[0:3]
            if i % 6 == 0:
                pair[7] = pair[3] + int(rng.integers(0, 300)) if pair[3] < (1 << 31) - 300 else pair[3]
        rows.append(cfg + [h, a, d, ap, dp] + pair)
    return rows


def _sign(x, y):
    return (x > y) - (x < y)


def test_header_arithmetic_against_reference(tmp_path):
    """The probes, the supported interval, the offset, the preference rank and the order of the packed keys of
    panako_match.h, on 12 000 random (query triple, posting, config) cases."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "panako_match_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(HERE, "native", "panako_match_check.cpp"),
                    "-o", exe], check=True)
    rows = _header_cases(np.random.default_rng(1402), 12000)
    r = subprocess.run([exe], input="".join(" ".join(map(str, row)) + "\n" for row in rows), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    n_bad = n_support = 0
    for row, line in zip(rows, lines):
        smin, smax, step, win, slack, rs, h, a, d, ap, dp, o1, c1, j1, f1, o2, c2, j2, f2 = row
        try:
            c = pm.config(scale_min=smin, scale_max=smax, scale_step=step, window=win, slack=slack, r_slack=rs)
        except pm.Invalid:
            assert line == "0", row
            n_bad += 1
            continue
        sc = c["scales"]
        sup = [j for j, s in enumerate(sc) if abs(256 * dp - s * d) <= 256 * slack]
        assert sup == list(range(sup[0], sup[-1] + 1)) if sup else True        # one contiguous interval
        off = lambda s: ap - ((s * a + 128) >> 8)
        r0 = h & 31
        probes = [(h & ~31) | x for x in range(max(0, r0 - rs), min(31, r0 + rs) + 1)]
        rank = pm.pref_ranks(sc)
        past = (o2, j2) > (o1, j1) if (o2, j2) != (o1, j1) else f2 >= f1 + win
        want = [1, len(sc), probes[0], len(probes)]
        got = [int(x) for x in line.split()]
        assert got[:4] == want, row
        if sup:
            n_support += 1
            assert got[4:8] == [sup[0], sup[-1], off(sc[sup[0]]), off(sc[sup[-1]])], row
        else:
            assert got[4] > got[5], row
        assert got[8:] == [rank[j1], rank[j2], _sign((c1, -rank[j1], -f1), (c2, -rank[j2], -f2)),
                           _sign((o1, j1, f1), (o2, j2, f2)), int(past)], row
    assert n_bad >= 100 and n_support >= 5000, (n_bad, n_support)


@pytest.fixture(scope="module")
def recordings(oracle):
    return {100 + i: pr.panako_ref(oracle, pm.recording(i)) for i in range(pm.N_RECORDINGS)}


def test_a_stretched_excerpt_finds_its_recording(oracle, recordings):
    """Eight recordings of 20 s of tone bursts; the excerpt [4 s, 12 s) of recording 3 re-rendered at seven speeds,
    under the default match parameters.  The reference's votes for the true record (no other record gets any) against
    A10's over the (hash, t_anchor) projection:

        speed   0.85  0.9  0.96  1.0  1.03  1.1  1.2
        A14      186  193   196  279   186  191  183      offset 245 ... 251, scale within 4/256 of the speed
        A10       10   13    16  278    19    8    9
    """
    ref = pm.PanakoMatchRef(recordings)
    a10 = LandmarkRef({rid: pr.landmarks(r) for rid, r in recordings.items()})
    for speed in pm.SPEEDS:
        q = pr.panako_ref(oracle, pm.stretched_excerpt(3, speed))
        hits = ref.query(q, 8)
        others = max([h[1] for h in hits[1:]], default=0)
        old = {rid: v for rid, v, _, _ in a10.query(pr.landmarks(q), 8)}.get(103, 0)
        print(f"speed {speed}: {hits[0]}, any other record {others}, A10 {old}")
        assert hits[0][0] == 103 and hits[0][1] >= 3 * others and hits[0][1] >= 3, (speed, hits)
        assert abs(hits[0][2] - 250) <= pm.DEFAULTS["window"], (speed, hits[0])
        assert abs(hits[0][3] - 256 * speed) <= 12, (speed, hits[0])
        if speed != 1.0:
            assert 2 * old < hits[0][1], (speed, old, hits[0])
