"""The LSH edge cases of tests/lsh_cases.py are what they claim to be, proved from the numpy checker alone (no GPU):
test_lsh_edges_gpu.py compares the kernels with the checker on these cases, and these tests say that each case does
sit on its edge -- the run ends at n, the list is cut at the entry it names, the one band matches and no other.
Plus one statement that is independent of keys and sorting: where no cap binds, the checker equals brute force."""
import functools

import numpy as np
import pytest

import lsh_cases as lc
from lsh_cases import RUN_CAPS, RUN_LENGTHS, SWEEP_SHAPES, SWEEP_SIZES


def _tables(oracle, corpus, bands, rows):
    """Per band the stably sorted (keys, rows) table of L2, from the checker's keys."""
    ck = oracle.lsh_band_keys(lc.records(corpus), bands, rows)
    order = [np.argsort(ck[:, b], kind="stable") for b in range(bands)]
    return [(ck[order[b], b], order[b]) for b in range(bands)]


def _precut(oracle, corpus, query, bands, rows, cap, tables=None):
    """The concatenated candidate list of L3 before the cut at 1024, and per band (lower bound, run length)."""
    qk = oracle.lsh_band_keys(lc.records(query[None]), bands, rows)[0]
    out, runs = [], []
    for b, (sk, order) in enumerate(tables or _tables(oracle, corpus, bands, rows)):
        lo, hi = np.searchsorted(sk, qk[b], "left"), np.searchsorted(sk, qk[b], "right")
        runs.append((int(lo), int(hi - lo)))
        out += order[lo:min(hi, lo + cap)].tolist()
    return out, runs


def _query(oracle, case, k):
    ids, corpus, queries, p, _ = case
    return oracle.lsh_query(ids, lc.records(corpus), lc.records(queries), k, p["bands"], p["rows"], p["cand_per_band"])


def _agree(corpus, q):
    return (corpus == q).sum(axis=1)


def test_records_cover_the_full_slot_range():
    slots = np.array([[0, lc.M64, 1 << 63, (1 << 63) - 1] * 32], np.uint64)
    rec = lc.records(slots)
    assert rec.shape == (1, 1032) and rec[0, 0] == 1 and not rec[0, 1:8].any()
    assert np.array_equal(rec[0, 8:].view("<u8"), slots[0])
    assert lc._slots(lc._rng("range"), 64).max() >= np.uint64(1 << 63)


@pytest.mark.parametrize("bands,rows", SWEEP_SHAPES)
def test_one_band_queries_match_exactly_one_band(oracle, bands, rows):
    for n in SWEEP_SIZES:
        ids, corpus, queries, p, f = lc.one_band_matches(bands, rows, n)
        assert np.unique(ids).size == n and corpus.shape == (n, 128)
        ck = oracle.lsh_band_keys(lc.records(corpus), bands, rows)
        qk = oracle.lsh_band_keys(lc.records(queries), bands, rows)
        for b in range(bands):
            hit = ck == qk[b]                                   # [n, bands]
            assert hit.sum() == 1 and hit[f["band_src"][b], b]
            assert _agree(corpus, queries[b])[f["band_src"][b]] == rows
        for j, r in enumerate(f["whole"]):
            assert (ck[r] == qk[bands + j]).all() and np.array_equal(queries[bands + j], corpus[r])
        assert {0, n - 1} <= set(f["band_src"]) | set(f["whole"])
        o_ids, o_sc, o_ct = _query(oracle, (ids, corpus, queries, p, f), 128)
        assert (o_ct == 1).all()
        assert np.array_equal(o_ids[:bands, 0], ids[f["band_src"]])
        assert (o_sc[:bands, 0] == np.float32(rows / 128)).all() and (o_sc[bands:, 0] == 1).all()


@pytest.mark.parametrize("bands,rows", [s for s in SWEEP_SHAPES if s[0] * s[1] < 128])
def test_uncovered_slots_score_but_never_nominate(oracle, bands, rows):
    for n in SWEEP_SIZES:
        case = lc.uncovered_slots(bands, rows, n)
        ids, corpus, queries, p, f = case
        u = f["uncovered"]
        assert u == 128 - bands * rows and np.unique(ids).size == n
        o_ids, o_sc, o_ct = _query(oracle, case, 128)
        seen = set()
        for j, (kind, s, agree) in enumerate(f["kinds"]):
            seen.add(kind)
            if kind == "U":                                     # u equal slots, none of them in a band
                assert _agree(corpus, queries[j])[s] == u and o_ct[j] == 0
            elif kind == "P":
                p0, p1, p2, p3 = f["planted"]["rows"]
                assert _agree(corpus, queries[j])[[p0, p1, p2, p3]].tolist() == f["planted"]["agree"]
                assert o_ct[j] == 3 and o_ids[j, :3].tolist() == ids[[p1, p2, p3]].tolist()
                assert o_sc[j, :3].tolist() == [(rows + u) / 128, (rows + u // 2) / 128, rows / 128]
                assert ids[p3] < ids[p2] < ids[p1]              # the score ranks them, the id would not
                assert ids[p0] not in o_ids[j]
            else:
                assert _agree(corpus, queries[j])[s] == agree
                assert o_ct[j] == 1 and o_ids[j, 0] == ids[s] and o_sc[j, 0] == np.float32(agree / 128)
                if kind == "MIX":                               # the absent row agrees in at least as many slots
                    assert _agree(corpus, queries[j])[(s + 1) % n] == u and u >= 1
        assert {"U", "BA", "BH", "BD"} <= seen and ("MIX" in seen) == (n >= 2) and ("P" in seen) == (n >= 16)
        assert len({a for k_, _, a in f["kinds"] if k_ in ("BA", "BH", "BD")}) == 3     # the uncovered slots move the score


@pytest.mark.parametrize("position", lc.POSITIONS)
@pytest.mark.parametrize("L", RUN_LENGTHS)
def test_run_sits_where_it_says(oracle, position, L):
    ids, corpus, queries, p, f = lc.run_at(position, L)
    n, b = f["n"], f["band"]
    assert corpus.shape[0] == n == ids.size == np.unique(ids).size
    sk, order = _tables(oracle, corpus, p["bands"], p["rows"])[b]
    key = oracle.lsh_band_keys(lc.records(queries[:1]), p["bands"], p["rows"])[0, b]
    lo, hi = np.searchsorted(sk, key, "left"), np.searchsorted(sk, key, "right")
    assert hi - lo == L                                                     # the run length, exactly
    assert order[lo:hi].tolist() == f["run_rows"] == sorted(f["run_rows"])  # rows ascend inside the run
    if position == "first":
        assert lo == 0 and (hi < n or L == n)
    if position == "last":
        assert hi == n and n == 256 + L                                     # the run ends at n exactly
    if position == "middle":
        assert 0 < lo and hi < n
    if position == "whole_table":
        assert lo == 0 and hi == n == L
    # query 0 meets the run in that band alone; ids do not follow the rows
    lst, runs = _precut(oracle, corpus, queries[0], p["bands"], p["rows"], 1 << 20)
    assert lst == f["run_rows"] and [r[1] for r in runs] == [L if i == b else 0 for i in range(p["bands"])]
    if L >= 63:
        run_ids = ids[f["run_rows"]]
        assert (np.diff(run_ids.astype(np.float64)) < 0).any() and (np.diff(run_ids.astype(np.float64)) > 0).any()
        assert len(set(_agree(corpus, queries[0])[f["run_rows"]].tolist())) == 7    # rows differ outside the band
    # query 1 is the run's last row; query 2 finds nothing
    assert np.array_equal(queries[1], corpus[f["run_rows"][-1]])
    assert _precut(oracle, corpus, queries[2], p["bands"], p["rows"], 1 << 20)[0] == []
    # what the cap does to the run: the first `cap` rows stay
    for cap in RUN_CAPS:
        o_ids, o_sc, o_ct = oracle.lsh_query(ids, lc.records(corpus), lc.records(queries), 128, p["bands"], p["rows"], cap)
        assert o_ct[0] == min(L, cap, 128) and o_ct[2] == 0
        if min(L, cap) <= 128:
            assert set(o_ids[0, :o_ct[0]].tolist()) == set(ids[f["run_rows"][:cap]].tolist())
        assert o_ids[1, 0] == ids[f["run_rows"][-1]] and o_sc[1, 0] == 1     # found through the other bands


@pytest.mark.parametrize("variant", lc.CUT_VARIANTS)
def test_cut_cases_sit_on_the_cut(oracle, variant):
    case = lc.cut_at_1024(variant)
    ids, corpus, queries, p, f = case
    lst, _ = _precut(oracle, corpus, queries[0], p["bands"], p["rows"], p["cand_per_band"])
    assert len(lst) == f["precut"]
    want = {"inside": (1024, 1023), "outside_cut": (1040, 1039), "outside_cap": (1024, None), "duplicates": (1040, None),
            "dup_inside": (1009, 1008), "dup_outside": (1025, 1024), "b128_cap8": (129, 128), "b128_cap64": (1025, 1024)}
    assert (f["precut"], f["x_entry"]) == want[variant]
    x = f["x"]
    if x is not None:
        assert _agree(corpus, queries[0])[x] == f["x_agree"]
        assert (lst.index(x) if x in lst else None) == f["x_entry"] and lst.count(x) <= 1
    present = f["x_entry"] is not None and f["x_entry"] < lc.MAX_CAND
    for k in (1, 128):
        o_ids, o_sc, o_ct = _query(oracle, case, k)
        distinct = len(set(lst[:lc.MAX_CAND]))
        assert o_ct[0] == min(k, distinct)
        if x is not None and (k == 128 or variant != "dup_inside"):     # there the 63 copies of q outrank X
            assert (ids[x] in o_ids[0]) == present
    o_ids, o_sc, _ = _query(oracle, case, 1)
    if variant == "inside":
        assert o_ids[0, 0] == ids[x] and o_sc[0, 0] == np.float32(0.8828125)
    if variant in ("outside_cut", "outside_cap"):
        assert o_sc[0, 0] == np.float32(0.0625)
    if variant == "duplicates":
        assert len(set(lst)) == 65 and o_sc[0, 0] == 1
    if variant == "dup_inside":
        assert len(set(lst[:1024])) == 64
    if variant == "dup_outside":
        assert len(set(lst[:1024])) == 64 and len(set(lst)) == 65      # cut first, duplicates dropped afterwards
    if variant.startswith("b128"):                                      # every score ties: X would come first by id
        assert o_sc[0, 0] == np.float32(1 / 128) and ids[x] == ids.min()


@pytest.mark.parametrize("order", lc.ORDERS)
@pytest.mark.parametrize("mixed_ids", [False, True])
def test_graded_case_fills_the_list(oracle, order, mixed_ids):
    case = lc.graded(order, mixed_ids=mixed_ids)
    ids, corpus, queries, p, f = case
    m = f["n_cand"]
    assert 260 <= m <= 340 and np.unique(ids).size == ids.size
    agree = _agree(corpus, queries[0])[:m]
    assert np.array_equal(agree, f["agree"]) and set(agree.tolist()) == set(range(8, 129))
    ties = np.bincount(agree)[8:]
    assert ties.min() >= 2 and ties.max() <= 4 and {2, 3, 4} == set(ties.tolist())
    lst, runs = _precut(oracle, corpus, queries[0], 16, 8, 1024)
    assert runs[0][1] == m and lst[:m] == list(range(m))           # band 0 brings all of them, in row order
    assert len(set(lst[:1024])) == m > 128
    d = np.diff(agree)
    assert {"ascending": (d >= 0).all(), "descending": (d <= 0).all(), "random": (d > 0).any() and (d < 0).any()}[order]
    cand_ids = ids[:m]
    if mixed_ids:
        assert (cand_ids < np.uint64(1 << 63)).sum() > 100 and (cand_ids >= np.uint64(1 << 63)).sum() > 100
        lows = [(cand_ids[agree == a] < np.uint64(1 << 63)) for a in range(8, 129)]
        assert sum(1 for t in lows if t.any() and not t.all()) > 30      # ties that a signed compare gets wrong
    else:
        assert (ids >= np.uint64(1 << 63)).all()
    assert sorted(cand_ids[agree == 128].tolist())[-2:] == [lc.M64 - 1, lc.M64]
    assert (np.diff(cand_ids.astype(np.float64)) < 0).any() and (np.diff(cand_ids.astype(np.float64)) > 0).any()
    o_ids, o_sc, o_ct = _query(oracle, case, 128)
    n_full = int((agree == 128).sum())
    assert o_ct[0] == 128 and o_ids[0, n_full - 1] == lc.M64 and o_ids[0, n_full - 2] == lc.M64 - 1
    # query 1: few candidates, all tied at 8, ranked by id alone; the found 2^64-1 is the last of them
    c1 = int(o_ct[1])
    assert 3 <= c1 < 63 and (o_sc[1, :c1] == np.float32(8 / 128)).all()
    assert o_ids[1, c1 - 1] == lc.M64 and o_ids[1, c1 - 2] == lc.M64 - 1
    assert (np.diff(o_ids[1, :c1].astype(np.float64)) >= 0).all() and np.unique(o_ids[1, :c1]).size == c1
    assert (o_ids[1, c1:] == lc.M64).all() and (o_sc[1, c1:] == -1).all()


def test_resize_sequence_is_disjoint_and_looks_back(oracle):
    steps = lc.resize_sequence()
    assert [s[1].shape[0] for s in steps] == [5000, 10, 70_001, 0, 300]
    all_ids = np.concatenate([s[0] for s in steps])
    assert np.unique(all_ids).size == all_ids.size
    allrows = np.concatenate([s[1] for s in steps])
    assert np.unique(allrows[:, 0]).size == allrows.shape[0]            # disjoint corpora: even slot 0 never repeats
    for i, (ids, corpus, queries, p, f) in enumerate(steps):
        n_prev = [s[1].shape[0] for s in steps[:i] if s[1].shape[0]]
        assert queries.shape[0] == f["n_own"] + 3 * len(n_prev)
        if i:
            assert queries.shape[0] > f["n_own"]                        # rows of earlier builds are asked for
        if n_prev and i in (1, 3, 4):
            prev = [s[1] for s in steps[:i] if s[1].shape[0]][-1]
            assert prev.shape[0] > corpus.shape[0]                      # the previous build was larger
            assert np.array_equal(queries[f["n_own"]], prev[0])
            assert np.array_equal(queries[f["n_own"] + 2], prev[-1])   # ... and its last row sat behind the new n
    # the checker on the two small steps (the GPU test compares every step)
    for i in (1, 4):
        ids, corpus, queries, p, f = steps[i]
        o_ids, o_sc, o_ct = _query(oracle, steps[i], 4)
        assert o_ct.tolist() == [1] * f["n_own"] + [0] * (queries.shape[0] - f["n_own"])
        assert o_ids[:f["n_own"], 0].tolist() == ids[f["own"]].tolist()


# ---- the checker against brute force: no keys, no sort ----

def _brute(ids, corpus, queries, k, bands, rows):
    """A row is a candidate iff the slots of some band are all equal, slot by slot; rank by (-agreement, id)."""
    nq = queries.shape[0]
    o_ids = np.full((nq, k), lc.M64, np.uint64)
    o_sc = np.full((nq, k), -1.0, np.float32)
    o_ct = np.zeros(nq, np.uint32)
    for q in range(nq):
        eq = corpus == queries[q]                                                   # [n, 128]
        cand = eq[:, :bands * rows].reshape(-1, bands, rows).all(axis=2).any(axis=1)
        agree = eq.sum(axis=1)
        best = sorted((-int(agree[r]), int(ids[r])) for r in np.flatnonzero(cand))[:k]
        o_ct[q] = len(best)
        for j, (na, i) in enumerate(best):
            o_ids[q, j] = i
            o_sc[q, j] = np.float32(-na / 128)
    return o_ids, o_sc, o_ct


@functools.lru_cache(maxsize=None)
def _brute_corpus():
    """About 1800 rows: noise, 40 families of 6 near copies at several keep rates, a few exact copies.  Fewer than 64
    rows share any band with any query and the lists stay below 1024 even at 128 x 1, so no cap binds."""
    rng = lc._rng("brute")
    bases = lc._slots(rng, 40)
    rows = [lc._slots(rng, 1500)]
    for v in range(6):
        keep = rng.random((40, 128)) < (0.5 + 0.08 * v)
        rows.append(np.where(keep, bases, lc._slots(rng, 40)))
    rows.append(bases[:20])
    corpus = np.concatenate(rows)
    corpus = corpus[rng.permutation(corpus.shape[0])]
    ids = lc._ids(rng, corpus.shape[0])
    queries = np.concatenate([bases, corpus[:10], lc._slots(rng, 5)])
    return ids, corpus, queries


@pytest.mark.parametrize("bands,rows", [(16, 8), (32, 4), (20, 6), (128, 1), (64, 2), (5, 3), (3, 42), (7, 9), (1, 64),
                                        (1, 1)])
@pytest.mark.parametrize("k", [1, 128])
def test_checker_equals_brute_force_where_no_cap_binds(oracle, bands, rows, k):
    ids, corpus, queries = _brute_corpus()
    got = oracle.lsh_query(ids, lc.records(corpus), lc.records(queries), k, bands, rows, cand_per_band=64)
    want = _brute(ids, corpus, queries, k, bands, rows)
    tables = _tables(oracle, corpus, bands, rows)
    for q in range(queries.shape[0]):                               # the premise: no cap binds
        lst, runs = _precut(oracle, corpus, queries[q], bands, rows, 64, tables)
        assert max(r[1] for r in runs) <= 64 and len(lst) <= lc.MAX_CAND
    assert want[2].max() >= 1 and want[2].min() == 0
    if bands * rows >= 120 and rows <= 8:
        assert want[2].max() >= min(k, 5)                           # the families are found
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
