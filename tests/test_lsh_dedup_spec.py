"""The LSH de-duplication spec (DESIGN.md "LSH" L5-L7) on the CPU: the restatement the GPU tests compare against
(tests/dedup_ref.py) agrees with the brute-force reading of the definitions, its `pairs` is the closed form, a bounded
span refines the unbounded clusters; plus the host-side pieces of the feature that need no device."""
import numpy as np
import pytest

import dedup_ref
from dedup_ref import SPAN_ALL, brute_force, dedup_ref as ref, pairs_closed_form, records_of

SHAPES = [(16, 8), (32, 4), (5, 3), (1, 64), (128, 1)]


def _small_corpus(rng):
    """5-60 rows over a tiny alphabet: a few bases and copies with some slots redrawn, so that runs, chains and
    near-misses all occur."""
    n = int(rng.integers(5, 61))
    alphabet = int(rng.integers(2, 5))
    bases = rng.integers(0, alphabet, size=(int(rng.integers(1, 5)), 128), dtype=np.uint64)
    rows = bases[rng.integers(0, bases.shape[0], n)]
    redraw = rng.random((n, 128)) < rng.choice([0.0, 0.02, 0.1, 0.3], size=(n, 1))
    rows = np.where(redraw, rng.integers(0, alphabet, size=(n, 128), dtype=np.uint64), rows)
    ids = rng.permutation(np.arange(1000, 1000 + n, dtype=np.uint64))
    return ids, records_of(rows)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("block", range(10))
def test_reference_equals_brute_force_when_span_covers_the_corpus(block):
    """300 seeded corpora (10 blocks of 30): runs + union-find == all n^2 pairs."""
    for seed in range(block * 30, block * 30 + 30):
        rng = np.random.default_rng(seed)
        ids, rec = _small_corpus(rng)
        n = rec.shape[0]
        bands, rows = SHAPES[seed % len(SHAPES)]
        min_agree = int(rng.choice([1, 40, 64, 90, 110, 128]))
        want = brute_force(ids, rec, bands, rows, min_agree)
        for span in (n, SPAN_ALL):
            got = ref(ids, rec, bands, rows, min_agree, span)
            assert _same(got, want), (seed, bands, rows, min_agree, span)


@pytest.mark.parametrize("span", [0, 1, 2, 16, 1000, SPAN_ALL])
def test_pairs_is_the_closed_form(span):
    for seed in range(40):
        rng = np.random.default_rng(5000 + seed)
        ids, rec = _small_corpus(rng)
        bands, rows = SHAPES[seed % len(SHAPES)]
        got = ref(ids, rec, bands, rows, 128, span)
        assert int(got[3][0]) == pairs_closed_form(rec, bands, rows, span), (seed, span)


def test_span_zero_means_sixteen():
    rng = np.random.default_rng(1)
    rows = np.repeat(rng.integers(0, 1 << 63, size=(1, 128), dtype=np.uint64), 40, axis=0)
    ids = np.arange(40, dtype=np.uint64)
    a, b = ref(ids, records_of(rows), 16, 8, 128, 0), ref(ids, records_of(rows), 16, 8, 128, 16)
    assert _same(a, b) and int(a[3][0]) == 16 * sum(min(16, 39 - i) for i in range(40))


def test_bounded_span_refines_the_unbounded_clusters():
    for seed in range(60):
        rng = np.random.default_rng(9000 + seed)
        ids, rec = _small_corpus(rng)
        bands, rows = SHAPES[seed % len(SHAPES)]
        min_agree = int(rng.choice([40, 64, 90, 110]))
        full = ref(ids, rec, bands, rows, min_agree, SPAN_ALL)[0]
        for span in (1, 2, 16):
            part = ref(ids, rec, bands, rows, min_agree, span)[0]
            # every bounded cluster lies inside one unbounded cluster, and its label is its smallest row
            assert np.array_equal(full[part], full), (seed, span)
            assert (part >= full).all() and (part <= np.arange(part.size)).all()


def test_chain_joins_rows_that_are_not_an_edge_themselves():
    """A-B and B-C are edges, A-C is a candidate (they share bands 4..15) but not an edge: one cluster of three."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 63, size=128, dtype=np.uint64)
    b = a.copy()
    b[:16] = rng.integers(0, 1 << 63, size=16, dtype=np.uint64)        # bands 0, 1 differ from A: agree 112
    c = b.copy()
    c[16:32] = rng.integers(0, 1 << 63, size=16, dtype=np.uint64)      # bands 2, 3 differ from B: agree(A, C) = 96
    noise = rng.integers(0, 1 << 63, size=(4, 128), dtype=np.uint64)
    rows = np.stack([noise[0], a, noise[1], b, noise[2], c, noise[3]])
    ids = np.arange(7, dtype=np.uint64) + np.uint64(70)
    labels, rep, keep, stats = ref(ids, records_of(rows), 16, 8, 100, 16)
    assert labels.tolist() == [0, 1, 2, 1, 4, 1, 6]
    assert rep.tolist() == [70, 71, 72, 71, 74, 71, 76] and keep.tolist() == [True, True, True, False, True, False, True]
    assert stats.tolist() == [14 + 14 + 12, 5, 2, 3]                   # bands shared: A-B 14, B-C 14, A-C 12
    # without B the two ends stay apart
    labels2 = ref(ids[[0, 1, 2, 4, 5, 6]], records_of(rows[[0, 1, 2, 4, 5, 6]]), 16, 8, 100, 16)[0]
    assert labels2.tolist() == [0, 1, 2, 3, 4, 5]


def test_min_agree_for():
    from ucfp_amd import text
    from ucfp_amd.errors import InvalidArgument
    assert text.min_agree_for(1 / 128) == 1
    assert text.min_agree_for(0.5) == 64
    assert text.min_agree_for(0.8) == 103
    assert text.min_agree_for(1.0) == 128
    assert text.min_agree_for(1e-9) == 1
    for bad in (0, 0.0, -0.1, -1, 1.0000001, 2, float("nan")):
        with pytest.raises(InvalidArgument):
            text.min_agree_for(bad)


def test_dedup_entry_point_rejects_null_index_without_a_gpu():
    """The symbol exists and validates on the host, before any device call."""
    from ucfp_amd import _lib
    lib = _lib.load()
    assert lib.ucfp_lsh_dedup_dev(None, 103, 16, None, None, None, None, None) == -4     # UCFP_E_INVALID
    assert b"lsh" in lib.ucfp_last_error()


def test_reference_module_names_the_default_span():
    assert dedup_ref.DEFAULT_SPAN == 16 and SPAN_ALL == 2**32 - 1
