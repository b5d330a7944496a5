"""The float64 cosine reference (tests/cosine_ref.py) on the CPU: over every case of the small-shard GPU tests its own answer
passes its checker -- which asserts, from the reference alone, that at most a tenth of a case's places are near-ties exempt
from the id comparison -- and answers that are wrong in one respect do not."""
import numpy as np
import pytest

from cosine_ref import INVALID_ID, CosineRef, make_case
from test_index_gpu import (COS_TOL, COSINE_BOUNDARY_NQ, COSINE_BOUNDARY_SHAPE, COSINE_SMALL_SHARD_CASES,
                            COSINE_UNALIGNED_CASES, COSINE_UNALIGNED_K, _cosine_boundary_case, _cosine_case_seed)


def test_reference_answer_passes_on_every_gpu_case():
    for n, dim, nq, k, _, _ in COSINE_SMALL_SHARD_CASES:
        ids, rows, queries = make_case(n, dim, nq, _cosine_case_seed(n, dim, nq, k))
        ref = CosineRef(ids, rows, queries, k)
        g_ids, g_sc, g_c = ref.answer(k)
        assert ref.check(g_ids, g_sc, g_c, k, COS_TOL) <= 1e-7, (n, dim, nq, k)        # f32 rounding of a score <= 1
        if nq >= 3:
            assert g_c[2] == 0                                                          # the zero-norm query
        if n > 40:
            p0 = ref.best[0][0][0]                                                      # query 0's match, between the NaN and the Inf row
            assert g_sc[0, 0] > 0.999999 and ref.bad[p0 - 1] and ref.bad[p0 + 1] and (p0 - 1) // 8 == (p0 + 1) // 8
    ids, rows, queries, ref = _cosine_boundary_case()
    assert queries.shape[0] == max(COSINE_BOUNDARY_NQ)
    for k in (10, COSINE_BOUNDARY_SHAPE[2]):
        g_ids, g_sc, g_c = ref.answer(k)
        for nq in COSINE_BOUNDARY_NQ:
            ref.check(g_ids[:nq], g_sc[:nq], g_c[:nq], k, COS_TOL)
    for n, dim, nq in COSINE_UNALIGNED_CASES:
        k = COSINE_UNALIGNED_K
        ids, rows, queries = make_case(n, dim, nq, _cosine_case_seed(n, dim, nq, k))
        ref = CosineRef(ids, rows, queries, k)
        ref.check(*ref.answer(k), k, COS_TOL)


def test_checker_rejects_wrong_answers():
    n, dim, nq, k = 300, 24, 4, 5
    ids, rows, queries = make_case(n, dim, nq, 1)
    ref = CosineRef(ids, rows, queries, k)
    good = ref.answer(k)
    ref.check(*good, k, COS_TOL)
    assert good[2][2] == 0 and (good[0][2] == INVALID_ID).all()
    order1 = ref.best[1][0]
    assert all(np.array_equal(rows[order1[0]], rows[r]) for r in order1[:4])           # the four copies lead query 1 ...
    assert (np.diff(good[0][1, :4].astype(np.int64)) > 0).all()                         # ... in id order

    def broken(change):
        g_ids, g_sc, g_c = (a.copy() for a in good)
        change(g_ids, g_sc, g_c)
        with pytest.raises(AssertionError):
            ref.check(g_ids, g_sc, g_c, k, COS_TOL)

    def swap_copies(g_ids, g_sc, g_c):
        g_ids[1, [0, 1]] = g_ids[1, [1, 0]]

    def swap_decided(g_ids, g_sc, g_c):
        g_ids[3, [0, 1]] = g_ids[3, [1, 0]]

    def score_off(g_ids, g_sc, g_c):
        g_sc[3, 2] += np.float32(3e-5)

    def copy_score_off(g_ids, g_sc, g_c):
        g_sc[1, 1] = np.nextafter(g_sc[1, 1], np.float32(0))

    def count_off(g_ids, g_sc, g_c):
        g_c[2] = 1

    def zero_row_hit(g_ids, g_sc, g_c):
        g_ids[3, k - 1] = ref.bad_ids[0]

    def kth_replaced(g_ids, g_sc, g_c):        # the k-th place is not exempt when the (k+1)-th is far behind
        g_ids[0, k - 1] = ids[ref.best[0][0][k]]

    def hit_beyond_count(g_ids, g_sc, g_c):    # the zero-norm query has no hits: every place of it holds INVALID_ID
        g_ids[2, 0] = ids[0]

    assert ref.best[0][1][k - 1] - ref.best[0][1][k] > 2 * COS_TOL
    assert ref.best[3][1][0] - ref.best[3][1][1] > 2 * COS_TOL and ref.best[3][1][1] - ref.best[3][1][2] > 2 * COS_TOL
    for change in (swap_copies, swap_decided, score_off, copy_score_off, count_off, zero_row_hit, kth_replaced,
                   hit_beyond_count):
        broken(change)


def test_checker_rejects_rising_scores():
    """Two rows 4e-6 apart in score, among 28 far apart: either order of their ids passes, and each score may be off by the
    tolerance, but the answer's scores must not rise from one place to the next."""
    t = np.concatenate([[0.1, 0.10004], 0.1 * np.arange(2, 30)])
    rows = np.stack([np.cos(t), np.sin(t)], axis=1).astype(np.float32)
    ref = CosineRef(np.arange(30, dtype=np.uint64), rows, np.array([[1.0, 0.0]], np.float32), 20)
    g_ids, g_sc, g_c = ref.answer(20)
    assert 2e-6 < g_sc[0, 0] - g_sc[0, 1] < 6e-6
    ref.check(g_ids, g_sc, g_c, 20, COS_TOL)
    g_ids[0, [0, 1]] = g_ids[0, [1, 0]]
    ref.check(g_ids, g_sc, g_c, 20, COS_TOL)
    g_sc[0, [0, 1]] = g_sc[0, [1, 0]]
    with pytest.raises(AssertionError):
        ref.check(g_ids, g_sc, g_c, 20, COS_TOL)


def test_checker_caps_the_share_of_near_ties():
    """Rows that differ by less than the tolerance everywhere: nearly every place is exempt, and the checker says so."""
    rng = np.random.default_rng(3)
    base = rng.standard_normal(16).astype(np.float32)
    rows = base + np.float32(1e-4) * rng.standard_normal((50, 16)).astype(np.float32)
    ids = np.arange(50, dtype=np.uint64)
    ref = CosineRef(ids, rows, base[None, :], 10)
    with pytest.raises(AssertionError):
        ref.check(*ref.answer(10), 10, COS_TOL)
