"""CPU checks of tests/topk_ref.py, the numpy statement of the top-k contract the GPU tests compare against: the merge
against a literal pure-Python definition, and the cosine key image against the properties cosine.hip's
score_to_key / key_to_score promise."""
import numpy as np
import pytest

import topk_ref as ref


def _merge_literal(ids, keys, k):
    """The contract, word for word, on Python ints."""
    parts, nq, k_in = len(ids), len(ids[0]), len(ids[0][0])
    out = []
    for q in range(nq):
        pairs = set()
        for p in range(parts):
            for e in range(k_in):
                if keys[p][q][e] != 0xFFFFFFFF:
                    pairs.add((keys[p][q][e], ids[p][q][e]))
        best = sorted(pairs)[:k]
        pad = k - len(best)
        out.append(([i for _, i in best] + [2**64 - 1] * pad, [d for d, _ in best] + [0xFFFFFFFF] * pad, len(best)))
    return out


@pytest.mark.parametrize("seed", range(12))
def test_merge_lists_matches_literal_definition(seed):
    rng = np.random.default_rng(seed)
    parts, nq, k_in = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 9))
    k = int(rng.integers(1, 12))                                   # below, at and above the number of distinct pairs
    # few distinct keys and ids: ties, duplicates across parts, the same id under two keys, invalid entries anywhere
    key_pool = np.array([0, 1, 64, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    id_pool = np.array([0, 1, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**64 - 2], np.uint64)
    keys = key_pool[rng.integers(0, key_pool.size, (parts, nq, k_in))]
    ids = id_pool[rng.integers(0, id_pool.size, (parts, nq, k_in))]
    if seed % 3 == 0:
        keys[:, 0, :] = 0xFFFFFFFF                                 # an all-empty query
    g_ids, g_keys, g_cnt = ref.merge_lists(ids, keys, k)
    assert g_ids.dtype == np.uint64 and g_keys.dtype == np.uint32 and g_ids.shape == (nq, k) == g_keys.shape
    want = _merge_literal(ids.tolist(), keys.tolist(), k)
    for q in range(nq):
        assert g_ids[q].tolist() == want[q][0], q
        assert g_keys[q].tolist() == want[q][1], q
        assert int(g_cnt[q]) == want[q][2], q


def test_merge_lists_orders_ids_unsigned_and_emits_pairs_once():
    ids = np.array([[[2**63, 5, 2**32]], [[5, 2**64 - 2, 5]]], np.uint64)
    keys = np.array([[[3, 3, 3]], [[3, 3, 2]]], np.uint32)
    g_ids, g_keys, g_cnt = ref.merge_lists(ids, keys, 6)
    assert g_ids[0].tolist() == [5, 5, 2**32, 2**63, 2**64 - 2, 2**64 - 1]      # id 5 under two keys: twice
    assert g_keys[0].tolist() == [2, 3, 3, 3, 3, 0xFFFFFFFF]
    assert g_cnt.tolist() == [5]


def test_hamming_scores():
    d = np.arange(65, dtype=np.uint32)
    s = ref.hamming_scores(d)
    assert s.dtype == np.float32 and s[0] == 1.0 and s[64] == 0.0 and s[32] == 0.5
    assert np.array_equal(s, (1.0 - d.astype(np.float64) / 64.0).astype(np.float32))    # every d / 64 is exact in f32
    assert ref.hamming_scores(np.array([0xFFFFFFFF], np.uint32))[0] == np.float32(-1.0)


def test_cosine_key_round_trips_bit_exactly():
    rng = np.random.default_rng(5)
    bits = np.concatenate([rng.integers(0, 2**32, 200_000, dtype=np.uint64).astype(np.uint32),
                           ref.edge_floats().view(np.uint32)])
    f = bits.view(np.float32)
    bits = bits[~np.isnan(f)]
    back = ref.cosine_score(ref.cosine_key(bits.view(np.float32)))
    assert np.array_equal(back.view(np.uint32), bits)
    keys = rng.integers(0, 2**32, 200_000, dtype=np.uint64).astype(np.uint32)
    keys = keys[~np.isnan(ref.cosine_score(keys))]
    assert np.array_equal(ref.cosine_key(ref.cosine_score(keys)), keys)


def test_cosine_key_strictly_reverses_order():
    f = ref.edge_floats()
    assert np.all(f[:-1] <= f[1:]) and np.signbit(f[6]) and f[6] == 0 and not np.signbit(f[7]) and f[7] == 0
    assert {float(x) for x in f} >= {-np.inf, -1.0, 0.0, 1.0, np.inf}
    keys = ref.cosine_key(f).astype(np.int64)
    assert np.all(np.diff(keys) < 0), keys                         # ascending floats, strictly descending keys
    assert ref.cosine_key(np.float32(0.0)) < ref.cosine_key(np.float32(-0.0))          # +0.0 ahead of -0.0
    assert ref.cosine_key(np.float32(-0.0)) == np.uint32(0x80000000)                   # scores <= -0.0: keys >= 2^31
    assert ref.cosine_key(np.float32(0.0)) == np.uint32(0x7FFFFFFF)
    rng = np.random.default_rng(6)
    r = np.sort(rng.standard_normal(50_000).astype(np.float32))
    r = r[np.concatenate([[True], np.diff(r) > 0])]
    assert np.all(np.diff(ref.cosine_key(r).astype(np.int64)) < 0)


def test_no_score_has_the_invalid_key():
    """0xffffffff is the image of a NaN bit pattern only: the largest key of a real score is that of -inf."""
    s = ref.cosine_score(np.array([0xFFFFFFFF], np.uint32))
    assert np.isnan(s[0])
    assert ref.cosine_key(np.float32(-np.inf)) == np.uint32(0xFF800000)
    assert ref.cosine_key(np.float32(np.inf)) == np.uint32(0x007FFFFF)
    keys = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    sc = ref.cosine_scores(keys)
    assert sc[-1] == np.float32(-2.0) and sc.dtype == np.float32
    assert np.array_equal(sc[:-1].view(np.uint32), ref.cosine_score(keys[:-1]).view(np.uint32))
