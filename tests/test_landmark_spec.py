"""Landmark index spec on the CPU: the numpy reference against the literal definitions, the
`landmarks` field of a query body, and the byte-stability of vector and Hamming hits."""
import json

import numpy as np
import pytest

from landmark_ref import LandmarkRef, brute_force
from ucfp_amd.core import Hit, HitSource, QueryRequest, hit_to_json
from ucfp_amd.errors import InvalidArgument


def _case(seed):
    rng = np.random.default_rng(seed)
    nrec = int(rng.integers(1, 9))
    alpha = rng.integers(0, 2**32, 6, dtype=np.uint64).astype(np.uint32)
    recs = {}
    for _ in range(nrec):
        rid = int(rng.integers(0, 50))
        n = int(rng.integers(0, 25))
        pairs = np.stack([alpha[rng.integers(0, alpha.size, n)], rng.integers(0, 12, n).astype(np.uint32)], 1)
        if n and rng.random() < 0.5:
            pairs = np.concatenate([pairs, pairs[: n // 2]])      # duplicates
        recs[rid] = pairs
    nq = int(rng.integers(0, 15))
    q = np.stack([alpha[rng.integers(0, alpha.size, nq)], rng.integers(0, 20, nq).astype(np.uint32)], 1)
    return recs, q


@pytest.mark.parametrize("seed", range(300))
def test_reference_matches_definition(seed):
    recs, q = _case(seed)
    for max_postings in (0, 3, 8):
        ref = LandmarkRef(recs, max_postings)
        for k, mv in ((1, 1), (5, 1), (128, 2), (0, 1)):
            assert ref.query(q, k, mv) == brute_force(recs, q, k, mv, max_postings)


def test_stop_cap_exactly_at_and_one_above():
    # hash 7 has 3 postings; hash 9 has 4: with max_postings = 3 only hash 9 is stopped
    recs = {1: [[7, 0], [7, 1], [9, 0], [9, 1]], 2: [[7, 5], [9, 5], [9, 6]]}
    q = [[7, 0], [9, 0]]
    ref = LandmarkRef(recs, 3)
    assert ref.query(q, 10) == brute_force(recs, q, 10, 1, 3) == [(1, 1, 0, 0.5), (2, 1, 5, 0.5)]
    assert LandmarkRef(recs, 4).query(q, 10) == [(1, 2, 0, 1.0), (2, 2, 5, 1.0)]


def test_negative_offsets_ties_and_duplicates():
    recs = {5: [[1, 0], [2, 1], [1, 10], [2, 11]], 3: [[1, 0], [2, 1]], 4: [[1, 0], [1, 0]]}
    q = [[1, 10], [2, 11], [1, 10]]
    # record 5 matches at d = 0 and d = -10 with 2 votes: the smallest offset wins; 3 ties 5 and comes first
    assert LandmarkRef(recs).query(q, 10) == brute_force(recs, q, 10) == [(3, 2, -10, 1.0), (5, 2, -10, 1.0),
                                                                           (4, 1, -10, 0.5)]
    assert LandmarkRef(recs).query(q, 10, 2) == [(3, 2, -10, 1.0), (5, 2, -10, 1.0)]
    assert LandmarkRef(recs).query([], 10) == [] and LandmarkRef({}).query(q, 10) == []


def test_query_body_landmarks():
    r = QueryRequest.from_json({"tenant_id": 3, "modality": "Audio", "landmarks": [[1, 2], [0xFFFFFFFF, 5]], "k": 4})
    assert r.landmarks == np.array([[1, 2], [0xFFFFFFFF, 5]], np.uint32).tobytes() and r.k == 4
    raw = np.array([[9, 1]], np.uint32).tobytes()
    assert QueryRequest.from_json({"tenant_id": 0, "modality": "Audio", "landmarks": raw}).landmarks == raw
    assert QueryRequest.from_json({"tenant_id": 0, "modality": "Audio", "landmarks": []}).landmarks == b""
    for bad in (raw[:7], raw + b"\0", [[1]], [[1, 2, 3]], [[1, 1 << 31]], [[1 << 32, 0]], [[-1, 0]], [["1", 2]], 5):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json({"tenant_id": 0, "modality": "Audio", "landmarks": bad})


def test_valid_bodies_unchanged():
    a = QueryRequest.from_json({"tenant_id": 1, "modality": "Image", "vector": [1, 2]})
    assert (a.vector, a.hash, a.landmarks) == ([1.0, 2.0], None, None)
    b = QueryRequest.from_json({"tenant_id": 1, "modality": "Image", "hash": 5, "algorithm": "x"})
    assert (b.hash, b.algorithm, b.landmarks) == (5, "x", None)
    with pytest.raises(InvalidArgument):
        QueryRequest.from_json({"tenant_id": 1, "modality": "Image"})


def test_hit_json_byte_stable():
    v = Hit(tenant_id=1, record_id=9, score=0.5, source=HitSource.Vector, vector_score=0.5, vector_rank=1)
    assert json.dumps(hit_to_json(v)) == ('{"tenant_id": 1, "record_id": 9, "score": 0.5, "source": "vector", '
                                          '"vector_score": 0.5, "bm25_score": null, "vector_rank": 1, "bm25_rank": null, '
                                          '"term_hits": []}')
    h = Hit(tenant_id=1, record_id=9, score=0.75, source=HitSource.Hamming, distance=16)
    assert json.dumps(hit_to_json(h)) == ('{"tenant_id": 1, "record_id": 9, "score": 0.75, "source": "hamming", '
                                          '"vector_score": null, "bm25_score": null, "vector_rank": null, '
                                          '"bm25_rank": null, "term_hits": [], "distance": 16}')
    lm = hit_to_json(Hit(tenant_id=1, record_id=9, score=0.25, source=HitSource.Landmark, votes=3, offset=-7))
    assert lm["source"] == "landmark" and lm["votes"] == 3 and lm["offset"] == -7 and "distance" not in lm
