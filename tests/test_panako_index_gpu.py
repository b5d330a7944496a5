"""Identification from Panako records: a GpuIndex keeps the (hash, t_anchor) pairs of
`audiofp-panako-v1` records in a landmark index of their own; excerpts fingerprinted on the device find their recording
at rank 1 with the exact offset, every hit equals tests/landmark_ref.py, and the Wang index never answers for them."""
import numpy as np
import pytest

import panako_ref as pr
from landmark_ref import LandmarkRef

pytestmark = pytest.mark.gpu

TENANT = 1
PANAKO_IDS = [100 + i for i in range(pr.N_RECORDINGS)]
WANG_IDS = [200, 201]


@pytest.fixture(scope="module")
def world(gpu_ctx, tmp_path_factory):
    from ucfp_amd import audio, store
    from ucfp_amd.index import GpuIndex
    xs = [pr.recording(i) for i in range(pr.N_RECORDINGS)]
    path = str(tmp_path_factory.mktemp("panako") / "side.log")
    gi = GpuIndex(gpu_ctx, sidecar=store.Sidecar(path))
    recs = [audio.fingerprint_panako(x, 8000, TENANT, rid) for x, rid in zip(xs, PANAKO_IDS)]
    wang = [audio.fingerprint_wang(xs[i], 8000, TENANT, rid) for i, rid in enumerate(WANG_IDS)]
    gi.upsert(recs[:5] + wang)
    gi.upsert(recs[5:])
    cases = []
    for i, x in enumerate(xs):
        for start_s, length_s in pr.EXCERPTS:
            q = audio.panako_hashes(pr.excerpt(x, start_s, length_s), 8000, ctx=gpu_ctx)
            cases.append((i, start_s, audio.panako_landmarks(q.tobytes())))
    assert len(cases) == 24
    return gi, path, xs, recs, wang, cases


def _tuples(hits):
    return [(h.record_id, h.votes, h.offset, np.float32(h.score).tobytes()) for h in hits]


def _ref_tuples(ref, q, k):
    return [(rid, v, d, np.float32(s).tobytes()) for rid, v, d, s in ref.query(q, k)]


def test_identifies_every_excerpt_and_matches_reference(gpu_ctx, world):
    from ucfp_amd import audio
    from ucfp_amd.core import HitSource, QueryRequest
    gi, _, _, recs, _, cases = world
    ref = LandmarkRef({r.record_id: audio.panako_landmarks(r.fingerprint) for r in recs})
    assert gi._pk.size(TENANT) == (len(recs), ref.postings)
    for i, start_s, lm in cases:
        hits = gi.identify(TENANT, lm, 5, algorithm=audio.ALGORITHM_PANAKO)
        want = _ref_tuples(ref, lm, 5)
        assert _tuples(hits) == want, (i, start_s)                              # (a)
        assert hits[0].record_id == 100 + i and hits[0].offset == int(start_s * pr.FRAMES_PER_S), (i, start_s, want[:2])  # (b)
        assert hits[0].source == HitSource.Landmark
        body = {"tenant_id": TENANT, "modality": "Audio", "k": 5, "landmarks": lm.tolist(),
                "algorithm": "audiofp-panako-v1"}
        assert _tuples(gi.query(QueryRequest.from_json(body))) == want, (i, start_s)
    assert gi.identify(TENANT, cases[0][2].tobytes(), 5, algorithm=audio.ALGORITHM_PANAKO)[0].record_id == 100
    assert gi.identify(9, cases[0][2], 5, algorithm=audio.ALGORITHM_PANAKO) == []


def test_wang_and_panako_never_share_postings(gpu_ctx, world):
    from ucfp_amd import audio
    from ucfp_amd.core import QueryRequest
    from ucfp_amd.errors import InvalidArgument
    gi, _, xs, _, wang, cases = world
    wref = LandmarkRef({r.record_id: r.fingerprint for r in wang})
    for i, start_s, lm in cases[:6]:
        body = {"tenant_id": TENANT, "modality": "Audio", "k": 10, "landmarks": lm.tolist()}
        hits = gi.query(QueryRequest.from_json(body))                           # (c) no `algorithm`: the Wang index
        assert _tuples(hits) == _ref_tuples(wref, lm, 10)
        assert all(h.record_id in WANG_IDS for h in hits)
        assert _tuples(gi.identify(TENANT, lm, 10)) == _tuples(hits)
    # a Wang excerpt of recording 0 finds the Wang record, and nothing in the Panako index
    w = audio.wang_hashes(pr.excerpt(xs[0], 4, 4.5), 8000, ctx=gpu_ctx)
    hits = gi.identify(TENANT, w, 3)
    assert hits[0].record_id == 200 and hits[0].offset == 250
    assert all(h.votes < hits[0].votes // 10 for h in gi.identify(TENANT, w, 3, algorithm=audio.ALGORITHM_PANAKO))
    with pytest.raises(InvalidArgument):
        gi.identify(TENANT, w, 3, algorithm="audiofp-haitsma-v1")


def test_mutations_delete_and_rebuild(gpu_ctx, world):
    """Runs last: it changes the index."""
    from ucfp_amd import audio, store
    gi, path, xs, recs, wang, cases = world
    P = audio.ALGORITHM_PANAKO
    lm3 = next(lm for i, s, lm in cases if i == 3 and s == 4)
    assert gi.identify(TENANT, lm3, 1, algorithm=P)[0].record_id == 103
    n_pk, n_lm = gi._pk.size(TENANT)[0], gi._lm.size(TENANT)[0]
    # (d) a Wang record under a Panako key leaves the Panako index ...
    gi.upsert([audio.fingerprint_wang(xs[3], 8000, TENANT, 103)])
    assert gi._pk.size(TENANT)[0] == n_pk - 1 and gi._lm.size(TENANT)[0] == n_lm + 1
    assert all(h.record_id != 103 for h in gi.identify(TENANT, lm3, 10, algorithm=P))
    w3 = audio.wang_hashes(pr.excerpt(xs[3], 4, 4.5), 8000, ctx=gpu_ctx)
    assert gi.identify(TENANT, w3, 1)[0].record_id == 103
    # ... and a Panako record under a Wang key leaves the Wang index
    gi.upsert([audio.fingerprint_panako(xs[1], 8000, TENANT, 201)])
    assert gi._pk.size(TENANT)[0] == n_pk and gi._lm.size(TENANT)[0] == n_lm
    w1 = audio.wang_hashes(pr.excerpt(xs[1], 4, 4.5), 8000, ctx=gpu_ctx)
    assert all(h.record_id != 201 for h in gi.identify(TENANT, w1, 10))
    lm1 = next(lm for i, s, lm in cases if i == 1 and s == 4)
    top = gi.identify(TENANT, lm1, 2, algorithm=P)
    assert [h.record_id for h in top] == [101, 201] and top[0].votes == top[1].votes and top[0].offset == 250
    # (e) delete reaches the Panako index; a rebuild from the sidecar answers like the index that wrote the log
    gi.delete(TENANT, [104])
    lm4 = next(lm for i, s, lm in cases if i == 4 and s == 10)
    assert all(h.record_id != 104 for h in gi.identify(TENANT, lm4, 10, algorithm=P))
    gi.flush()
    gi2 = store.rebuild(path, gpu_ctx)
    assert gi2._pk.size(TENANT) == gi._pk.size(TENANT) and gi2._lm.size(TENANT) == gi._lm.size(TENANT)
    for _, _, lm in cases:
        assert _tuples(gi2.identify(TENANT, lm, 10, algorithm=P)) == _tuples(gi.identify(TENANT, lm, 10, algorithm=P))
        assert _tuples(gi2.identify(TENANT, lm, 10)) == _tuples(gi.identify(TENANT, lm, 10))
    live = {r.record_id: audio.panako_landmarks(r.fingerprint) for r in recs if r.record_id not in (103, 104)}
    live[201] = live[101]
    ref = LandmarkRef(live)
    for _, _, lm in cases:
        assert _tuples(gi2.identify(TENANT, lm, 10, algorithm=P)) == _ref_tuples(ref, lm, 10)
