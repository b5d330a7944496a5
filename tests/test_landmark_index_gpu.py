"""Landmark index on the device: every id, vote count, offset, score and hit count equals the numpy
reference (tests/landmark_ref.py), on both vote paths (LDS tables and the global spill); mutations and errors; the
device entry points; and end-to-end identification of noisy cuts and of a live stream from Wang fingerprints."""
import ctypes as C

import numpy as np
import pytest

from landmark_ref import LandmarkRef

pytestmark = pytest.mark.gpu

UCFP_E_INVALID = -4
LDS_VOTES = 3072          # lm_vote keeps a query with at most this many votes in LDS; more spill (DESIGN A10)


def _lib():
    from ucfp_amd import _lib as L
    return L


def _check_hits(got, ref_hits, q, k):
    ids, votes, offs, scores, counts = got
    assert counts[q] == len(ref_hits), (q, counts[q], len(ref_hits))
    for j, (rid, v, d, s) in enumerate(ref_hits):
        assert (int(ids[q, j]), int(votes[q, j]), int(offs[q, j])) == (rid, v, d), (q, j)
        assert scores[q, j] == np.float32(s), (q, j)
    for j in range(len(ref_hits), k):
        assert ids[q, j] == 0xFFFFFFFFFFFFFFFF


def _corpus(seed, nrec=2000, alphabet=1 << 16):
    """Hashes from a skewed small alphabet (density ~ 1/sqrt(rank)), so runs are long and ties common."""
    rng = np.random.default_rng(seed)
    alpha = rng.integers(0, 2**32, alphabet, dtype=np.uint64).astype(np.uint32)
    alpha[1::5] = (alpha[1::5] & 0xFFFFC000) | (alpha[::5][: alpha[1::5].size] & 0x3FFF)   # shared directory buckets
    def draw(n):
        return alpha[(alphabet * rng.random(n) ** 2).astype(np.int64)]
    recs = {}
    ids = rng.choice(1 << 40, nrec, replace=False).astype(np.uint64)
    for rid in ids.tolist():
        n = int(rng.integers(0, 3001))
        recs[rid] = np.stack([draw(n), rng.integers(0, 20000, n).astype(np.uint32)], 1)
    return rng, recs, draw


def _queries(rng, recs, draw, nq):
    """Cuts of records at known offsets (t shifted by -t0), some landmarks dropped, random ones added, some duplicated."""
    keys = list(recs)
    out = []
    for i in range(nq):
        r = recs[keys[int(rng.integers(0, len(keys)))]]
        t0 = int(rng.integers(0, 18000))
        sel = r[(r[:, 1] >= t0) & (r[:, 1] < t0 + int(rng.integers(50, 1500)))]
        sel = sel[rng.random(sel.shape[0]) < 0.7].copy()
        sel[:, 1] -= t0
        n_noise = int(rng.integers(0, 60))
        noise = np.stack([draw(n_noise), rng.integers(0, 1500, n_noise).astype(np.uint32)], 1)
        q = np.concatenate([sel, noise, sel[: sel.shape[0] // 8]])
        out.append(q[rng.permutation(q.shape[0])] if i % 3 else q)
    out[0] = np.zeros((0, 2), np.uint32)   # an empty query
    return out


@pytest.fixture(scope="module")
def corpus(gpu_ctx):
    rng, recs, draw = _corpus(11)
    return rng, recs, draw, _queries(rng, recs, draw, 300)


@pytest.mark.parametrize("max_postings", [0, 50])
def test_random_corpus_matches_reference(gpu_ctx, corpus, max_postings):
    from ucfp_amd.index import LandmarkIndex
    rng, recs, draw, queries = corpus
    ref = LandmarkRef(recs, max_postings)
    ix = LandmarkIndex(max_postings, ctx=gpu_ctx)
    keys = list(recs)
    ix.upsert(4, np.array(keys[:1000], np.uint64), [recs[i] for i in keys[:1000]])    # two upserts, one rebuild
    ix.upsert(4, np.array(keys[1000:], np.uint64), [recs[i] for i in keys[1000:]])
    assert ix.size(4) == (len(recs), ref.postings)
    v = np.array([ref.votes_total(q) for q in queries])
    assert (v > LDS_VOTES).any() and ((v > 0) & (v <= LDS_VOTES)).any()   # both vote paths run
    for min_votes in (1, 3):
        full = [ref.query(q, 128, min_votes) for q in queries]
        for nq, k in ((300, 128), (300, 10), (64, 1), (7, 10), (1, 128)):
            sub = queries[:nq] if nq != 1 else queries[5:6]
            exp = full[:nq] if nq != 1 else full[5:6]
            got = ix.query(4, sub, k, min_votes)
            for q in range(len(sub)):
                _check_hits(got, exp[q][:k], q, k)
    ix.close()


def test_hot_hash_and_long_query_spill(gpu_ctx):
    """One hash with 1 M postings (max_postings = 0) and a query of 60 k landmarks: millions of votes per query."""
    from ucfp_amd.index import LandmarkIndex
    rng = np.random.default_rng(5)
    H = 0xDEADBEEF
    recs = {}
    for r in range(1000):
        t = rng.choice(100000, 1000, replace=False).astype(np.uint32)
        other = np.stack([rng.integers(0, 2**32, 200, dtype=np.uint64).astype(np.uint32),
                          rng.integers(0, 100000, 200).astype(np.uint32)], 1)
        recs[7 * r + 3] = np.concatenate([np.stack([np.full(1000, H, np.uint32), t], 1), other])
    own = recs[3][1000:]                                                           # record 3's other landmarks
    big = np.concatenate([np.stack([own[:, 0], own[:, 1] + 17], 1), np.array([[H, 1], [H, 2], [H, 3]], np.uint32),
                          np.stack([rng.integers(0, 2**32, 60000, dtype=np.uint64).astype(np.uint32),
                                    rng.integers(0, 100000, 60000).astype(np.uint32)], 1)])
    queries = [np.array([[H, 50], [H, 77], [H, 5000]], np.uint32), big, recs[3][1000:1100]]
    ref = LandmarkRef(recs, 0)
    assert ref.hashes[ref.hashes == H].size == 1_000_000
    assert ref.votes_total(queries[1]) > 2_000_000
    ix = LandmarkIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    for k in (1, 128):
        got = ix.query(0, queries, k)
        for q in range(len(queries)):
            _check_hits(got, ref.query(queries[q], k), q, k)
    assert got[0][1, 0] == 3 and got[2][1, 0] == -17 and got[0][2, 0] == 3 and got[2][2, 0] == 0
    ix.close()


def test_mutations_and_errors(gpu_ctx):
    from ucfp_amd import errors
    from ucfp_amd.index import LandmarkIndex
    rng = np.random.default_rng(2)
    mk = lambda n: np.stack([rng.integers(0, 64, n).astype(np.uint32), rng.integers(0, 500, n).astype(np.uint32)], 1)  # noqa
    recs = {i: mk(int(rng.integers(0, 200))) for i in range(40)}
    recs[41] = np.zeros((0, 2), np.uint32)
    ix = LandmarkIndex(0, ctx=gpu_ctx)
    ix.upsert(1, np.array(list(recs), np.uint64), list(recs.values()))
    ix.upsert(2, np.array([5], np.uint64), [recs[7]])                              # another tenant
    qs = [recs[7][:30], mk(50), recs[3][10:90].copy()]

    def agree(model, tenant=1):
        ref = LandmarkRef(model)
        got = ix.query(tenant, qs, 20)
        for q in range(len(qs)):
            _check_hits(got, ref.query(qs[q], 20), q, 20)
        assert ix.size(tenant) == (len(model), ref.postings)

    agree(recs)
    agree({5: recs[7]}, 2)
    orig7 = recs[7]
    recs[7] = mk(120)                                                              # upsert-replace
    ix.upsert(1, np.array([7], np.uint64), [recs[7].tobytes()])
    agree(recs)
    assert ix.delete(1, np.array([3, 999], np.uint64)) == 1
    del recs[3]
    agree(recs)
    recs[3] = mk(60)                                                               # re-upsert
    ix.upsert(1, np.array([3], np.uint64), [recs[3]])
    ix.flush()
    agree(recs)
    agree({5: orig7}, 2)                                                           # tenant 2 untouched
    # unknown tenant, k = 0, empty query
    ids, votes, offs, sc, n = ix.query(77, qs, 5)
    assert (n == 0).all() and (ids == 0xFFFFFFFFFFFFFFFF).all()
    assert (ix.query(1, qs, 0)[4] == 0).all()
    assert (ix.query(1, [b""], 5)[4] == 0).all()
    assert ix.size(77) == (0, 0)
    # errors
    bad_t = np.array([[1, 1 << 31]], np.uint32)
    for call in (lambda: ix.upsert(1, [9], [bad_t]), lambda: ix.query(1, [bad_t], 5),
                 lambda: ix.upsert(1, [9], [b"\0" * 12]), lambda: ix.query(1, [b"\0" * 12], 5),
                 lambda: ix.query(1, qs, 129)):
        with pytest.raises(errors.InvalidArgument):
            call()
    agree(recs)                                                                    # nothing changed
    ix.close()


def test_dev_entry_points_match_host(gpu_ctx, torch_cuda, corpus):
    from ucfp_amd.index import LandmarkIndex, _pack_landmarks
    torch = torch_cuda
    rng, recs, draw, queries = corpus
    keys = list(recs)[:300]
    host, dev = LandmarkIndex(50, ctx=gpu_ctx), LandmarkIndex(50, ctx=gpu_ctx)
    host.upsert(0, np.array(keys, np.uint64), [recs[i] for i in keys])
    blob, offs = _pack_landmarks([recs[i] for i in keys])
    st = torch.cuda.current_stream().cuda_stream
    d_ids = torch.from_numpy(np.array(keys, np.uint64).view(np.int64)).cuda()
    d_blob = torch.from_numpy(blob.copy()).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    dev.upsert_dev(0, d_ids.data_ptr(), d_blob.data_ptr(), d_offs.data_ptr(), len(keys), st)
    assert dev.size(0) == host.size(0)
    qs = queries[:64]
    qb, qo = _pack_landmarks(qs)
    d_qb, d_qo = torch.from_numpy(qb.copy()).cuda(), torch.from_numpy(qo.view(np.int64)).cuda()
    k = 10
    o_ids = torch.zeros((64, k), dtype=torch.int64, device="cuda")
    o_v = torch.zeros((64, k), dtype=torch.int32, device="cuda")
    o_o = torch.zeros((64, k), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((64, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(64, dtype=torch.int32, device="cuda")
    dev.query_dev(0, d_qb.data_ptr(), d_qo.data_ptr(), 64, k, 2, o_ids.data_ptr(), o_v.data_ptr(), o_o.data_ptr(),
                  o_s.data_ptr(), o_n.data_ptr(), st)
    torch.cuda.synchronize()
    h = host.query(0, qs, k, 2)
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint64), h[0])
    assert np.array_equal(o_v.cpu().numpy().view(np.uint32), h[1])
    assert np.array_equal(o_o.cpu().numpy(), h[2])
    assert np.array_equal(o_s.cpu().numpy(), h[3])
    assert np.array_equal(o_n.cpu().numpy().view(np.uint32), h[4])
    host.close()
    dev.close()


# ---------------------------------------------------------------- end to end, from Wang fingerprints

SR, HOP = 8000, 128
SNR_DB = 10.0             # noise added to every cut and to the live stream


def _track(i, seconds=30):
    """Seeded synthetic track: notes of 300 .. 1000 samples, three random tones each, plus a little noise (short notes
    of random length, so that the time alignment of a cut is unambiguous)."""
    rng = np.random.default_rng(1000 + i)
    n = seconds * SR
    lens = rng.integers(300, 1001, n // 300 + 1)
    idx = np.repeat(np.arange(lens.size), lens)[:n]
    f = rng.uniform(150.0, 3500.0, (3, lens.size))[:, idx]
    amp = rng.uniform(0.1, 0.3, (3, lens.size))[:, idx]
    x = (amp * np.sin(2 * np.pi * np.cumsum(f, 1) / SR)).sum(0)
    return (x + 0.01 * rng.standard_normal(n)).astype(np.float32)


def _noisy(x, rng):
    p = float(np.mean(x.astype(np.float64) ** 2))
    return (x + np.sqrt(p / 10 ** (SNR_DB / 10)) * rng.standard_normal(x.size)).astype(np.float32)


@pytest.fixture(scope="module")
def tracks(gpu_ctx):
    from ucfp_amd import audio
    xs = [_track(i) for i in range(200)]
    fps = audio.wang_hashes_batch(xs, SR, ctx=gpu_ctx)   # ucfp_audio_wang_batch_dev
    return xs, fps


def _check_identified(got, q, track_id, m):
    ids, votes, offs, _, n = got
    assert n[q] >= 1 and int(ids[q, 0]) == track_id and int(offs[q, 0]) == m, (q, ids[q, :3], offs[q, :3], track_id, m)
    if n[q] > 1:
        assert votes[q, 0] >= 3 * votes[q, 1], (q, votes[q, :3])


def test_identify_noisy_cuts(gpu_ctx, tracks):
    from ucfp_amd import audio
    from ucfp_amd.index import LandmarkIndex
    xs, fps = tracks
    ix = LandmarkIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.arange(200, dtype=np.uint64) + 500, fps)
    rng = np.random.default_rng(3)
    cuts, truth = [], []
    for j in range(40):
        i = int(rng.integers(0, 200))
        m = int(rng.integers(0, (25 * SR) // HOP))
        cuts.append(_noisy(xs[i][HOP * m: HOP * m + 5 * SR], rng))
        truth.append((500 + i, m))
    got = ix.query(0, audio.wang_hashes_batch(cuts, SR, ctx=gpu_ctx), 5)
    for q, (tid, m) in enumerate(truth):
        _check_identified(got, q, tid, m)
    ix.close()


def test_identify_live_stream(gpu_ctx, tracks):
    from ucfp_amd import audio
    from ucfp_amd.index import LandmarkIndex
    xs, fps = tracks
    ix = LandmarkIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.arange(200, dtype=np.uint64), fps)
    ws = audio.WangStreams(4, ctx=gpu_ctx)
    rng = np.random.default_rng(4)
    i, m0 = 17, 1234                       # the stream opens 1234 hops into track 17
    x = _noisy(xs[i][HOP * m0:], rng)
    slot = ws.open()
    got, n = [], 0
    while ws.frontier(n) < 5 * SR // HOP:  # until 5 s of frames have been emitted
        got.append(ws.push({slot: x[n:n + SR // 2]})[slot])
        n += SR // 2
    assert n < 8 * SR
    res = ix.query(0, [np.concatenate(got)], 3)
    _check_identified(res, 0, i, m0)
    ws.close(slot)
    ws.destroy()
    ix.close()


def test_gpu_index_route_and_rebuild(gpu_ctx, tracks, tmp_path):
    from ucfp_amd import audio, store
    from ucfp_amd.core import HitSource, Modality, QueryRequest, Record
    from ucfp_amd.index import GpuIndex
    xs, _ = tracks
    path = str(tmp_path / "side.log")
    gi = GpuIndex(gpu_ctx, sidecar=store.Sidecar(path))
    recs = [audio.fingerprint_wang(xs[i], SR, 2, 100 + i) for i in range(12)]
    gi.upsert(recs)
    rng = np.random.default_rng(8)
    cut = audio.wang_hashes(_noisy(xs[5][HOP * 300: HOP * 300 + 5 * SR], rng), SR)
    body = {"tenant_id": 2, "modality": "Audio", "k": 3, "landmarks": cut.tolist()}
    hits = gi.query(QueryRequest.from_json(body))
    assert hits and hits[0].record_id == 105 and hits[0].offset == 300 and hits[0].source == HitSource.Landmark
    assert hits[0].votes >= 3 * (hits[1].votes if len(hits) > 1 else 0) and 0 < hits[0].score <= 1
    assert gi.identify(2, cut.tobytes(), 3)[0].record_id == 105
    assert gi.identify(9, cut.tobytes(), 3) == [] and gi.identify(2, cut, 0) == []
    # re-ingesting 105 as an image record removes its landmarks
    gi.upsert([Record(tenant_id=2, record_id=105, modality=Modality.Image, format_version=1,
                      algorithm="imgfprint-ahash-v1", config_hash=0, fingerprint=bytes(168))])
    after = gi.query(QueryRequest.from_json(body))
    assert all(h.record_id != 105 for h in after)
    gi.delete(2, [104])
    gi.flush()
    want = [(h.record_id, h.score, h.votes, h.offset) for h in gi.identify(2, cut, 10)]
    probe = audio.wang_hashes(xs[3][HOP * 50: HOP * 50 + 5 * SR], SR)
    want3 = [(h.record_id, h.score, h.votes, h.offset) for h in gi.identify(2, probe, 10)]
    assert want3[0][0] == 103 and want3[0][3] == 50
    gi2 = store.rebuild(path, gpu_ctx)
    assert [(h.record_id, h.score, h.votes, h.offset) for h in gi2.identify(2, cut, 10)] == want
    assert [(h.record_id, h.score, h.votes, h.offset) for h in gi2.identify(2, probe, 10)] == want3
    assert gi2._lm.size(2) == gi._lm.size(2) and gi2._lm.size(2)[0] == 10
