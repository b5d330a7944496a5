"""The Panako index with the (scale, offset) vote on the GPU: every answer is compared tuple for tuple
(id, votes, offset, scale, score bits) with tests/panako_match_ref.py -- random configurations, the spec's fixed corners
through the C ABI, both vote paths around ucfp_panako_index_lds_votes(), a hot hash, the limits, mutations, the device
entry points, two host threads, and identification of time-stretched excerpts end to end through a GpuIndex."""
import threading

import numpy as np
import pytest

import panako_match_ref as pm
import panako_ref as pr
from landmark_ref import LandmarkRef

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFFFFFFFFFF


def _check(got, q, want, k):
    """Row q of a query() result against the reference's hits."""
    ids, votes, offs, scales, scores, counts = got
    assert counts[q] == len(want), (q, int(counts[q]), len(want))
    for j, (rid, v, d, s, sc) in enumerate(want):
        assert (int(ids[q, j]), int(votes[q, j]), int(offs[q, j]), int(scales[q, j])) == (rid, v, d, s), (q, j, want[j])
        assert np.float32(scores[q, j]).tobytes() == np.float32(sc).tobytes(), (q, j)
    for j in range(len(want), k):
        assert (ids[q, j], votes[q, j], offs[q, j], scales[q, j], scores[q, j]) == (NONE, 0, 0, 0, -1.0), (q, j)


def _check_all(ix, tenant, ref, queries, k, min_votes=1, **match):
    got = ix.query(tenant, queries, k, min_votes, **match)
    for q, item in enumerate(queries):
        _check(got, q, ref.query(item, k, min_votes, **match), k)
    return got


def _corpus(rng, n_rec, max_triples, alphabet=1 << 12):
    """Records of (hash, a', d') with hashes from a skewed alphabet whose members have neighbours in r."""
    base = rng.integers(0, 1 << 27, alphabet // 4, dtype=np.int64) << 5
    alpha = np.concatenate([base | rng.integers(0, 32, base.size), base | 0, base | 1, base | 31])

    def draw(n):
        return alpha[(alpha.size * rng.random(n) ** 2).astype(np.int64)]

    def item(n, t_max=4000):
        a = rng.integers(0, t_max, n)
        return np.stack([draw(n), a, a, a + rng.integers(8, 200, n)], axis=1).astype(np.uint32)

    recs = {int(i): item(int(rng.integers(0, max_triples + 1)))
            for i in rng.choice(1 << 40, n_rec, replace=False)}
    return recs, item


def _stretched_cut(rng, rec, item, speed):
    """A cut of a record played at `speed`: t_a and d divided by it, r jittered, triples dropped, added and repeated."""
    r = rec.astype(np.int64)
    t0 = int(rng.integers(0, 3000))
    sel = r[(r[:, 1] >= t0) & (r[:, 1] < t0 + int(rng.integers(50, 400)))]
    sel = sel[rng.random(sel.shape[0]) < 0.8]
    a = np.round((sel[:, 1] - t0) / speed).astype(np.int64)
    d = np.maximum(1, np.round((sel[:, 3] - sel[:, 1]) / speed).astype(np.int64))
    h = sel[:, 0]
    jit = rng.random(h.size) < 0.2
    h = np.where(jit, (h & ~np.int64(31)) | np.clip((h & 31) + rng.integers(-1, 2, h.size), 0, 31), h)
    q = np.stack([h, a, a, a + d], axis=1).astype(np.uint32)
    q = np.concatenate([q, item(int(rng.integers(0, 40)), 1500), q[: q.shape[0] // 8]])
    return q[rng.permutation(q.shape[0])]


def _configuration(seed):
    """-> (max_postings, match, [(tenant, records, queries, k, min_votes)]): two tenants of <= 50 records of <= 2000
    triples, every match parameter drawn, a ragged batch of 2 ... 64 queries with an empty one and one of one triple."""
    rng = np.random.default_rng(2000 + seed)
    max_postings = int(rng.choice([0, 0, 40, 400]))
    smin = int(rng.integers(150, 257))
    nh = int(rng.integers(1, 65))
    step = int(rng.integers(1, 9))
    match = dict(scale_min=smin, scale_max=smin + (nh - 1) * step + int(rng.integers(0, step)), scale_step=step,
                 window=int(rng.choice([1, 4, 16, 64, 256])), slack=int(rng.choice([0, 1, 2, 2, 4, 8])),
                 r_slack=int(rng.integers(0, 2)))
    if seed == 0:
        match = dict(pm.DEFAULTS)
    lo, hi = match["scale_min"] / 256.0, match["scale_max"] / 256.0                                # speeds the hypotheses cover
    tenants = []
    for tenant in (3, 0xFFFFFFF0):
        recs, item = _corpus(rng, int(rng.integers(1, 51)), int(rng.choice([30, 300, 2000])), alphabet=1 << 10)
        keys = list(recs)
        qs = [_stretched_cut(rng, recs[keys[int(rng.integers(0, len(keys)))]], item, float(rng.uniform(lo, hi + 0.01)))
              for _ in range(int(rng.integers(0, 63)))]
        qs += [np.zeros((0, 4), np.uint32), item(1)]                                              # empty; one triple
        qs = [qs[i] for i in rng.permutation(len(qs))]
        tenants.append((tenant, recs, qs, int(rng.choice([1, 5, 128])), int(rng.choice([0, 1, 2, 5]))))
    return max_postings, match, tenants


@pytest.mark.parametrize("seed", range(20))
def test_random_configurations(gpu_ctx, seed):
    from ucfp_amd.index import PanakoIndex
    max_postings, match, tenants = _configuration(seed)
    ix = PanakoIndex(max_postings, ctx=gpu_ctx)
    for tenant, recs, qs, k, min_votes in tenants:
        keys = list(recs)
        half = len(keys) // 2
        ix.upsert(tenant, np.array(keys[:half], np.uint64), [recs[i] for i in keys[:half]])       # two upserts, one rebuild
        ix.upsert(tenant, np.array(keys[half:], np.uint64), [recs[i].tobytes() for i in keys[half:]])
    for tenant, recs, qs, k, min_votes in tenants:
        ref = pm.PanakoMatchRef(recs, max_postings)
        assert ix.size(tenant) == (len(recs), ref.postings)
        _check_all(ix, tenant, ref, qs, k, min_votes, **match)
        _check_all(ix, tenant, ref, qs[:1], k, min_votes, **match)                                # a batch of one
    ix.close()


def test_random_configurations_stand_on_both_sides_of_the_vote_limit():
    """Not vacuous: configurations 0, 3 and 10 alone hold five batches with queries below and above lds_votes()."""
    from ucfp_amd.index import PanakoIndex
    lds = PanakoIndex.lds_votes()
    mixed = 0
    for seed in (0, 3, 10):
        max_postings, match, tenants = _configuration(seed)
        for tenant, recs, qs, k, min_votes in tenants:
            ref = pm.PanakoMatchRef(recs, max_postings)
            v = np.array([ref.votes_total(q, **match) for q in qs])
            mixed += bool((v > lds).any() and ((v > 0) & (v <= lds)).any())
    assert mixed == 5


@pytest.mark.parametrize("case", pm.corners(), ids=lambda c: c[0])
def test_fixed_corners_through_the_c_abi(gpu_ctx, case):
    from ucfp_amd.index import PanakoIndex
    _, records, q, match, want = case
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(1, np.array(list(records), np.uint64), list(records.values()))
    ref = pm.PanakoMatchRef(records)
    assert ix.size(1) == (len(records), ref.postings)
    got = _check_all(ix, 1, ref, [q], 5, **match)
    if want is not None:
        assert [(int(got[0][0, j]), int(got[1][0, j]), int(got[2][0, j]), int(got[3][0, j])) for j in range(got[5][0])] == want
    ix.close()


def test_invalid_inputs_and_limits(gpu_ctx):
    from ucfp_amd import errors
    from ucfp_amd.index import PanakoIndex
    good = pm.rec((pm.H0, 1, 5))
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(1, [1], [good])
    for name, item, bad_record, bad_query in pm.invalid_items():
        for bad, run in ((bad_record, lambda: ix.upsert(1, [2], [item])), (bad_query, lambda: ix.query(1, [good, item], 3))):
            if bad:
                with pytest.raises(errors.InvalidArgument):
                    run()
            else:
                run()
        ix.delete(1, [2])
    assert ix.size(1) == (1, 1)
    for match in pm.INVALID_CONFIGS:
        with pytest.raises(errors.InvalidArgument):
            ix.query(1, [good], 3, **match)
    with pytest.raises(errors.InvalidArgument):
        ix.query(1, [good], 129)
    # 64 hypotheses are allowed, 65 are not
    ref = pm.PanakoMatchRef({1: good})
    _check_all(ix, 1, ref, [good], 3, scale_min=200, scale_max=263, scale_step=1)
    _check_all(ix, 1, ref, [good], 3, scale_min=64, scale_max=1024, scale_step=16, slack=8)      # 61 over the whole range
    with pytest.raises(errors.InvalidArgument):
        ix.query(1, [good], 3, scale_min=200, scale_max=264, scale_step=1)
    # unknown tenant, k = 0, empty query
    ids, votes, offs, scales, sc, n = ix.query(77, [good], 5)
    assert (n == 0).all() and (ids == NONE).all() and (sc == -1).all() and (scales == 0).all()
    assert (ix.query(1, [good], 0)[5] == 0).all()
    assert (ix.query(1, [b""], 5)[5] == 0).all()
    assert ix.size(77) == (0, 0)
    ix.close()


def test_records_per_tenant_cap(gpu_ctx):
    """A posting keeps 23 bits for the ordinal: 2^23 records rebuild, one more is UCFP_E_INVALID at the rebuild."""
    from ucfp_amd import errors
    from ucfp_amd.index import PanakoIndex
    ix = PanakoIndex(0, ctx=gpu_ctx)
    n = (1 << 23) + 1
    ids = np.arange(n, dtype=np.uint64)
    offs = np.zeros(n + 1, np.uint64)
    from ucfp_amd import _lib
    _lib.check(ix._lib.ucfp_panako_index_upsert(ix.handle, 1, ids.ctypes.data, None, offs.ctypes.data, n))
    with pytest.raises(errors.InvalidArgument):
        ix.size(1)
    assert ix.delete(1, [5]) == 1
    assert ix.size(1) == (1 << 23, 0)
    ix.close()


def test_both_vote_paths_around_the_limit(gpu_ctx):
    """One query built three times, with lds_votes() - 1, lds_votes() and lds_votes() + 1 expanded votes: postings with
    d' = 64 support all three hypotheses of a query triple with d = 64, postings with d' = 66 support one."""
    from ucfp_amd.index import PanakoIndex
    L = PanakoIndex.lds_votes()
    match = dict(scale_min=252, scale_max=260, scale_step=4, slack=1, window=16)
    rng = np.random.default_rng(77)
    p3 = (L - 200) // 3
    hashes = [(40 + i) << 5 for i in range(3)]
    rows = {rid: [] for rid in range(5)}
    for i, h in enumerate(hashes):
        p1 = L - 1 + i - 3 * p3
        for n, d in ((p3, 64), (p1, 66)):
            a = rng.choice(3000, n, replace=False)
            for x in a:
                rows[int(rng.integers(0, 5))].append((h, int(x), d))
    recs = {10 + rid: pm.rec(*r) for rid, r in rows.items()}
    qs = [pm.rec((h, 20, 64)) for h in hashes]
    ref = pm.PanakoMatchRef(recs)
    assert [ref.votes_total(q, **match) for q in qs] == [L - 1, L, L + 1]
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    for k in (1, 5):
        _check_all(ix, 0, ref, qs, k, **match)                    # one batch mixes the two paths
        for q in qs:
            _check_all(ix, 0, ref, [q], k, **match)
    ix.close()


def test_hot_hash_with_and_without_stop(gpu_ctx):
    """One hash with 50 000 postings in a single record, with and without a max_postings that stops it."""
    from ucfp_amd.index import PanakoIndex
    rng = np.random.default_rng(78)
    H = (0x155 << 23) | (0x0AA << 14) | (0x111 << 5) | 9
    a = rng.choice(1 << 20, 50000, replace=False)
    hot = np.stack([np.full(50000, H), a, a, a + rng.integers(1, 1024, 50000)], axis=1).astype(np.uint32)
    other = pm.rec(*[(H + 64 * i, 100 + 3 * i, 40 + i) for i in range(1, 60)])
    recs = {7: np.concatenate([hot, other]), 8: other[:30], 9: pm.rec((H, 5, 100), (H + 1, 9, 90))}
    qs = [pm.rec((H, 10, 80), (H, 400, 300), *[(H + 64 * i, 3 * i, 40 + i) for i in range(1, 40)]), pm.rec((H - 1, 0, 500))]
    for max_postings in (0, 1000):
        ref = pm.PanakoMatchRef(recs, max_postings)
        ix = PanakoIndex(max_postings, ctx=gpu_ctx)
        ix.upsert(5, np.array(list(recs), np.uint64), list(recs.values()))
        assert ix.size(5) == (3, ref.postings)
        assert (ref.votes_total(qs[0]) > PanakoIndex.lds_votes()) == (max_postings == 0)
        for k in (1, 128):
            _check_all(ix, 5, ref, qs, k)
        ix.close()


@pytest.fixture(scope="module")
def small(gpu_ctx):
    """200 short records over few hashes (more than UCFP_INDEX_MAX_K of them answer a query), and 40 queries."""
    rng = np.random.default_rng(79)
    recs, item = _corpus(rng, 200, 120, alphabet=256)
    keys = list(recs)
    qs = [_stretched_cut(rng, recs[keys[int(rng.integers(0, 200))]], item, float(rng.uniform(0.85, 1.2))) for _ in range(38)]
    qs += [np.zeros((0, 4), np.uint32), item(1)]
    return recs, qs, item


def test_k_min_votes_and_r_slack(gpu_ctx, small):
    from ucfp_amd.index import PanakoIndex
    recs, qs, _ = small
    ref = pm.PanakoMatchRef(recs)
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(2, np.array(list(recs), np.uint64), list(recs.values()))
    assert max(len(ref.query(q, 10 ** 6)) for q in qs) > 128          # k = UCFP_INDEX_MAX_K cuts something off
    top = max(h[1] for q in qs for h in ref.query(q, 1))
    differ = 0
    for k, min_votes in ((1, 1), (128, 1), (128, 3), (10, top + 1)):
        for r_slack in (0, 1):
            got = _check_all(ix, 2, ref, qs, k, min_votes, r_slack=r_slack)
            if min_votes == top + 1:
                assert (got[5] == 0).all() and (got[0] == NONE).all()
    for q in qs:
        differ += ref.query(q, 5, r_slack=0) != ref.query(q, 5, r_slack=1)
    assert differ >= 10
    ix.close()


def test_mutations(gpu_ctx, small):
    from ucfp_amd.index import PanakoIndex
    recs, qs, item = small
    recs = dict(list(recs.items())[:40])
    recs[41] = np.zeros((0, 4), np.uint32)
    keys = list(recs)
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(1, np.array(keys, np.uint64), list(recs.values()))
    ix.upsert(2, np.array([5], np.uint64), [recs[keys[7]]])                         # another tenant

    def agree(model, tenant=1):
        ref = pm.PanakoMatchRef(model)
        _check_all(ix, tenant, ref, qs[:12] + qs[-2:], 20)
        assert ix.size(tenant) == (len(model), ref.postings)

    agree(recs)
    agree({5: recs[keys[7]]}, 2)
    orig7 = recs[keys[7]]
    recs[keys[7]] = item(90)                                                        # upsert-replace
    ix.upsert(1, np.array([keys[7]], np.uint64), [recs[keys[7]].tobytes()])
    agree(recs)
    assert ix.delete(1, np.array([keys[3], 999], np.uint64)) == 1
    del recs[keys[3]]
    agree(recs)
    recs[keys[3]] = item(60)                                                        # re-upsert
    ix.upsert(1, np.array([keys[3]], np.uint64), [recs[keys[3]]])
    ix.flush()
    agree(recs)
    assert ix.delete(1, np.array([41], np.uint64)) == 1                             # the empty record counted
    del recs[41]
    agree(recs)
    agree({5: orig7}, 2)                                                            # tenant 2 untouched
    ix.close()


def test_dev_entry_points_on_a_side_stream(gpu_ctx, torch_cuda, small):
    from ucfp_amd.index import PanakoIndex, _pack_triplets
    torch = torch_cuda
    recs, qs, _ = small
    keys = list(recs)
    match = dict(window=8, slack=1)
    host, dev = PanakoIndex(30, ctx=gpu_ctx), PanakoIndex(30, ctx=gpu_ctx)
    host.upsert(0, np.array(keys, np.uint64), [recs[i] for i in keys])
    blob, offs = _pack_triplets([recs[i] for i in keys])
    side = torch.cuda.Stream()
    nq, k = len(qs), 10
    with torch.cuda.stream(side):
        d_ids = torch.from_numpy(np.array(keys, np.uint64).view(np.int64)).cuda()
        d_blob = torch.from_numpy(blob.copy()).cuda()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        dev.upsert_dev(0, d_ids.data_ptr(), d_blob.data_ptr(), d_offs.data_ptr(), len(keys), side.cuda_stream)
        assert dev.size(0) == host.size(0)
        qb, qo = _pack_triplets(qs)
        d_qb, d_qo = torch.from_numpy(qb.copy()).cuda(), torch.from_numpy(qo.view(np.int64)).cuda()
        o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        o_v = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        o_o = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        o_c = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
        dev.query_dev(0, d_qb.data_ptr(), d_qo.data_ptr(), nq, k, 2, o_ids.data_ptr(), o_v.data_ptr(), o_o.data_ptr(),
                      o_c.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), side.cuda_stream, **match)
    side.synchronize()
    h = host.query(0, qs, k, 2, **match)
    ref = pm.PanakoMatchRef(recs, 30)
    for q in range(nq):
        _check(h, q, ref.query(qs[q], k, 2, **match), k)
    assert np.array_equal(o_ids.cpu().numpy().view(np.uint64), h[0])
    assert np.array_equal(o_v.cpu().numpy().view(np.uint32), h[1])
    assert np.array_equal(o_o.cpu().numpy(), h[2])
    assert np.array_equal(o_c.cpu().numpy().view(np.uint32), h[3])
    assert np.array_equal(o_s.cpu().numpy().view(np.uint32), h[4].view(np.uint32))
    assert np.array_equal(o_n.cpu().numpy().view(np.uint32), h[5])
    host.close()
    dev.close()


def test_two_host_threads_query_one_index(gpu_ctx, small):
    from ucfp_amd.index import PanakoIndex
    recs, qs, _ = small
    ref = pm.PanakoMatchRef(recs)
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    want = {r_slack: [ref.query(q, 7, r_slack=r_slack) for q in qs] for r_slack in (0, 1)}
    errs = []

    def work(r_slack):
        try:
            for rep in range(6):
                sub = slice(rep, len(qs), 2)
                got = ix.query(0, qs[sub], 7, r_slack=r_slack)
                for q, w in enumerate(want[r_slack][sub]):
                    _check(got, q, w, 7)
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errs.append(e)

    threads = [threading.Thread(target=work, args=(r,)) for r in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    ix.close()


# ---------------------------------------------------------------- end to end, from audio

TENANT = 1
IDS = [100 + i for i in range(pm.N_RECORDINGS)]


def _hits(hits):
    return [(h.record_id, h.votes, h.offset, h.scale, np.float32(h.score).tobytes()) for h in hits]


def _ref_hits(ref, q, k):
    return [(rid, v, d, s / 256.0, np.float32(sc).tobytes()) for rid, v, d, s, sc in ref.query(q, k)]


def test_stretched_excerpts_end_to_end(gpu_ctx, tmp_path):
    """The recordings of the spec test through audio.fingerprint_panako into a GpuIndex with a sidecar; the excerpt
    [4 s, 12 s) of recording 3 at seven speeds, fingerprinted on the device, finds it at rank 1 through
    identify_stretched and through a `triplets` query body; the hits equal the reference's, survive store.rebuild, and
    identify(algorithm=ALGORITHM_PANAKO) over the same index still equals LandmarkRef."""
    from ucfp_amd import audio, store
    from ucfp_amd.core import HitSource, QueryRequest, hit_to_json
    from ucfp_amd.index import GpuIndex
    path = str(tmp_path / "side.log")
    gi = GpuIndex(gpu_ctx, sidecar=store.Sidecar(path))
    recs = [audio.fingerprint_panako(pm.recording(i), 8000, TENANT, rid) for i, rid in enumerate(IDS)]
    gi.upsert(recs[:5] + [audio.fingerprint_wang(pm.recording(0), 8000, TENANT, 200)])
    gi.upsert(recs[5:])
    ref = pm.PanakoMatchRef({r.record_id: bytes(r.fingerprint) for r in recs})
    a10 = LandmarkRef({r.record_id: audio.panako_landmarks(r.fingerprint) for r in recs})
    assert gi._ps.size(TENANT) == (len(recs), ref.postings)
    assert gi.identify_stretched(TENANT, b"", 5) == [] and gi.identify_stretched(9, recs[0].fingerprint, 5) == []
    cases = []
    for speed in pm.SPEEDS:
        q = audio.panako_hashes(pm.stretched_excerpt(3, speed), 8000, ctx=gpu_ctx)
        cases.append((speed, q))
        hits = gi.identify_stretched(TENANT, q, 5)
        want = _ref_hits(ref, q, 5)
        assert _hits(hits) == want, speed
        assert hits[0].record_id == 103 and hits[0].source == HitSource.Landmark
        assert abs(hits[0].offset - 250) <= 16 and abs(hits[0].scale * 256 - 256 * speed) <= 12, (speed, want[0])
        assert all(h.votes * 3 <= hits[0].votes for h in hits[1:])
        assert hit_to_json(hits[0])["scale"] == hits[0].scale
        body = {"tenant_id": TENANT, "modality": "Audio", "k": 5, "triplets": q.tolist(), "algorithm": "audiofp-panako-v1"}
        assert _hits(gi.query(QueryRequest.from_json(body))) == want, speed
        assert _hits(gi.identify_stretched(TENANT, q.tobytes(), 5, r_slack=0, window=8)) == [
            (rid, v, d, s / 256.0, np.float32(sc).tobytes()) for rid, v, d, s, sc in ref.query(q, 5, r_slack=0, window=8)]
        # nothing existing moved: the A10 projection index answers as before, without a scale
        lm = audio.panako_landmarks(q.tobytes())
        old = gi.identify(TENANT, lm, 5, algorithm=audio.ALGORITHM_PANAKO)
        assert [(h.record_id, h.votes, h.offset, np.float32(h.score).tobytes()) for h in old] == [
            (rid, v, d, np.float32(s).tobytes()) for rid, v, d, s in a10.query(lm, 5)]
        assert all(h.scale is None and "scale" not in hit_to_json(h) for h in old)
    # a Wang record under a Panako key leaves both Panako indexes; delete reaches them; rebuild answers the same
    gi.upsert([audio.fingerprint_wang(pm.recording(6), 8000, TENANT, 106)])
    gi.delete(TENANT, [105])
    assert gi._ps.size(TENANT)[0] == len(recs) - 2 and gi._pk.size(TENANT)[0] == len(recs) - 2
    gi.flush()
    gi2 = store.rebuild(path, gpu_ctx)
    assert gi2._ps.size(TENANT) == gi._ps.size(TENANT)
    live = pm.PanakoMatchRef({r.record_id: bytes(r.fingerprint) for r in recs if r.record_id not in (105, 106)})
    for speed, q in cases:
        assert _hits(gi2.identify_stretched(TENANT, q, 8)) == _hits(gi.identify_stretched(TENANT, q, 8)) == _ref_hits(live, q, 8)
        lm = audio.panako_landmarks(q.tobytes())
        assert ([(h.record_id, h.votes, h.offset) for h in gi2.identify(TENANT, lm, 8, algorithm=audio.ALGORITHM_PANAKO)]
                == [(h.record_id, h.votes, h.offset) for h in gi.identify(TENANT, lm, 8, algorithm=audio.ALGORITHM_PANAKO)])
