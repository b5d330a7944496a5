"""The Panako index with the bins following the scale on the GPU: every answer is compared tuple for
tuple (id, votes, offset, scale, score bits) with tests/panako_pitch_ref.py -- random configurations over both modes, the
spec's fixed corners through the C ABI, the new entry with bins = 0 against the old entry byte for byte, both vote
paths around ucfp_panako_index_lds_votes(), a hot hash beside a live one, the invalid configurations, the device entry
on a side stream, two host threads, a live window, and resampled excerpts end to end through a GpuIndex."""
import ctypes as C
import threading

import numpy as np
import pytest

import panako_match_ref as pm
import panako_pitch_ref as pp

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFFFFFFFFFF
BINS = {0: "kept", 1: "scaled"}


def _py(match):
    """Reference keywords -> keywords of ucfp_amd.index (bins by name; every default spelled out)."""
    m = {**pm.DEFAULTS, "f_slack": 0, **match}
    m["bins"] = BINS[m.get("bins", 0)]
    return m


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
    got = ix.query(tenant, queries, k, min_votes, **_py(match))
    for q, item in enumerate(queries):
        _check(got, q, ref.query(item, k, min_votes, **match), k)
    return got


def _hash(k, r):
    return (k[:, 0] << 23) | (k[:, 1] << 14) | (k[:, 2] << 5) | r


def _corpus(rng, n_rec, max_triples):
    """Records whose bins come from 48 base triples (two of them at the ends of the bin range) with +-2 of jitter, so
    buckets are shared and their neighbours are populated."""
    base = rng.integers(3, 509, (48, 3))
    base[0], base[1] = [0, 1, 2], [511, 510, 508]

    def item(n, t_max=1500):
        k = np.clip(base[rng.integers(0, 48, n)] + rng.integers(-2, 3, (n, 3)) * (rng.random((n, 3)) < 0.5), 0, 511)
        a = rng.integers(0, t_max, n)
        return np.stack([_hash(k, rng.integers(0, 4, n)), a, a, a + rng.integers(8, 200, n)], axis=1).astype(np.uint32)

    recs = {int(i): item(int(rng.integers(0, max_triples + 1))) for i in rng.choice(1 << 40, n_rec, replace=False)}
    return recs, item


def _resampled_cut(rng, rec, item, s, scaled):
    """A cut of a record played at s / 256: t_a and d divided by it and, when `scaled`, the bins multiplied by it with +-2
    bins of jitter (record bin = B_s(query bin)); r jittered; triples dropped, noise added, some repeated."""
    r = rec.astype(np.int64)
    t0 = int(rng.integers(0, 1000))
    sel = r[(r[:, 1] >= t0) & (r[:, 1] < t0 + int(rng.integers(200, 1500)))]
    sel = sel[rng.permutation(sel.shape[0])[:int(rng.integers(40, 220))]]
    a = (sel[:, 1] - t0) * 256 // s
    d = np.maximum(1, ((sel[:, 3] - sel[:, 1]) * 256 + s // 2) // s)
    k = np.stack([(sel[:, 0] >> 23) & 511, (sel[:, 0] >> 14) & 511, (sel[:, 0] >> 5) & 511], axis=1)
    if scaled:
        k = np.clip((k * s + 128) // 256 + rng.integers(-2, 3, k.shape) * (rng.random(k.shape) < 0.3), 0, 511)
    rr = np.clip((sel[:, 0] & 31) + rng.integers(-1, 2, sel.shape[0]) * (rng.random(sel.shape[0]) < 0.2), 0, 31)
    q = np.stack([_hash(k, rr), a, a, a + d], axis=1).astype(np.uint32)
    q = np.concatenate([q, item(int(rng.integers(0, 40)), 800), q[: q.shape[0] // 8]])
    return q[rng.permutation(q.shape[0])]


def _configuration(seed):
    """-> (max_postings, match, [(tenant, records, queries, k, min_votes)]): two tenants of <= 60 records of <= 400
    triples, every match parameter drawn (both modes, f_slack 0 ... 3, step 1 ... 8), a ragged batch of <= 8 queries of
    <= 300 triples with an empty one and one of one triple."""
    rng = np.random.default_rng(2760 + seed)
    bins = int(seed % 5 != 4)
    max_postings = int(rng.choice([0, 0, 60, 250]))
    smin = int(rng.integers(150, 257))
    nh = int(rng.integers(2, 65))
    step = 1 + seed % 8
    match = dict(scale_min=smin, scale_max=smin + (nh - 1) * step + int(rng.integers(0, step)), scale_step=step,
                 window=int(rng.choice([1, 4, 16, 64, 256])), slack=int(rng.choice([0, 1, 2, 2, 4, 8])),
                 r_slack=int(rng.integers(0, 2)), bins=bins, f_slack=seed % 4 if bins else 0)
    if seed == 0:
        match = dict(pm.DEFAULTS, bins=1, **pp.SCALED_DEFAULTS)
    tenants = []
    for tenant in (3, 0xFFFFFFF0):
        recs, item = _corpus(rng, int(rng.integers(1, 61)), int(rng.choice([40, 400])))
        keys = list(recs)
        qs = [_resampled_cut(rng, recs[keys[int(rng.integers(0, len(keys)))]], item,
                             int(rng.integers(match["scale_min"], match["scale_max"] + 1)), bins)
              for _ in range(int(rng.integers(1, 7)))]
        qs += [np.zeros((0, 4), np.uint32), item(1)]
        qs = [qs[i] for i in rng.permutation(len(qs))]
        tenants.append((tenant, recs, qs, int(rng.choice([1, 5, 128])), int(rng.choice([0, 1, 2, 3]))))
    return max_postings, match, tenants


@pytest.mark.parametrize("seed", range(20))
def test_random_configurations(gpu_ctx, seed):
    from ucfp_amd.index import PanakoIndex
    max_postings, match, tenants = _configuration(seed)
    ix = PanakoIndex(max_postings, ctx=gpu_ctx)
    for tenant, recs, qs, k, min_votes in tenants:
        ix.upsert(tenant, np.array(list(recs), np.uint64), list(recs.values()))
    answered = 0
    for tenant, recs, qs, k, min_votes in tenants:
        ref = pp.PanakoPitchRef(recs, max_postings)
        assert ix.size(tenant) == (len(recs), ref.postings)
        got = _check_all(ix, tenant, ref, qs, k, min_votes, **match)
        _check_all(ix, tenant, ref, qs[:1], k, min_votes, **match)                                # a batch of one
        answered += int(got[5].sum())
    assert answered > 0, match                                                                    # not vacuous
    ix.close()


@pytest.mark.parametrize("case", pp.corners(), ids=lambda c: c[0])
def test_fixed_corners_through_the_c_abi(gpu_ctx, case):
    from ucfp_amd.index import PanakoIndex
    _, records, q, kw, want = case
    kw = dict(kw)
    max_postings = kw.pop("max_postings", 0)
    ix = PanakoIndex(max_postings, ctx=gpu_ctx)
    ix.upsert(1, np.array(list(records), np.uint64), list(records.values()))
    ref = pp.PanakoPitchRef(records, max_postings)
    got = _check_all(ix, 1, ref, [q], 5, **kw)
    if want is not None:
        assert [(int(got[0][0, j]), int(got[1][0, j]), int(got[2][0, j]), int(got[3][0, j])) for j in range(got[5][0])] == want
    ix.close()


@pytest.fixture(scope="module")
def small(gpu_ctx):
    """120 records of <= 100 triples and 10 queries played at scales 204 ... 320, with an empty one and one of one triple."""
    rng = np.random.default_rng(2790)
    recs, item = _corpus(rng, 120, 100)
    keys = list(recs)
    qs = [_resampled_cut(rng, recs[keys[int(rng.integers(0, len(keys)))]], item, int(rng.integers(204, 321)), True)
          for _ in range(8)]
    qs += [np.zeros((0, 4), np.uint32), item(1)]
    return recs, qs


def _raw_query(lib, entry, cfg, ix, tenant, blob, offs, nq, k, min_votes):
    """One call of a C query entry -> the bytes of its six outputs, which start as 0xA5."""
    outs = [np.full(nq * k * w, 0xA5, np.uint8) for w in (8, 4, 4, 4, 4)] + [np.full(nq * 4, 0xA5, np.uint8)]
    rc = getattr(lib, entry)(ix.handle, tenant, blob.ctypes.data, offs.ctypes.data, nq, k, min_votes,
                             C.byref(cfg) if cfg is not None else None, *[o.ctypes.data for o in outs])
    return rc, b"".join(o.tobytes() for o in outs)


def test_new_entry_with_kept_bins_is_the_old_entry(gpu_ctx, small):
    from ucfp_amd import _lib
    from ucfp_amd.index import PanakoIndex, _pack_triplets
    recs, qs = small
    lib = _lib.load()
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(4, np.array(list(recs), np.uint64), list(recs.values()))
    # kept-mode queries: the stored bins as they are
    rng = np.random.default_rng(2791)
    keys = list(recs)
    kept = [_resampled_cut(rng, recs[keys[i]], lambda n, t=0: np.zeros((0, 4), np.uint32), 240, False) for i in range(6)] + qs[-2:]
    blob, offs = _pack_triplets(kept)
    nonempty = 0
    for fields in ((204, 320, 4, 16, 2, 1), (230, 250, 1, 64, 4, 0), None):
        old_cfg = _lib.PanakoMatchConfig(*fields) if fields else None
        new_cfg = _lib.PanakoMatchConfigEx(*fields, 0, 0) if fields else None
        for k in (1, 7):
            rc_old, old = _raw_query(lib, "ucfp_panako_index_query", old_cfg, ix, 4, blob, offs, len(kept), k, 1)
            rc_new, new = _raw_query(lib, "ucfp_panako_index_query_ex", new_cfg, ix, 4, blob, offs, len(kept), k, 1)
            assert rc_old == rc_new == 0 and old == new
            nonempty += int(np.frombuffer(new[-4 * len(kept):], np.uint32).sum())
    assert nonempty >= 20
    assert C.sizeof(_lib.PanakoMatchConfig) == 24 and C.sizeof(_lib.PanakoMatchConfigEx) == 32
    ix.close()


def test_invalid_configurations(gpu_ctx):
    from ucfp_amd import _lib, errors
    from ucfp_amd.index import PanakoIndex, _pack_triplets, panako_match_config
    good = pm.rec((pm.H0, 1, 5))
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(1, [1], [good])
    blob, offs = _pack_triplets([good])
    lib = _lib.load()
    for bins, f_slack in ((2, 0), (1, 4), (0, 1), (0xFFFFFFFF, 0), (1, 0xFFFFFFFF)):
        cfg = _lib.PanakoMatchConfigEx(204, 320, 4, 16, 2, 1, bins, f_slack)
        rc, out = _raw_query(lib, "ucfp_panako_index_query_ex", cfg, ix, 1, blob, offs, 1, 3, 1)
        assert rc == -4 and set(out) == {0xA5}, (bins, f_slack)                    # UCFP_E_INVALID before anything runs
    for match in pp.INVALID_CONFIGS[1:] + [dict(bins=1, f_slack=1, **m) for m in pm.INVALID_CONFIGS]:
        with pytest.raises(errors.InvalidArgument):
            ix.query(1, [good], 3, **_py(match))
    for match in (dict(bins="both"), dict(bins=1), dict(bins="scaled", f_slack=-1), dict(bins="scaled", bogus=1)):
        with pytest.raises(errors.InvalidArgument):
            ix.query(1, [good], 3, **match)
    # the Python defaults of the two modes
    c = panako_match_config(bins="scaled")
    assert (c.scale_min, c.scale_max, c.scale_step, c.window, c.slack, c.r_slack, c.bins, c.f_slack) == (204, 320, 2, 16, 2, 1, 1, 1)
    c = panako_match_config()
    assert (c.scale_step, c.bins, c.f_slack) == (4, 0, 0)
    ref = pp.PanakoPitchRef({1: good})
    _check_all(ix, 1, ref, [good], 3, bins=1, f_slack=3, scale_min=200, scale_max=263, scale_step=1)       # 64 hypotheses
    _check_all(ix, 1, ref, [good], 3, bins=1, f_slack=3, scale_min=64, scale_max=1024, scale_step=16, slack=8)
    # unknown tenant, k = 0, empty query
    assert (ix.query(77, [good], 5, bins="scaled")[5] == 0).all()
    assert (ix.query(1, [good], 0, bins="scaled")[5] == 0).all()
    assert (ix.query(1, [b""], 5, bins="scaled")[5] == 0).all()
    ix.close()


def test_both_vote_paths_around_the_limit(gpu_ctx):
    """One scaled-mode query built three times, with lds_votes() - 1, lds_votes() and lds_votes() + 1 expanded votes:
    with bins 40 / 60 / 80 and f_slack = 1 a posting of the query's own hash follows it under 252, 256 and 260 alike
    (B_s moves by one bin), so postings with d' = 64 support all three hypotheses of a triple with d = 64 and postings
    with d' = 66 support one."""
    from ucfp_amd.index import PanakoIndex
    L = PanakoIndex.lds_votes()
    match = dict(scale_min=252, scale_max=260, scale_step=4, slack=1, window=16, bins=1, f_slack=1)
    rng = np.random.default_rng(2777)
    p3 = (L - 200) // 3
    hashes = [pp.hsh(ka, 40, 40, 3) for ka in (40, 60, 80)]
    rows = {rid: [] for rid in range(5)}
    for i, h in enumerate(hashes):
        p1 = L - 1 + i - 3 * p3
        for n, d in ((p3, 64), (p1, 66)):
            for x in rng.choice(3000, n, replace=False):
                rows[int(rng.integers(0, 5))].append((h, int(x), d))
    recs = {10 + rid: pm.rec(*r) for rid, r in rows.items()}
    qs = [pm.rec((h, 20, 64)) for h in hashes]
    ref = pp.PanakoPitchRef(recs)
    assert [ref.votes_total(q, **match) for q in qs] == [L - 1, L, L + 1]
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    for k in (1, 5):
        _check_all(ix, 0, ref, qs, k, **match)                    # one batch mixes the two paths
        for q in qs:
            _check_all(ix, 0, ref, [q], k, **match)
    ix.close()


def test_hot_hash_beside_a_live_one(gpu_ctx):
    """One hash with 50 000 postings in a single record, with and without a max_postings that stops it; its bucket also
    holds a hash that is not stopped (the same bins, another r) and the neighbouring buckets hold more."""
    from ucfp_amd.index import PanakoIndex
    rng = np.random.default_rng(2778)
    H = pp.hsh(0x155, 0x0AA, 0x111, 9)
    a = rng.choice(1 << 20, 50000, replace=False)
    hot = np.stack([np.full(50000, H), a, a, a + rng.integers(70, 91, 50000)], axis=1).astype(np.uint32)
    near = pm.rec((H + 1, 500, 80), (H - 1, 520, 80), (pp.hsh(0x155, 0x0AB, 0x110, 9), 540, 80),
                  (pp.hsh(0x154, 0x0AA, 0x112, 10), 560, 80), (pp.hsh(0x155, 0x0AA, 0x111, 12), 580, 80))
    recs = {7: np.concatenate([hot, near]), 8: near[:3], 9: pm.rec((H, 505, 80), (H + 1, 509, 80))}
    qs = [pm.rec((H, 10, 80), (H, 400, 300)), pm.rec((pp.hsh(0x156, 0x0AA, 0x111, 9), 0, 80))]
    match = dict(scale_min=250, scale_max=262, scale_step=2, bins=1, f_slack=1)
    for max_postings in (0, 1000):
        ref = pp.PanakoPitchRef(recs, max_postings)
        ix = PanakoIndex(max_postings, ctx=gpu_ctx)
        ix.upsert(5, np.array(list(recs), np.uint64), list(recs.values()))
        assert ix.size(5) == (3, ref.postings)
        assert (ref.votes_total(qs[0], **match) > PanakoIndex.lds_votes()) == (max_postings == 0)
        assert ref.query(qs[0], 5, **match)                       # the live hashes still answer beside the stopped one
        for k in (1, 128):
            _check_all(ix, 5, ref, qs, k, **match)
        _check_all(ix, 5, ref, qs, 5)                             # kept mode on the same index, stop flags made or not
        ix.close()


def test_dev_entry_on_a_side_stream(gpu_ctx, torch_cuda, small):
    from ucfp_amd.index import PanakoIndex, _pack_triplets
    torch = torch_cuda
    recs, qs = small
    match = dict(window=8, slack=1, bins=1, scale_step=2, f_slack=2)
    ix = PanakoIndex(30, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    side = torch.cuda.Stream()
    nq, k = len(qs), 10
    with torch.cuda.stream(side):
        qb, qo = _pack_triplets(qs)
        d_qb, d_qo = torch.from_numpy(qb.copy()).cuda(), torch.from_numpy(qo.view(np.int64)).cuda()
        o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        o_v, o_o, o_c = (torch.zeros((nq, k), dtype=torch.int32, device="cuda") for _ in range(3))
        o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
        ix.query_dev(0, d_qb.data_ptr(), d_qo.data_ptr(), nq, k, 2, o_ids.data_ptr(), o_v.data_ptr(), o_o.data_ptr(),
                     o_c.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), side.cuda_stream, **_py(match))
    side.synchronize()
    got = (o_ids.cpu().numpy().view(np.uint64), o_v.cpu().numpy().view(np.uint32), o_o.cpu().numpy(),
           o_c.cpu().numpy().view(np.uint32), o_s.cpu().numpy(), o_n.cpu().numpy().view(np.uint32))
    ref = pp.PanakoPitchRef(recs, 30)
    for q in range(nq):
        _check(got, q, ref.query(qs[q], k, 2, **match), k)
    assert got[5].sum() >= 8
    ix.close()


def test_two_host_threads_query_one_index(gpu_ctx, small):
    from ucfp_amd.index import PanakoIndex
    recs, qs = small
    ref = pp.PanakoPitchRef(recs)
    ix = PanakoIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    modes = {0: dict(bins=0), 1: dict(bins=1, **pp.SCALED_DEFAULTS)}                  # one thread per mode
    want = {b: [ref.query(q, 7, **m) for q in qs] for b, m in modes.items()}
    errs = []

    def work(b):
        try:
            for rep in range(4):
                sub = slice(rep % 2, len(qs), 2)
                got = ix.query(0, qs[sub], 7, **_py(modes[b]))
                for q, w in enumerate(want[b][sub]):
                    _check(got, q, w, 7)
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errs.append(e)

    threads = [threading.Thread(target=work, args=(b,)) for b in modes]
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


def _ref_hits(ref, q, k, **match):
    return [(rid, v, d, s / 256.0, np.float32(sc).tobytes()) for rid, v, d, s, sc in ref.query(q, k, **match)]


@pytest.fixture(scope="module")
def library(gpu_ctx):
    """The eight tone-burst recordings in a GpuIndex, and their reference."""
    from ucfp_amd import audio
    from ucfp_amd.index import GpuIndex
    gi = GpuIndex(gpu_ctx)
    recs = [audio.fingerprint_panako(pm.recording(i), 8000, TENANT, rid) for i, rid in enumerate(IDS)]
    gi.upsert(recs)
    return gi, pp.PanakoPitchRef({r.record_id: bytes(r.fingerprint) for r in recs})


def test_resampled_excerpts_end_to_end(gpu_ctx, library):
    """The excerpt [4 s, 12 s) of recording 3 played at seven speeds through a resampler, fingerprinted on the device:
    bins="scaled" finds it at rank 1 through identify_stretched and through a query body with `resampled`: true, with
    the reference's hits; the kept bins find it at speed 1.0 alone."""
    from ucfp_amd import audio
    from ucfp_amd.core import QueryRequest
    from ucfp_amd.errors import InvalidArgument
    gi, ref = library
    scaled = dict(bins=1, **pp.SCALED_DEFAULTS)
    for speed in pm.SPEEDS:
        q = audio.panako_hashes(pp.resampled_excerpt(3, speed), 8000, ctx=gpu_ctx)
        hits = gi.identify_stretched(TENANT, q, 5, bins="scaled")
        want = _ref_hits(ref, q, 5, **scaled)
        assert _hits(hits) == want, speed
        assert hits[0].record_id == 103 and hits[0].votes >= 50, (speed, want[:1])
        assert all(h.votes * 3 <= hits[0].votes for h in hits[1:])
        assert abs(hits[0].offset - 250) <= 16 and abs(hits[0].scale * 256 - 256 * speed) <= 6, (speed, want[0])
        body = {"tenant_id": TENANT, "modality": "Audio", "k": 5, "triplets": q.tolist(), "algorithm": "audiofp-panako-v1"}
        assert _hits(gi.query(QueryRequest.from_json({**body, "resampled": True}))) == want, speed
        kept = _hits(gi.query(QueryRequest.from_json(body)))
        assert kept == _ref_hits(ref, q, 5) == _hits(gi.query(QueryRequest.from_json({**body, "resampled": False})))
        assert (103 in [h[0] for h in kept]) == (speed == 1.0), speed
        assert _hits(gi.identify_stretched(TENANT, q, 5, bins="scaled", scale_step=4, f_slack=3)) == \
            _ref_hits(ref, q, 5, bins=1, scale_step=4, f_slack=3)
    body = {"tenant_id": TENANT, "modality": "Audio", "triplets": [], "algorithm": "audiofp-panako-v1"}
    assert QueryRequest.from_json(body).resampled is False
    for bad in ({**body, "resampled": 1}, {**body, "resampled": "true"},
                {"tenant_id": TENANT, "modality": "Audio", "landmarks": [], "resampled": True}):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json(bad)


def test_a_live_feed_that_runs_fast(gpu_ctx, library):
    """Recording 3 and recording 5 from 4 s on, fed to a PanakoStreams set at speeds 1.05 and 0.93 one second at a time:
    identify_live(bins="scaled") names them from the windows on the device and equals identify_stretched(bins="scaled")
    on the host copies of those windows."""
    from ucfp_amd import audio
    gi, ref = library
    live = audio.PanakoStreams(3, ctx=gpu_ctx, window_frames=500)
    slots = [live.open() for _ in range(3)]                        # the third stays empty
    feeds = [pp.render_resampled(pm.make_score(9300 + i), 4.0, 12.0, speed) for i, speed in ((3, 1.05), (5, 0.93))]
    for sec in range(7):
        live.push({s: x[sec * 8000:(sec + 1) * 8000] for s, x in zip(slots, feeds)})
    got = gi.identify_live(TENANT, live, slots, 3, 2, bins="scaled")
    host = live.windows(slots)
    for s, rid, speed in zip(slots, (103, 105, None), (1.05, 0.93, None)):
        hits, origin = got[s]
        assert origin == host[s][1]
        assert hits == gi.identify_stretched(TENANT, host[s][0], 3, 2, bins="scaled")
        assert _hits(hits) == _ref_hits(ref, host[s][0], 3, min_votes=2, bins=1, **pp.SCALED_DEFAULTS)
        if rid is None:
            assert hits == [] and host[s][0].shape[0] == 0
        else:
            assert hits[0].record_id == rid and hits[0].votes >= 20 and abs(hits[0].scale * 256 - 256 * speed) <= 6, (s, hits[:1])
            assert rid not in [h.record_id for h in gi.identify_live(TENANT, live, [s], 3, 2)[s][0]]   # the kept bins miss it
