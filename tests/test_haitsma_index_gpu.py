"""Haitsma sub-fingerprint index on the device: every id, distance, offset, score and hit count equals
the numpy reference (tests/haitsma_ref.py), on both paths (the LDS seed set and the global sort); mutations and errors;
the device entry points; and end-to-end identification of noisy excerpts from GPU fingerprints through GpuIndex and a
sidecar rebuild."""
import threading

import numpy as np
import pytest

import haitsma_ref as hr
from haitsma_ref import HaitsmaRef

pytestmark = pytest.mark.gpu

LDS_SEEDS = 3072          # hx_small answers a query with at most this many seeds from LDS; more go through global memory
INVALID_ID = 0xFFFFFFFFFFFFFFFF


def _check_hits(got, ref_hits, q, k, m):
    ids, dist, offs, scores, counts = got
    assert counts[q] == len(ref_hits), (q, counts[q], len(ref_hits), ref_hits[:3], ids[q, :3], dist[q, :3])
    for j, (rid, ds, d, _) in enumerate(ref_hits):
        assert (int(ids[q, j]), int(dist[q, j]), int(offs[q, j])) == (rid, ds, d), (q, j)
        want = np.float32(1) - np.float32(ds) / np.float32(32 * m)
        assert scores[q, j].tobytes() == want.tobytes(), (q, j)
    for j in range(len(ref_hits), k):
        assert ids[q, j] == INVALID_ID and dist[q, j] == 0xFFFFFFFF and offs[q, j] == 0 and scores[q, j] == -1.0


def _agree(ix, tenant, ref, queries, k, flip_bits, ppm=350_000):
    got = ix.query(tenant, queries, k, flip_bits, ppm)
    for q, qf in enumerate(queries):
        _check_hits(got, ref.query(qf, k, flip_bits, ppm), q, k, max(len(hr.as_frames(qf)), 1))
    return got


def _query_dev(torch, ix, tenant, queries, k, flip_bits, ppm):
    from ucfp_amd.index import _pack_frames
    flat, offs = _pack_frames(queries)
    nq = len(queries)
    d_f = torch.from_numpy(flat.view(np.int32).copy()).cuda()
    d_o = torch.from_numpy(offs.view(np.int64)).cuda()
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_d = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_o = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    ix.query_dev(tenant, d_f.data_ptr(), d_o.data_ptr(), nq, k, flip_bits, ppm, o_ids.data_ptr(), o_d.data_ptr(),
                 o_o.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (o_ids.cpu().numpy().view(np.uint64), o_d.cpu().numpy().view(np.uint32), o_o.cpu().numpy(), o_s.cpu().numpy(),
            o_n.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name,recs,q,max_postings", hr.fixed_cases(), ids=[c[0] for c in hr.fixed_cases()])
def test_fixed_cases(gpu_ctx, torch_cuda, name, recs, q, max_postings):
    from ucfp_amd.index import HaitsmaIndex
    ref = HaitsmaRef(recs, max_postings)
    ix = HaitsmaIndex(max_postings, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), [np.array(v, np.uint32) for v in recs.values()])
    assert ix.size(0) == (len(recs), sum(len(v) for v in recs.values()))
    qs = [np.array(q, np.uint32)]
    for flip_bits in (0, 1, 2):
        for k, ppm in ((10, 1_000_000), (1, 1_000_000), (10, 350_000), (10, 31_250), (10, 31_249)):
            host = _agree(ix, 0, ref, qs, k, flip_bits, ppm)
            dev = _query_dev(torch_cuda, ix, 0, qs, k, flip_bits, ppm)
            for a, b in zip(host, dev):
                assert np.array_equal(a, b)
    ix.close()


def _flip_bits(rng, frames, rate):
    noise = np.zeros(frames.size, np.uint32)
    for b in range(32):
        noise |= (rng.random(frames.size) < rate).astype(np.uint32) << np.uint32(b)
    return frames ^ noise


def _tenant(rng, nrec, max_len, alphabet):
    """Frames drawn partly from a skewed alphabet (long runs, shared values between records) and partly at random, with
    near neighbours of alphabet values mixed in."""
    alpha = rng.integers(0, 2**32, alphabet, dtype=np.uint64).astype(np.uint32)
    recs = {}
    for rid in rng.choice(1 << 40, nrec, replace=False).astype(np.uint64).tolist():
        n = int(rng.integers(0, max_len + 1))
        f = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        common = rng.random(n) < 0.3
        f[common] = alpha[(alphabet * rng.random(int(common.sum())) ** 3).astype(np.int64)]
        near = rng.random(n) < 0.05
        f[near] ^= np.uint32(1) << rng.integers(0, 32, int(near.sum())).astype(np.uint32)
        recs[rid] = f
    return recs


def _queries(rng, recs, nq, m_max, budget):
    """Slices of records with bits flipped at rates 0 .. 0.3, and unrelated blocks; ragged m from 1 to m_max (the first
    query has m_max frames, of the longest record if it is long enough, the second one frame), at most `budget` frames in
    all (the numpy reference looks 529 values up per frame)."""
    keys = [r for r in recs if recs[r].size]
    longest = max(keys, key=lambda r: recs[r].size) if keys else None
    out, used = [], 0
    for i in range(nq):
        m = int(min(m_max, max(1, rng.integers(1, m_max + 1) if i % 4 == 0 else rng.integers(1, 65))))
        if i < 2:
            m = (m_max, 1)[i]
        m = max(1, min(m, budget - used - (nq - i - 1)))
        used += m
        src = recs[keys[int(rng.integers(0, len(keys)))]] if keys else np.zeros(0, np.uint32)
        if i == 0 and keys:
            src = recs[longest]
        if i % 5 == 4 or src.size < m:
            out.append(rng.integers(0, 2**32, m, dtype=np.uint64).astype(np.uint32))
        else:
            a = int(rng.integers(0, src.size - m + 1))
            out.append(_flip_bits(rng, src[a:a + m].copy(), float(rng.choice([0.0, 0.02, 0.1, 0.2, 0.3]))))
    return out


# (records, longest record, alphabet, queries, largest m, k, flip_bits, max_postings, frame budget of the batch)
CONFIGS = [
    (1, 5000, 64, 1, 4096, 1, 2, 0, 4096), (400, 300, 4096, 512, 64, 10, 0, 0, 20000), (50, 5000, 16, 64, 512, 128, 1, 0, 12000),
    (3, 50, 4, 7, 40, 5, 2, 0, 280), (200, 1000, 256, 128, 256, 16, 2, 50, 6000), (30, 5000, 1024, 33, 4096, 3, 1, 0, 30000),
    (120, 2000, 8, 300, 32, 100, 0, 200, 9000), (10, 100, 2, 16, 100, 128, 2, 0, 1000), (400, 60, 512, 512, 16, 1, 1, 0, 8000),
    (64, 3000, 32, 20, 2048, 20, 2, 1000, 8000), (2, 5000, 1, 5, 1000, 2, 0, 0, 3000), (250, 500, 65536, 256, 128, 64, 2, 0, 6000),
    (17, 4000, 128, 64, 300, 7, 2, 5, 5000), (90, 900, 16, 90, 90, 90, 1, 0, 8000), (5, 5000, 4096, 1, 1, 128, 2, 0, 1),
    (300, 200, 64, 400, 24, 12, 0, 0, 9000), (40, 2500, 2, 40, 700, 40, 1, 3000, 12000), (8, 800, 8, 100, 8, 8, 2, 0, 800),
    (150, 1500, 2048, 10, 4096, 10, 0, 0, 40000), (25, 5000, 256, 200, 50, 128, 2, 0, 6000), (60, 60, 60, 60, 60, 60, 2, 60, 3000),
    (1, 1, 1, 3, 2, 1, 2, 0, 6),
    # more than 1024 queries: the batch is processed in passes
    (300, 200, 64, 2500, 8, 5, 0, 0, 12000), (50, 400, 16, 1100, 6, 3, 2, 0, 5000),
]


@pytest.fixture(scope="module")
def paths_seen():
    seen = {"lds": 0, "global": 0}
    yield seen
    assert seen["lds"] and seen["global"], seen      # both paths ran against the reference


@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_random_configurations_match_reference(gpu_ctx, paths_seen, cfg):
    from ucfp_amd.index import HaitsmaIndex
    nrec, max_len, alphabet, nq, m_max, k, flip_bits, max_postings, budget = CONFIGS[cfg]
    rng = np.random.default_rng(100 + cfg)
    ix = HaitsmaIndex(max_postings, ctx=gpu_ctx)
    tenants = {3: _tenant(rng, nrec, max_len, alphabet), 9: _tenant(rng, max(1, nrec // 3), max_len, alphabet)}
    for t, recs in tenants.items():
        keys = list(recs)
        half = len(keys) // 2
        ix.upsert(t, np.array(keys[:half], np.uint64), [recs[i] for i in keys[:half]])      # two upserts, one rebuild
        ix.upsert(t, np.array(keys[half:], np.uint64), [recs[i].tobytes() for i in keys[half:]])
    for t, recs in tenants.items():
        ref = HaitsmaRef(recs, max_postings)
        assert ix.size(t) == (len(recs), int(ref.flat.size))
        queries = _queries(rng, recs, nq if t == 3 else max(1, nq // 4), m_max, budget if t == 3 else max(1, budget // 4))
        for q in queries:
            paths_seen["global" if ref.seeds(q, flip_bits)[2] > LDS_SEEDS else "lds"] += 1
        _agree(ix, t, ref, queries, k, flip_bits)
        _agree(ix, t, ref, queries[:3], min(k, 4), flip_bits, 1_000_000)
    ix.close()


@pytest.mark.parametrize("max_postings", [0, 1000])
def test_hot_value_goes_through_global_memory(gpu_ctx, max_postings):
    """One value 50 000 times in the corpus: with max_postings = 0 a query holding it gathers more than 10^5 seeds, beside
    small queries in the same batch; with max_postings = 1000 the value is stopped."""
    from ucfp_amd.index import HaitsmaIndex
    rng = np.random.default_rng(6)
    H = 0xDEADBEEF
    recs = {}
    for r in range(50):
        f = rng.integers(0, 2**32, 3000, dtype=np.uint64).astype(np.uint32)
        f[rng.choice(3000, 1000, replace=False)] = H
        recs[11 * r + 2] = f
    src = recs[13]
    hot = np.flatnonzero(src == H)
    a = int(hot[hot < 2900][5])
    queries = [src[a:a + 48].copy(), _flip_bits(rng, src[100:164].copy(), 0.05), np.array([H, H ^ 1, H], np.uint32),
               rng.integers(0, 2**32, 20, dtype=np.uint64).astype(np.uint32), src[2000:2010].copy()]
    ref = HaitsmaRef(recs, max_postings)
    assert (ref.flat == H).sum() == 50_000
    seeds = [ref.seeds(q, 2)[2] for q in queries]
    if max_postings == 0:
        assert seeds[0] > 100_000 and seeds[2] > 100_000 and seeds[3] <= LDS_SEEDS
    else:
        assert max(seeds) <= LDS_SEEDS
    ix = HaitsmaIndex(max_postings, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    for flip_bits in (0, 2):
        for k in (1, 128):
            got = _agree(ix, 0, ref, queries, k, flip_bits, 1_000_000)
    assert int(got[0][0, 0]) == 13 and int(got[1][0, 0]) == 0 and int(got[2][0, 0]) == a
    ix.close()


def test_mutations_and_errors(gpu_ctx):
    from ucfp_amd import errors
    from ucfp_amd.index import HaitsmaIndex
    rng = np.random.default_rng(2)
    mk = lambda n: rng.integers(0, 64, n).astype(np.uint32) * np.uint32(0x01010101)  # noqa: E731
    recs = {i: mk(int(rng.integers(1, 200))) for i in range(40)}
    recs[41] = np.zeros(0, np.uint32)
    ix = HaitsmaIndex(0, ctx=gpu_ctx)
    ix.upsert(1, np.array(list(recs), np.uint64), list(recs.values()))
    ix.upsert(2, np.array([5], np.uint64), [recs[7]])                              # another tenant
    qs = [recs[7][:30].copy(), mk(5), recs[3][:8] ^ np.uint32(1), mk(1)]

    def agree(ix_, model, tenant=1):
        ref = HaitsmaRef(model)
        for flip_bits in (0, 2):
            _agree(ix_, tenant, ref, qs, 20, flip_bits, 1_000_000)
        assert ix_.size(tenant) == (len(model), int(ref.flat.size))

    agree(ix, recs)
    agree(ix, {5: recs[7]}, 2)
    orig7 = recs[7]
    recs[7] = mk(120)                                                              # upsert-replace
    ix.upsert(1, np.array([7], np.uint64), [recs[7].tobytes()])
    agree(ix, recs)
    assert ix.delete(1, np.array([3, 999], np.uint64)) == 1
    del recs[3]
    agree(ix, recs)
    recs[3] = mk(60)                                                               # re-upsert
    ix.upsert(1, np.array([3], np.uint64), [recs[3]])
    ix.flush()
    agree(ix, recs)
    agree(ix, {5: orig7}, 2)                                                       # tenant 2 untouched
    fresh = HaitsmaIndex(0, ctx=gpu_ctx)                                           # a fresh index over the final state
    fresh.upsert(1, np.array(list(recs), np.uint64), list(recs.values()))
    agree(fresh, recs)
    for a, b in zip(ix.query(1, qs, 20, 2, 1_000_000), fresh.query(1, qs, 20, 2, 1_000_000)):
        assert np.array_equal(a, b)
    fresh.close()
    # unknown tenant, k = 0, empty query, a tenant emptied by deletes
    ids, dist, offs, sc, n = ix.query(77, qs, 5)
    assert (n == 0).all() and (ids == INVALID_ID).all() and (dist == 0xFFFFFFFF).all() and (sc == -1).all()
    assert (ix.query(1, qs, 0)[4] == 0).all()
    both = ix.query(1, [b"", qs[0]], 5, 2, 1_000_000)
    assert both[4][0] == 0 and (both[0][0] == INVALID_ID).all()
    _check_hits(both, HaitsmaRef(recs).query(qs[0], 5, 2, 1_000_000), 1, 5, qs[0].size)
    assert ix.size(77) == (0, 0)
    assert ix.delete(2, [5]) == 1 and (ix.query(2, qs, 5)[4] == 0).all() and ix.size(2) == (0, 0)
    # errors
    too_long = np.zeros(4097, np.uint32)
    for call in (lambda: ix.query(1, [too_long], 5), lambda: ix.query(1, qs, 5, 3), lambda: ix.query(1, qs, 5, 2, 1_000_001),
                 lambda: ix.query(1, qs, 129), lambda: ix.upsert(1, [9], [b"\0" * 6]), lambda: ix.query(1, [b"\0" * 6], 5)):
        with pytest.raises(errors.InvalidArgument):
            call()
    assert ix.query(1, [np.zeros(4096, np.uint32)], 5)[4][0] == 0                  # the longest query is accepted
    agree(ix, recs)                                                                # nothing changed
    ix.close()


def test_dev_upsert_matches_host(gpu_ctx, torch_cuda):
    from ucfp_amd.index import HaitsmaIndex, _pack_frames
    torch = torch_cuda
    rng = np.random.default_rng(12)
    recs = _tenant(rng, 120, 800, 64)
    keys = list(recs)
    host, dev = HaitsmaIndex(40, ctx=gpu_ctx), HaitsmaIndex(40, ctx=gpu_ctx)
    host.upsert(0, np.array(keys, np.uint64), [recs[i] for i in keys])
    flat, offs = _pack_frames([recs[i] for i in keys])
    d_ids = torch.from_numpy(np.array(keys, np.uint64).view(np.int64)).cuda()
    d_f = torch.from_numpy(flat.view(np.int32).copy()).cuda()
    d_o = torch.from_numpy(offs.view(np.int64)).cuda()
    dev.upsert_dev(0, d_ids.data_ptr(), d_f.data_ptr(), d_o.data_ptr(), len(keys), torch.cuda.current_stream().cuda_stream)
    assert dev.size(0) == host.size(0)
    qs = _queries(rng, recs, 64, 256, 4000)
    h = host.query(0, qs, 10, 2, 400_000)
    d = _query_dev(torch, dev, 0, qs, 10, 2, 400_000)
    for a, b in zip(h, d):
        assert np.array_equal(a, b)
    ref = HaitsmaRef(recs, 40)
    for q in range(len(qs)):
        _check_hits(d, ref.query(qs[q], 10, 2, 400_000), q, 10, qs[q].size)
    host.close()
    dev.close()


def test_two_threads_query_one_index(gpu_ctx):
    from ucfp_amd.index import HaitsmaIndex
    rng = np.random.default_rng(21)
    recs = _tenant(rng, 150, 1500, 32)
    ref = HaitsmaRef(recs)
    ix = HaitsmaIndex(0, ctx=gpu_ctx)
    ix.upsert(0, np.array(list(recs), np.uint64), list(recs.values()))
    batches = [_queries(rng, recs, 40, 128, 2500), _queries(rng, recs, 25, 512, 3000)]
    want = [[ref.query(q, 8, f) for q in b] for b, f in zip(batches, (2, 1))]
    errs = []

    def work(i):
        try:
            for _ in range(6):
                got = ix.query(0, batches[i], 8, (2, 1)[i])
                for q, qf in enumerate(batches[i]):
                    _check_hits(got, want[i][q], q, 8, qf.size)
        except BaseException as e:   # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    ix.close()


# ---------------------------------------------------------------- end to end, from GPU fingerprints

@pytest.fixture(scope="module")
def corpora(gpu_ctx):
    from ucfp_amd import audio
    out = {}
    for name, gen, corpus_seed, excerpt_seed, snr, flips in hr.END_TO_END:
        xs = hr.corpus(gen, corpus_seed)
        fps = audio.haitsma_frames_batch(xs, hr.SR, ctx=gpu_ctx)
        ex = hr.excerpts(xs, snr, excerpt_seed)
        qs = audio.haitsma_frames_batch([clip for _, clip in ex], hr.SR, ctx=gpu_ctx)
        out[name] = (fps, [s0 for s0, _ in ex], qs, flips)
    return out


def _hit_tuple(h):
    return (h.record_id, h.distance, h.offset, np.float32(h.score).tobytes())


@pytest.mark.parametrize("name", [c[0] for c in hr.END_TO_END])
def test_end_to_end_through_gpu_index(gpu_ctx, corpora, name, tmp_path):
    from ucfp_amd import audio, store
    from ucfp_amd.core import HitSource, QueryRequest
    from ucfp_amd.index import GpuIndex
    fps, s0s, qs, flips = corpora[name]
    assert all(q.size == 256 for q in qs)
    path = str(tmp_path / "side.log")
    gi = GpuIndex(gpu_ctx, sidecar=store.Sidecar(path))
    gi.upsert([audio._record(audio.ALGORITHM_HAITSMA, f.tobytes(), 4, hr.FIRST_ID + i) for i, f in enumerate(fps)])
    ref = HaitsmaRef({hr.FIRST_ID + i: f for i, f in enumerate(fps)})
    assert gi._hx.size(4) == (24, sum(f.size for f in fps))
    for flip_bits in (0, 1, 2):
        good = 0
        for i, q in enumerate(qs):
            hits = gi.identify_frames(4, q, 5, flip_bits)
            want = ref.query(q, 5, flip_bits, 350_000)
            assert [_hit_tuple(h) for h in hits] == [(r, ds, d, np.float32(s).tobytes()) for r, ds, d, s in want]
            assert all(h.source == HitSource.Haitsma for h in hits)
            good += hr.identified(want, hr.FIRST_ID + i, s0s[i])
        print(name, "flip_bits", flip_bits, "identified", good, "of 24")
        if flip_bits in flips:
            assert good == 24
    # the wire route: flip_bits 2, max_ber 0.35
    body = {"tenant_id": 4, "modality": "Audio", "k": 5, "subfingerprints": qs[3].tobytes()}
    routed = gi.query(QueryRequest.from_json(body))
    assert [_hit_tuple(h) for h in routed] == [_hit_tuple(h) for h in gi.identify_frames(4, qs[3], 5)]
    assert routed[0].record_id == hr.FIRST_ID + 3
    body["subfingerprints"] = [int(x) for x in qs[3]]
    assert [_hit_tuple(h) for h in gi.query(QueryRequest.from_json(body))] == [_hit_tuple(h) for h in routed]
    assert gi.identify_frames(9, qs[3], 5) == [] and gi.identify_frames(4, qs[3], 0) == []
    # a record re-ingested under the same id as a Wang record leaves the Haitsma index
    gi.upsert([audio._record(audio.ALGORITHM_WANG, np.array([[1, 2], [3, 4]], np.uint32).tobytes(), 4, hr.FIRST_ID + 3)])
    assert all(h.record_id != hr.FIRST_ID + 3 for h in gi.identify_frames(4, qs[3], 5))
    assert gi._hx.size(4)[0] == 23 and gi._lm.size(4)[0] == 1
    gi.delete(4, [hr.FIRST_ID + 5])
    gi.flush()
    # an index rebuilt from the sidecar log answers like the one that wrote it
    gi2 = store.rebuild(path, gpu_ctx)
    assert gi2._hx.size(4) == gi._hx.size(4) and gi2._hx.size(4)[0] == 22
    for q in qs:
        assert [_hit_tuple(h) for h in gi2.identify_frames(4, q, 5)] == [_hit_tuple(h) for h in gi.identify_frames(4, q, 5)]
    assert gi2.identify_frames(4, qs[7], 5)[0].record_id == hr.FIRST_ID + 7
    assert all(h.record_id not in (hr.FIRST_ID + 3, hr.FIRST_ID + 5) for q in (qs[3], qs[5]) for h in gi2.identify_frames(4, q, 5))
