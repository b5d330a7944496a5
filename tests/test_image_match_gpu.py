"""Image search that scores global and block hashes together, on the device (image_match.hip): ids, score
bytes and counts equal the exact top-k by (score desc, id asc) of the restatement (tests/image_match_ref.py) -- over
random records with edited copies of the queries planted, for both record sizes, every weighting, ties, the score cut,
tenants, mutations, the pass loop, the device entry points, and end to end from frames through GpuIndex.query and
store.rebuild.  Every comparison is bit-exact: there is no tolerance anywhere."""
import numpy as np
import pytest

import image_match_ref as ref

pytestmark = pytest.mark.gpu

INVALID_ID = ref.INVALID_ID
N_BIG, N_SMALL, NQ, NQ_BIG = 70_001, 5000, 65, 3
ALGO = {168: 2, 536: 7}            # UCFP_IMG_PHASH, UCFP_IMG_MULTI
STARTS = {168: [32], 536: [64, 232, 400]}
T = 32                             # the default block_distance_threshold: planted blocks sit at T and T + 1


def _set_block(rec, start, b, value):
    rec[start + 8 + 8 * b:start + 16 + 8 * b] = np.frombuffer(int(value).to_bytes(8, "little"), np.uint8)


def _get_block(rec, start, b):
    return int.from_bytes(rec[start + 8 + 8 * b:start + 16 + 8 * b].tobytes(), "little")


def _flip(rng, value, nbits):
    for bit in rng.choice(64, nbits, replace=False).tolist():
        value ^= 1 << bit
    return value


def _edited(rng, rec, kind):
    """A planted copy.  kind 0: exact.  kind 1: 1-4 blocks of every algorithm replaced by random words, a few bits flipped
    in the others and in the global hash.  kind 2: like 1 with 0 replaced, and two blocks at distance exactly T and two at
    T + 1.  kind 3: a light edit -- a few bits only."""
    out = rec.copy()
    if kind == 0:
        return out
    for s in STARTS[rec.size]:
        g = int.from_bytes(out[s:s + 8].tobytes(), "little")
        out[s:s + 8] = np.frombuffer(_flip(rng, g, int(rng.integers(0, 9))).to_bytes(8, "little"), np.uint8)
        replaced = rng.choice(16, int(rng.integers(1, 5)), replace=False).tolist() if kind == 1 else []
        exact = rng.choice(16, 4, replace=False).tolist() if kind == 2 else []
        for b in range(16):
            v = _get_block(out, s, b)
            if b in replaced:
                v = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
            elif b in exact:
                v = _flip(rng, v, T if exact.index(b) < 2 else T + 1)
            else:
                v = _flip(rng, v, int(rng.integers(0, 4)))
            _set_block(out, s, b, v)
    return out


def _make_pool(size):
    rng = np.random.default_rng(size)
    rows = rng.integers(0, 256, (N_BIG, size), dtype=np.uint8)
    queries = rng.integers(0, 256, (NQ, size), dtype=np.uint8)
    for q in range(NQ):                 # four copies each: those of the first 15 queries among the first 60 rows, the rest
        for j in range(4):              # among rows 64 .. 263
            slot = q * 4 + j if q < 15 else 64 + (q - 15) * 4 + j
            rows[slot] = _edited(rng, queries[q], j)
    ids = rng.permutation(np.arange(1, N_BIG + 1, dtype=np.uint64) * np.uint64(0x9E3779B1))   # row order is not id order
    small = ref.score_matrix(queries, rows[:N_SMALL])
    big = ref.score_matrix(queries[:NQ_BIG], rows)
    return rows, ids, queries, small, big


@pytest.fixture(scope="module")
def pools():
    """Per record size: rows, ids, queries and the restatement's default-config scores, computed once: `small` is 65
    queries over the first 5000 rows, `big` 3 queries over all 70 001."""
    return {size: _make_pool(size) for size in (168, 536)}


def _want(ids, sm, k, min_score=0.0):
    res = [ref.topk(ids, sm[q], k, min_score) for q in range(sm.shape[0])]
    return (np.array([r[0] for r in res], np.uint64).reshape(-1, k), np.array([r[1] for r in res], np.float32).reshape(-1, k),
            np.array([r[2] for r in res], np.uint32))


def _check(got, want, k):
    g_ids, g_s, g_n = got
    w_ids, w_s, w_n = want
    assert g_ids.shape == g_s.shape == (w_n.size, k)
    assert np.array_equal(g_n, w_n), (g_n[:8], w_n[:8])
    assert np.array_equal(g_ids, w_ids), np.argwhere(g_ids != w_ids)[:4]
    assert g_s.tobytes() == w_s.tobytes(), np.argwhere(g_s.view(np.uint32) != w_s.view(np.uint32))[:4]


def _index(gpu_ctx, size):
    from ucfp_amd.index import ImageMatchIndex
    return ImageMatchIndex(ALGO[size], 0, gpu_ctx)


def _cfg(c: ref.Cfg):
    from ucfp_amd.image import MultiHashConfig
    return MultiHashConfig(c.ahash_weight, c.phash_weight, c.dhash_weight, c.global_weight, c.block_weight,
                           c.block_distance_threshold, c.min_score)


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("nq", [1, 3, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 512, 513, 1000, 5000])
@pytest.mark.parametrize("size", [168, 536])
def test_sizes(gpu_ctx, pools, size, n, nq, k):
    rows, ids, queries, small, _ = pools[size]
    ix = _index(gpu_ctx, size)
    ix.upsert(5, ids[:n], rows[:n])
    assert ix.size(5) == n
    got = ix.query(5, queries[:nq], k)
    _check(got, _want(ids[:n], small[:nq, :n], k), k)
    m = min(nq, 15, (n + 3) // 4)                             # queries whose exact copy lies among the first n rows
    assert (got[1][:m, 0] == 1.0).all()                       # it comes first, at exactly 1.0
    if k > n:
        assert (got[2] == n).all() and (got[0][:, n:] == INVALID_ID).all() and (got[1][:, n:] == -1.0).all()
    ix.close()


@pytest.mark.parametrize("size", [168, 536])
def test_two_level_merge(gpu_ctx, pools, size):
    rows, ids, queries, _, big = pools[size]
    ix = _index(gpu_ctx, size)
    ix.upsert(0, ids, rows)
    for k in (10, 128):
        _check(ix.query(0, queries[:NQ_BIG], k), _want(ids, big, k), k)
    ix.close()


@pytest.mark.parametrize("size", [168, 536])
def test_pass_loop(gpu_ctx, pools, monkeypatch, size):
    """A key matrix smaller than the batch: 4096 bytes hold 3 key rows of 300, so 7 queries run in passes of 3, 3 and 1."""
    rows, ids, queries, small, _ = pools[size]
    monkeypatch.setenv("UCFP_IMAGE_MATCH_KEY_BYTES", "4096")
    ix = _index(gpu_ctx, size)
    monkeypatch.delenv("UCFP_IMAGE_MATCH_KEY_BYTES")
    ix.upsert(0, ids[:300], rows[:300])
    for k in (10, 128):
        _check(ix.query(0, queries[:7], k), _want(ids[:300], small[:7, :300], k), k)
    ix.close()


@pytest.mark.parametrize("size", [168, 536])
def test_identical_rows_return_the_smallest_ids(gpu_ctx, size):
    rng = np.random.default_rng(12)
    row = rng.integers(0, 256, size, dtype=np.uint8)
    ids = rng.permutation(np.arange(1000, dtype=np.uint64) * np.uint64(7) + np.uint64(3))    # inserted in shuffled order
    ix = _index(gpu_ctx, size)
    ix.upsert(0, ids, np.tile(row, (1000, 1)))
    near = _edited(rng, row, 3)
    g_ids, g_s, g_n = ix.query(0, np.stack([row, near]), 10)
    assert g_ids[0].tolist() == g_ids[1].tolist() == sorted(ids.tolist())[:10] and g_n.tolist() == [10, 10]
    assert (g_s[0] == 1.0).all() and (g_s[1] == ref.score_matrix(near[None], row[None])[0, 0]).all()
    ix.close()


WEIGHTS = [ref.Cfg(), ref.Cfg(0.0, 1.0, 0.0), ref.Cfg(global_weight=1.0, block_weight=0.0),
           ref.Cfg(global_weight=0.0, block_weight=1.0), ref.Cfg(block_distance_threshold=0),
           ref.Cfg(block_distance_threshold=64), ref.Cfg(0.25, 0.5, 0.125, 0.7, 0.3, 33),
           ref.Cfg(1.0, 1.0, 1.0, 1.0, 1.0, 32)]       # the last one scores above 1


@pytest.mark.parametrize("size", [168, 536])
def test_weights(gpu_ctx, pools, size):
    rows, ids, queries, _, _ = pools[size]
    n, nq = 1000, 20
    ix = _index(gpu_ctx, size)
    ix.upsert(0, ids[:n], rows[:n])
    for cfg in WEIGHTS:
        sm = ref.score_matrix(queries[:nq], rows[:n], cfg)
        got = ix.query(0, queries[:nq], 10, _cfg(cfg))
        _check(got, _want(ids[:n], sm, 10), 10)
    over = ix.query(0, queries[:nq], 10, _cfg(WEIGHTS[-1]))[1]
    assert (over[:, 0] == (6.0 if size == 536 else 2.0)).all()       # no clamp: the exact copy scores the sum of the weights
    assert (np.diff(over.astype(np.float64), axis=1) <= 0).all()      # and a score above 1 still orders
    ix.close()


@pytest.mark.parametrize("size", [168, 536])
def test_min_score(gpu_ctx, pools, size):
    rows, ids, queries, small, _ = pools[size]
    n = 1000
    ix = _index(gpu_ctx, size)
    ix.upsert(0, ids[:n], rows[:n])
    q = queries[20:23]
    sm = small[20:23, :n]
    for q_i in range(3):
        third = np.sort(sm[q_i])[::-1][2]                           # a hit whose score equals min_score stays
        cfg = ref.Cfg(min_score=float(third))
        got = ix.query(0, q[q_i:q_i + 1], 10, _cfg(cfg))
        _check(got, _want(ids[:n], sm[q_i:q_i + 1], 10, cfg.min_score), 10)
        cnt = int(got[2][0])
        assert cnt == int((sm[q_i] >= third).sum()) >= 3 and got[1][0, cnt - 1] == third
        above = float(np.nextafter(third, np.float32(2.0)))         # one ulp more and it goes
        assert int(ix.query(0, q[q_i:q_i + 1], 10, _cfg(ref.Cfg(min_score=above)))[2][0]) == int((sm[q_i] > third).sum())
    # a cut at exactly 1.0 keeps the exact copies only; above every score there is nothing
    got = ix.query(0, q, 10, _cfg(ref.Cfg(min_score=1.0)))
    _check(got, _want(ids[:n], sm, 10, 1.0), 10)
    assert got[2].tolist() == [1, 1, 1]
    e_ids, e_s, e_n = ix.query(0, q, 10, _cfg(ref.Cfg(min_score=1.5)))
    assert not e_n.any() and (e_ids == INVALID_ID).all() and (e_s == -1.0).all()
    ix.close()


def test_invalid_arguments(gpu_ctx):
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.image import MultiHashConfig
    from ucfp_amd.index import ImageMatchIndex
    for algo, flags in ((3, 0), (0, 0), (7, 1)):
        with pytest.raises(InvalidArgument):
            ImageMatchIndex(algo, flags, gpu_ctx)
    ix = _index(gpu_ctx, 536)
    ix.upsert(0, np.array([1], np.uint64), np.zeros((1, 536), np.uint8))
    q = np.zeros((1, 536), np.uint8)
    for bad in (MultiHashConfig(0.0, 0.0, 0.0), MultiHashConfig(global_weight=0.0, block_weight=0.0),
                MultiHashConfig(phash_weight=float("nan")), MultiHashConfig(block_distance_threshold=65),
                MultiHashConfig(min_score=-1.0), MultiHashConfig(dhash_weight=1.5)):
        with pytest.raises(InvalidArgument):
            ix.query(0, q, 1, bad)
    with pytest.raises(InvalidArgument):
        ix.query(0, q, 129)
    with pytest.raises(InvalidArgument):
        ix.upsert(0, np.array([1], np.uint64), np.zeros((1, 168), np.uint8))
    one = _index(gpu_ctx, 168)                                       # the algorithm weights do not count there
    one.upsert(0, np.array([1], np.uint64), np.zeros((1, 168), np.uint8))
    assert one.query(0, np.zeros((1, 168), np.uint8), 1, MultiHashConfig(0.0, 0.0, 0.0))[1][0, 0] == 1.0
    ix.close()
    one.close()


@pytest.mark.parametrize("size", [168, 536])
def test_tenants_mutations_and_empty_answers(gpu_ctx, pools, size):
    rows, ids, queries, small, _ = pools[size]
    ix = _index(gpu_ctx, size)
    a_ids, b_ids = ids[:300], ids[300:500]
    ix.upsert(1, a_ids, rows[:300])
    ix.upsert(2, b_ids, rows[300:500])
    assert (ix.size(1), ix.size(2), ix.size(3)) == (300, 200, 0)
    q = queries[:5]
    sm_a, sm_b = small[:5, :300], small[:5, 300:500]
    _check(ix.query(1, q, 10), _want(a_ids, sm_a, 10), 10)
    _check(ix.query(2, q, 10), _want(b_ids, sm_b, 10), 10)
    # unknown tenant, k = 0, nq = 0
    e_ids, e_s, e_n = ix.query(9, q, 10)
    assert (e_ids == INVALID_ID).all() and (e_s == -1.0).all() and not e_n.any()
    assert not ix.query(1, q, 0)[2].any()
    assert ix.query(1, np.zeros((0, size), np.uint8), 10)[2].shape == (0,)
    # upsert of a known id replaces its row: the exact copy of query 0 becomes a stranger's record
    first = int(ix.query(1, q[:1], 1)[0][0, 0])
    pos = int(np.flatnonzero(a_ids == np.uint64(first))[0])
    assert pos == 0
    changed = rows[:300].copy()
    changed[pos] = rows[N_SMALL + 7]
    ix.upsert(1, a_ids[pos:pos + 1], changed[pos:pos + 1])
    assert ix.size(1) == 300
    _check(ix.query(1, q, 10), ref.search(a_ids, changed, q, 10), 10)
    assert int(ix.query(1, q[:1], 1)[0][0, 0]) != first
    # delete: known ids go, unknown ones are not counted, the other tenant is untouched
    gone = a_ids[:50]
    assert ix.delete(1, np.concatenate([gone, np.array([1], np.uint64)])) == 50 and ix.delete(1, gone) == 0
    assert (ix.size(1), ix.size(2)) == (250, 200)
    ix.flush()
    _check(ix.query(1, q, 10), ref.search(a_ids[50:], changed[50:], q, 10), 10)
    _check(ix.query(2, q, 10), _want(b_ids, sm_b, 10), 10)
    assert ix.delete(2, b_ids) == 200 and not ix.query(2, q, 10)[2].any()
    ix.close()


@pytest.mark.parametrize("size", [168, 536])
def test_device_entry_points(gpu_ctx, torch_cuda, pools, size):
    torch = torch_cuda
    rows, ids, queries, small, _ = pools[size]
    n, nq, k = 777, 33, 10
    st = torch.cuda.current_stream().cuda_stream
    ix = _index(gpu_ctx, size)
    d_ids = torch.from_numpy(ids[:n].view(np.int64).copy()).cuda()
    d_rows = torch.from_numpy(rows[:n].copy()).cuda()
    ix.upsert_dev(0, d_ids.data_ptr(), d_rows.data_ptr(), n, st)
    assert ix.size(0) == n
    d_q = torch.from_numpy(queries[:nq].copy()).cuda()
    cfg = ref.Cfg(0.2, 0.5, 0.3, 0.5, 0.5, 30, 0.25)
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    ix.query_dev(0, d_q.data_ptr(), nq, k, _cfg(cfg), o_ids.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)
    torch.cuda.synchronize()
    got = (o_ids.cpu().numpy().view(np.uint64), o_s.cpu().numpy(), o_n.cpu().numpy().view(np.uint32))
    _check(got, ref.search(ids[:n], rows[:n], queries[:nq], k, cfg), k)
    _check(ix.query(0, queries[:nq], k, _cfg(cfg)), got, k)            # the host twin
    ix.query_dev(0, d_q.data_ptr(), nq, k, None, o_ids.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)   # no config: defaults
    torch.cuda.synchronize()
    got = (o_ids.cpu().numpy().view(np.uint64), o_s.cpu().numpy(), o_n.cpu().numpy().view(np.uint32))
    _check(got, _want(ids[:n], small[:nq, :n], k), k)
    ix.close()


def _frames(rng, n):
    """Synthetic 256 x 256 grey frames (normalisation is the identity at that size): 16 x 16 cells of random grey with
    pixel noise on top."""
    cells = rng.integers(0, 256, (n, 16, 16)).astype(np.float64)
    fr = np.kron(cells, np.ones((16, 16))) + rng.normal(0.0, 6.0, (n, 256, 256))
    return np.clip(fr, 0, 255).astype(np.uint8)


def test_gpu_index_end_to_end(gpu_ctx, tmp_path):
    """frames -> fingerprint_frames -> GpuIndex.upsert -> query with an `image_record` body: a copy with one or two 64 x 64
    blocks overwritten finds its original first, above every unrelated frame; the answers equal the restatement; and
    the same after store.rebuild."""
    from ucfp_amd import image, store
    from ucfp_amd.core import HitSource, Modality, QueryRequest, Record
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.index import GpuIndex
    rng = np.random.default_rng(21)
    n = 12
    originals = _frames(rng, n)
    copies = originals.copy()
    for i in range(n):
        for _ in range(1 + i % 2):
            by, bx = int(rng.integers(0, 4)), int(rng.integers(0, 4))
            copies[i, 64 * by:64 * by + 64, 64 * bx:64 * bx + 64] = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    tags = {image.MULTI: image.ALGORITHM_MULTIHASH, image.DHASH: image.ALGORITHM_DHASH}
    base = {image.MULTI: 100, image.DHASH: 200}
    recs, fps, qfps = [], {}, {}
    for algo, tag in tags.items():
        fp, st = image.fingerprint_frames(originals, algo=algo)
        qfp, qst = image.fingerprint_frames(copies, algo=algo)
        assert not st.any() and not qst.any()
        fps[algo], qfps[algo] = fp, qfp
        recs += [Record(tenant_id=3, record_id=base[algo] + i, modality=Modality.Image, format_version=image.FORMAT_VERSION,
                        algorithm=tag, config_hash=0, fingerprint=fp[i].tobytes()) for i in range(n)]
    recs += [Record(tenant_id=4, record_id=100 + i, modality=Modality.Image, format_version=image.FORMAT_VERSION,
                    algorithm=image.ALGORITHM_MULTIHASH, config_hash=0, fingerprint=fps[image.MULTI][i].tobytes())
             for i in range(3)]                                                      # another tenant
    path = str(tmp_path / "side.log")
    gi = GpuIndex(gpu_ctx, sidecar=store.Sidecar(path))
    gi.upsert(recs)
    dto = {"phash-weight": 0.5, "dhash-weight": 0.25, "ahash-weight": 0.25, "block-distance-threshold": 24}
    dto_cfg = ref.Cfg(0.25, 0.5, 0.25, 0.4, 0.6, 24, 0.0)

    def check_all(index):
        for algo, tag in tags.items():
            ids = np.arange(base[algo], base[algo] + n, dtype=np.uint64)
            for i in range(n):
                for body, cfg in (({}, ref.Cfg()), ({"multi_hash": dto, "min_score": 0.125}, dto_cfg)):
                    wire = list(qfps[algo][i].tobytes()) if i % 2 else qfps[algo][i].tobytes().hex()
                    req = QueryRequest.from_json({"tenant_id": 3, "modality": "Image", "image_record": wire, "k": 5,
                                                  "algorithm": tag, **body})
                    hits = index.query(req)
                    cfg.min_score = body.get("min_score", 0.0)
                    w_ids, w_s, w_n = ref.search(ids, fps[algo], qfps[algo][i:i + 1], 5, cfg)
                    assert [h.record_id for h in hits] == w_ids[0, :w_n[0]].tolist()
                    assert np.array([h.score for h in hits], np.float32).tobytes() == w_s[0, :w_n[0]].tobytes()
                    assert all(h.source == HitSource.ImageMatch and h.tenant_id == 3 for h in hits)
                    assert hits[0].record_id == base[algo] + i, (algo, i, hits[:2])     # the original, above every stranger
                    assert len(hits) == 1 or hits[0].score > hits[1].score

    check_all(gi)
    # an exact copy scores 1.0; without `algorithm` a bundle searches the bundles and a 168-byte record the only
    # single-algorithm index; the other tenant only sees its own three
    rec0 = fps[image.MULTI][0].tobytes()
    top = gi.similar_images(3, rec0, 1)
    assert [(h.record_id, h.score) for h in top] == [(100, 1.0)]
    assert gi.similar_images(3, fps[image.DHASH][1].tobytes(), 1)[0].record_id == 201
    assert len(gi.similar_images(4, rec0, 10)) == 3 and gi.similar_images(5, rec0, 10) == [] and gi.similar_images(3, rec0, 0) == []
    assert [h.record_id for h in gi.similar_images(3, rec0, 10, config=image.MultiHashConfig(min_score=1.0))] == [100]
    assert gi.similar_images(3, fps[image.DHASH][1].tobytes(), 3, algorithm=image.ALGORITHM_AHASH) == []   # nothing indexed there
    with pytest.raises(InvalidArgument):
        gi.similar_images(3, rec0, 1, algorithm=image.ALGORITHM_PHASH)
    with pytest.raises(InvalidArgument):
        gi.similar_images(3, rec0, 1, config=image.MultiHashConfig(block_distance_threshold=99))
    # the global hashes still feed the Hamming spaces exactly as before
    gh = image.global_hashes(rec0)
    assert gi.hamming(3, image.ALGORITHM_PHASH, gh["phash"], 1)[0].record_id == 100
    gi.flush()
    gi2 = store.rebuild(path, gpu_ctx)
    assert {t: ix.size(3) for t, ix in gi2._im.items()} == {image.ALGORITHM_MULTIHASH: n, image.ALGORITHM_DHASH: n}
    check_all(gi2)
    # overwrite rule: id 100 re-ingested as a phash record leaves the bundle index and enters the phash one
    ph, _ = image.fingerprint_frames(originals[:1], algo=image.PHASH)
    gi.upsert([Record(tenant_id=3, record_id=100, modality=Modality.Image, format_version=image.FORMAT_VERSION,
                      algorithm=image.ALGORITHM_PHASH, config_hash=0, fingerprint=ph[0].tobytes())])
    assert 100 not in [h.record_id for h in gi.similar_images(3, rec0, 12)]
    assert [h.record_id for h in gi.similar_images(3, ph[0].tobytes(), 1, algorithm=image.ALGORITHM_PHASH)] == [100]
    with pytest.raises(InvalidArgument):                   # two single-algorithm indexes now: which one must be said
        gi.similar_images(3, ph[0].tobytes(), 1)
    gi.delete(3, range(100, 100 + n))
    assert gi.similar_images(3, rec0, 10) == [] and gi.similar_images(3, ph[0].tobytes(), 1, algorithm=image.ALGORITHM_PHASH) == []
    assert len(gi.similar_images(3, fps[image.DHASH][1].tobytes(), 20, algorithm=image.ALGORITHM_DHASH)) == n
