"""The merge entry points of ucfp_hip.h on synthetic lists, with no index involved: ucfp_topk_merge_dev,
ucfp_topk_pack_dev, ucfp_topk_merge_packed_dev and ucfp_topk_merge_packed_ex_dev against tests/topk_ref.py, bit for bit
(ids, keys, counts, scores).

Shapes come from the constants of topk_merge_u32 (topk.hip) and of its entry points (index.hip, shard.hip):
  kStage = 2048          a query's parts x k candidates are staged in LDS up to this many and re-read from global memory
                         in each of the k rounds beyond it;
  UCFP_INDEX_MAX_K = 128 the largest k;
  64                     the bits of the missing-shard mask, and the most parts of a packed merge beyond kStage candidates.
"""
import numpy as np
import pytest

import topk_ref as ref

pytestmark = pytest.mark.gpu

K_STAGE = 2048            # topk.hip topk_merge_u32: kStage
MAX_K = 128               # ucfp_hip.h: UCFP_INDEX_MAX_K
MASK_BITS = 64            # shard.hip: the missing-shard mask is one u64
E_UNSUPPORTED, E_INVALID = -2, -4      # ucfp_hip.h: ucfp_status
INVALID_KEY, INVALID_ID = ref.INVALID_KEY, ref.INVALID_ID
KINDS = (ref.HAMMING64, ref.COSINE_F32)

SMALL = [(1, 1), (1, MAX_K), (2, 10), (3, 7), (8, 10), (MASK_BITS - 1, 10), (MASK_BITS, 10)]
STAGED_EDGE = [(K_STAGE // MAX_K, MAX_K), (MASK_BITS, K_STAGE // MASK_BITS)]              # (16,128), (64,32): 2048 exactly
UNSTAGED = [(K_STAGE // MAX_K + 1, MAX_K), (MASK_BITS, K_STAGE // MASK_BITS + 1), (MASK_BITS, MAX_K)]   # (17,128) (64,33) (64,128)
# beyond 64 parts (a packed merge takes these only while parts x k <= kStage); 205 x 10 = 2050 and 2049 x 1 are unstaged
MANY_PARTS = [(MASK_BITS + 1, 10), (K_STAGE // 10 + 1, 10), (K_STAGE, 1), (K_STAGE + 1, 1)]
ALL_SHAPES = SMALL + STAGED_EDGE + UNSTAGED + MANY_PARTS
assert ALL_SHAPES == [(1, 1), (1, 128), (2, 10), (3, 7), (8, 10), (63, 10), (64, 10), (16, 128), (64, 32), (17, 128),
                      (64, 33), (64, 128), (65, 10), (205, 10), (2048, 1), (2049, 1)]
NQS = [1, 3, 64, 65, 130]                # one query, a few, a wave's worth of workgroups, one more, and twice that
# every content class runs on both sides of the staging edge, through both entries and, at 205 parts, the unpacked one alone
CONTENT_SHAPES = [(2, 10), (8, 10), (16, 128), (64, 32), (17, 128), (64, 33), (205, 10)]
CONTENT_NQS = [3, 65]


def packed_ok(parts, k):
    """shard.hip ucfp_topk_merge_packed_ex_dev: more than 64 parts only while the candidates fit the LDS stage."""
    return parts <= MASK_BITS or parts * k <= K_STAGE


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


class Merger:
    """Calls the entry points on device copies of host arrays and returns host arrays."""

    def __init__(self, torch, ctx):
        from ucfp_amd import _lib
        self.torch, self.ctx, self.lib = torch, ctx, _lib.load()

    def outputs(self, nq, k):
        t = self.torch
        # (filled with a pattern no answer holds: an entry the merge did not write shows)
        return (t.full((nq, k), 0x5A5A5A5A5A5A5A5A, dtype=t.int64, device="cuda"),
                t.full((nq, k), 12345.0, dtype=t.float32, device="cuda"),
                t.full((nq, k), 0x5A5A5A5A, dtype=t.int32, device="cuda"),
                t.full((nq,), 0x5A5A5A5A, dtype=t.int32, device="cuda"))

    def host(self, outs):
        o_ids, o_sc, o_keys, o_cnt = outs
        return (o_ids.cpu().numpy().view(np.uint64), o_sc.cpu().numpy().view(np.uint32), o_keys.cpu().numpy().view(np.uint32),
                o_cnt.cpu().numpy().view(np.uint32))

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream or None

    def lists(self, kind, ids, keys):
        parts, nq, k = ids.shape
        d_ids, d_keys = _dev(self.torch, ids), _dev(self.torch, keys)
        outs = self.outputs(nq, k)
        rc = self.lib.ucfp_topk_merge_dev(self.ctx.handle, kind, d_ids.data_ptr(), d_keys.data_ptr(), parts, nq, k,
                                          outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                          self.stream())
        assert rc == 0, rc
        self.torch.cuda.synchronize()
        return self.host(outs)

    def pack(self, ids, keys):
        """ucfp_topk_pack_dev over [parts][nq][k] at once: entries are packed one by one, so the result is the layout an
        all-gather of the parts' packed lists delivers."""
        t = self.torch
        d_ids, d_keys = _dev(t, ids), _dev(t, keys)
        ent = t.full(tuple(ids.shape) + (2,), 0x5A5A5A5A5A5A5A5A, dtype=t.int64, device="cuda")
        rows = int(np.prod(ids.shape[:-1]))
        rc = self.lib.ucfp_topk_pack_dev(self.ctx.handle, d_ids.data_ptr(), d_keys.data_ptr(), rows, ids.shape[-1],
                                         ent.data_ptr(), self.stream())
        assert rc == 0, rc
        return ent

    def packed(self, kind, ids, keys, missing=None, ex=False):
        """-> (ids, scores, keys, counts[, mask]).  missing: parts replaced by 0xff bytes, as a shard that could not scan
        sends them."""
        t = self.torch
        parts, nq, k = ids.shape
        ent = self.pack(ids, keys)
        if missing:
            ent[sorted(missing)] = -1
        outs = self.outputs(nq, k)
        args = [self.ctx.handle, kind, ent.data_ptr(), parts, nq, k, outs[0].data_ptr(), outs[1].data_ptr(),
                outs[2].data_ptr(), outs[3].data_ptr()]
        if ex:
            mask = t.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=t.int64, device="cuda")
            rc = self.lib.ucfp_topk_merge_packed_ex_dev(*args, mask.data_ptr(), self.stream())
        else:
            rc = self.lib.ucfp_topk_merge_packed_dev(*args, self.stream())
        assert rc == 0, rc
        t.cuda.synchronize()
        res = self.host(outs)
        return res + (int(mask.cpu().numpy().view(np.uint64)[0]),) if ex else res


@pytest.fixture(scope="module")
def merger(gpu_ctx, torch_cuda):
    return Merger(torch_cuda, gpu_ctx)


def check(got, want, kind, what):
    g_ids, g_sc, g_keys, g_cnt = got[:4]
    w_ids, w_keys, w_cnt = want
    assert np.array_equal(g_cnt, w_cnt), (what, "counts")
    assert np.array_equal(g_keys, w_keys), (what, "keys")
    assert np.array_equal(g_ids, w_ids), (what, "ids")
    assert np.array_equal(g_sc, ref.scores(kind, w_keys).view(np.uint32)), (what, "scores")


def check_all_entries(merger, ids, keys, what, kinds=KINDS):
    """Every entry point that takes this shape, for both kinds, against the contract."""
    parts, nq, k = ids.shape
    want = ref.merge_lists(ids, keys, k)
    for kind in kinds:
        check(merger.lists(kind, ids, keys), want, kind, (what, "lists", kind))
        if packed_ok(parts, k):
            check(merger.packed(kind, ids, keys), want, kind, (what, "packed", kind))
    return want


# ---- contents ---------------------------------------------------------------------------------------------------------------

def sort_lists(ids, keys):
    """Every list sorted by (key, id) as a shard returns it: its invalid entries at the tail, carrying the invalid id."""
    ids = np.where(keys == np.uint32(INVALID_KEY), np.uint64(INVALID_ID), ids)
    order = np.lexsort((ids, keys), axis=-1)
    return np.take_along_axis(ids, order, -1), np.take_along_axis(keys, order, -1)


def random_ids(rng, shape):
    return rng.integers(0, 2**64 - 1, shape, dtype=np.uint64)          # (never 2^64 - 1)


def thin_out(rng, keys, nq_empty=True):
    """Different fill levels: lists of 0 .. k entries, whole parts empty, some lists full, the last query empty everywhere."""
    parts, nq, k = keys.shape
    fill = rng.integers(0, k + 1, (parts, nq))
    fill[rng.random((parts, nq)) < 0.15] = 0
    fill[rng.random((parts, nq)) < 0.30] = k
    if parts > 1:
        fill[rng.integers(0, parts), :] = 0                          # one part answers nothing at all
    if nq_empty and nq >= 3:
        fill[:, nq - 1] = 0                                           # count 0
    keys = keys.copy()
    keys[np.arange(k)[None, None, :] >= fill[..., None]] = INVALID_KEY
    return keys


def realistic(rng, parts, nq, k):
    """Hamming distances 0 .. 64 (ties everywhere) under distinct ids."""
    keys = thin_out(rng, rng.integers(0, 65, (parts, nq, k)).astype(np.uint32))
    return sort_lists(random_ids(rng, keys.shape), keys)


SPECIAL_IDS = [0, 1, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**64 - 2]


def id_pool(rng, m):
    """The ids on which a comparison of 64 bits in two halves goes wrong."""
    pool = list(SPECIAL_IDS)
    for _ in range(m):
        h1, l1 = (int(x) for x in rng.integers(0, 2**32 - 1, 2))
        h2, l2 = int(rng.integers(h1 + 1, 2**32)), int(rng.integers(l1 + 1, 2**32))      # h1 < h2, l1 < l2
        pool += [(h1 << 32) | l1, (h2 << 32) | l1,        # the low word shared, the high words differ
                 (h1 << 32) | l2,                         # the high word shared with the first, the low words differ
                 (h2 << 32) | l1, (h1 << 32) | l2,        # (again) the order of the low words contradicts that of the high words
                 int(rng.integers(0, 2**64 - 1, dtype=np.uint64))]
    pool = np.unique(np.array(pool, np.uint64))
    assert pool[-1] != np.uint64(INVALID_ID)
    return pool


def equal_keys(rng, parts, nq, k):
    """One key everywhere: the order is by id alone."""
    pool = id_pool(rng, max(16, parts * k // 6))
    ids = pool[rng.integers(0, pool.size, (parts, nq, k))]
    keys = thin_out(rng, np.full((parts, nq, k), 7, np.uint32), nq_empty=False)
    return sort_lists(ids, keys)


EDGE_KEYS = np.array([0, 1, 64, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], np.uint32)


def edge_keys(rng, parts, nq, k):
    """The keys around the sign bit and at both ends of the range, mixed with random ones."""
    shape = (parts, nq, k)
    # every third query holds nothing below 0x7fffffff (cosine scores <= +0.0): its whole answer lies around the sign bit
    high = (np.arange(nq) % 3 == 0)[None, :, None]
    edge = np.where(high, EDGE_KEYS[3:][rng.integers(0, 3, shape)], EDGE_KEYS[rng.integers(0, EDGE_KEYS.size, shape)])
    rand = rng.integers(np.where(high, 0x7FFFFFFF, 0), 2**32 - 1, shape, dtype=np.uint64)
    # (there about k / 3 entries of each edge key over all parts, so that the best k reach past 0x7fffffff and 0x80000000)
    keys = np.where(rng.random(shape) < np.where(high, min(0.5, 1.5 / parts), 0.5), edge, rand).astype(np.uint32)
    pool = id_pool(rng, 8)
    ids = np.where(rng.random(shape) < 0.5, pool[rng.integers(0, pool.size, shape)], random_ids(rng, shape))
    return sort_lists(ids, thin_out(rng, keys))


def duplicates(rng, parts, nq, k):
    """A stale row lives in several shards: the same (key, id) in 2, 3 and all parts is emitted once; the same id under two
    keys twice.  Query 0 (and every third): all parts hold the same k pairs, so k distinct pairs remain only after
    de-duplication; the others: each part returns the best k of its random share of k + 3 pairs."""
    ids = np.full((parts, nq, k), INVALID_ID, np.uint64)
    keys = np.full((parts, nq, k), INVALID_KEY, np.uint32)
    for q in range(nq):
        identical = q % 3 == 0
        npool = k if identical else k + 3
        pkeys = rng.integers(0, 6, npool).astype(np.uint32)           # few keys: ties by id among the duplicates
        pids = random_ids(rng, npool)
        if npool >= 5:
            pids[4] = pids[3]                                        # one id under two different keys
            pkeys[4] = pkeys[3] + 1
        member = np.ones((parts, npool), bool) if identical else rng.random((parts, npool)) < 0.5
        if not identical:
            member[:, 0] = True                                      # in all parts
            member[:, 1] = np.arange(parts) < 2                      # in two
            member[:, 2] = np.arange(parts) < 3                      # in three
        for p in range(parts):
            mk, mi = pkeys[member[p]], pids[member[p]]
            order = np.lexsort((mi, mk))[:k]                         # a shard returns its best k
            keys[p, q, :order.size] = mk[order]
            ids[p, q, :order.size] = mi[order]
    return ids, keys


def invalid_anywhere(rng, parts, nq, k):
    """Invalid entries in front of and between the valid ones, half of them under some other id than 2^64 - 1."""
    ids, keys = realistic(rng, parts, nq, k)
    order = np.argsort(rng.random(keys.shape), axis=-1)
    ids, keys = np.take_along_axis(ids, order, -1).copy(), np.take_along_axis(keys, order, -1).copy()
    if k >= 2:
        keys[..., 0][rng.random((parts, nq)) < 0.5] = INVALID_KEY    # in front
    dead = keys == np.uint32(INVALID_KEY)
    ids[dead] = INVALID_ID
    other = dead & (rng.random(keys.shape) < 0.5)
    ids[other] = random_ids(rng, int(other.sum()))
    return ids, keys


def cosine_lists(rng, parts, nq, k):
    """Keys of real scores: the edge floats of the spec test among random scores in [-1, 1]."""
    edge = ref.edge_floats()
    shape = (parts, nq, k)
    sc = np.where(rng.random(shape) < 0.4, edge[rng.integers(0, edge.size, shape)],
                  rng.uniform(-1.0, 1.0, shape).astype(np.float32)).astype(np.float32)
    keys = thin_out(rng, ref.cosine_key(sc))
    return sort_lists(random_ids(rng, shape), keys)


CONTENTS = {"realistic": realistic, "equal_keys": equal_keys, "edge_keys": edge_keys, "duplicates": duplicates,
            "invalid_anywhere": invalid_anywhere, "cosine_scores": cosine_lists}


def _seed(*xs):
    s = 0
    for x in xs:
        s = s * 1000003 + (sum(map(ord, x)) if isinstance(x, str) else int(x))
    return s % 2**32


# ---- the merges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parts,k", ALL_SHAPES)
def test_merge_realistic_lists_every_shape(merger, parts, k):
    """Sorted, tail-padded lists with different fill levels, empty parts and an all-empty query, at every shape and every
    number of queries, through the unpacked and (where the shape is allowed) the packed entry, for both kinds."""
    for nq in NQS:
        rng = np.random.default_rng(_seed(parts, k, nq))
        ids, keys = realistic(rng, parts, nq, k)
        _, _, w_cnt = check_all_entries(merger, ids, keys, (parts, k, nq))
        if nq >= 3:
            assert w_cnt[nq - 1] == 0                                  # (the empty query is really there)


@pytest.mark.parametrize("parts,k", CONTENT_SHAPES)
@pytest.mark.parametrize("content", [c for c in CONTENTS if c != "realistic"])
def test_merge_contents_both_sides_of_the_stage(merger, content, parts, k):
    for nq in CONTENT_NQS:
        rng = np.random.default_rng(_seed(content, parts, k, nq))
        ids, keys = CONTENTS[content](rng, parts, nq, k)
        assert not np.any((ids == np.uint64(INVALID_ID)) & (keys != np.uint32(INVALID_KEY)))
        w_ids, w_keys, w_cnt = check_all_entries(merger, ids, keys, (content, parts, k, nq))
        # what each class is there for must really occur in its expectation
        if content == "equal_keys":
            hi, lo = w_ids >> np.uint64(32), w_ids & np.uint64(0xFFFFFFFF)
            live = w_keys[:, 1:] != np.uint32(INVALID_KEY)
            assert np.any((np.diff(lo.astype(np.int64), axis=1) < 0) & live)      # id order against the low words' order
            assert np.any((hi[:, 1:] == hi[:, :-1]) & live) and np.any((hi[:, 1:] != hi[:, :-1]) & live)
        if content == "edge_keys":
            assert w_keys[0, 0] >= np.uint32(0x7FFFFFFF) and np.any((w_keys[0] >= np.uint32(0x80000000)) & (w_keys[0] != np.uint32(INVALID_KEY)))
            assert np.any(w_keys[1] < np.uint32(0x7FFFFFFF))
        if content == "duplicates":
            assert w_cnt[0] == k and np.all(keys[:, 0, :] == keys[:1, 0, :])       # k distinct pairs, all parts alike
            live = keys[:, 1, :].reshape(-1) != np.uint32(INVALID_KEY)
            flat = np.stack([keys[:, 1, :].reshape(-1).astype(np.uint64), ids[:, 1, :].reshape(-1)], 1)[live]
            assert np.unique(flat, axis=0).shape[0] < flat.shape[0]              # pairs that several parts hold
            twice = [q for q in range(nq) if np.unique(w_ids[q, :w_cnt[q]]).size < w_cnt[q]]
            assert twice, "no id was emitted under two keys"
        if content == "invalid_anywhere":
            assert np.any((keys[..., :-1] == np.uint32(INVALID_KEY)) & (keys[..., 1:] != np.uint32(INVALID_KEY)))


def test_same_id_under_two_keys_is_emitted_twice_and_equal_pairs_once(merger):
    """The documented rule in the small: (3, A) in all four parts -> once; A again under key 5 -> a second time."""
    a, b = 2**63 + 5, 9
    ids = np.full((4, 1, 3), INVALID_ID, np.uint64)
    keys = np.full((4, 1, 3), INVALID_KEY, np.uint32)
    for p in range(4):
        ids[p, 0, 0], keys[p, 0, 0] = a, 3
    ids[1, 0, 1], keys[1, 0, 1] = a, 5
    ids[2, 0, 1], keys[2, 0, 1] = b, 3
    ids[3, 0, 1], keys[3, 0, 1] = b, 3
    want = check_all_entries(merger, ids, keys, "pairs")
    assert want[0][0].tolist() == [b, a, a] and want[1][0].tolist() == [3, 3, 5] and want[2][0] == 3


@pytest.mark.parametrize("kind", KINDS)
def test_merge_scores_of_real_keys(merger, kind):
    """Hamming: every distance 0 .. 64 -> 1 - d / 64, padding -1.0.  Cosine: the scores that went in come back bit for
    bit, in descending order (+0.0 ahead of -0.0), padding -2.0."""
    rng = np.random.default_rng(60 + kind)
    for parts, k in [(8, 10), (64, 32), (64, 33), (205, 10)]:
        nq = 5
        if kind == ref.HAMMING64:
            keys = rng.integers(0, 65, (parts, nq, k)).astype(np.uint32)
            keys[0, 0, :min(k, 65)] = np.arange(min(k, 65))
            ids, keys = sort_lists(random_ids(rng, keys.shape), thin_out(rng, keys))
            pool = ref.hamming_scores(np.arange(65, dtype=np.uint32))
            pad = np.float32(-1.0)
        else:
            ids, keys = cosine_lists(rng, parts, nq, k)
            pool = ref.cosine_score(keys[keys != np.uint32(INVALID_KEY)])
            pad = np.float32(-2.0)
        want = ref.merge_lists(ids, keys, k)
        for got in [merger.lists(kind, ids, keys)] + ([merger.packed(kind, ids, keys)] if packed_ok(parts, k) else []):
            check(got, want, kind, (parts, k))
            sc = got[1].view(np.float32)
            for q in range(nq):
                c = int(got[3][q])
                assert np.all(np.isin(sc[q, :c].view(np.uint32), pool.view(np.uint32)))
                assert np.all(sc[q, c:] == pad)
                assert np.all(sc[q, 1:c] <= sc[q, :c - 1]) if c > 1 else True
        assert want[2][nq - 1] == 0 and want[2].max() == k


def test_merge_config5_all_gather_shape(merger):
    """BASELINE configs[4]: 8 ranks x 4096 queries x k = 10 -- the buffer one all-gather delivers to every rank."""
    parts, nq, k = 8, 4096, 10
    rng = np.random.default_rng(55)
    ids, keys = realistic(rng, parts, nq, k)
    ids[3], keys[3] = ids[2], keys[2]                                  # a rank that holds a stale copy of its neighbour's rows
    want = ref.merge_lists(ids, keys, k)
    check(merger.packed(ref.HAMMING64, ids, keys), want, ref.HAMMING64, "packed")
    check(merger.packed(ref.COSINE_F32, ids, keys, ex=True), want, ref.COSINE_F32, "packed_ex")
    check(merger.lists(ref.HAMMING64, ids, keys), want, ref.HAMMING64, "lists")


# ---- packing -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq,k", [(1, 1), (51, 5), (2, MAX_K), (257, 1), (4096, 10)])
def test_pack_equals_the_host_wire_format(merger, nq, k):
    """ucfp_topk_pack_dev == sharded.pack_entries byte for byte: nq x k = 1, 255, 256, 257 (the 256-thread blocks of the
    pack kernel and one entry either side) and 40 960 (config 5's list), with high-bit ids and padding entries."""
    from ucfp_amd import sharded
    assert nq * k in (1, 255, 256, 257, 40_960)
    rng = np.random.default_rng(nq * 131 + k)
    pool = id_pool(rng, 8)
    ids = np.where(rng.random((nq, k)) < 0.5, pool[rng.integers(0, pool.size, (nq, k))], random_ids(rng, (nq, k)))
    keys = rng.integers(0, 2**32 - 1, (nq, k), dtype=np.uint64).astype(np.uint32)
    ids[0, 0], keys[0, 0] = 2**64 - 2, 0xFFFFFFFE
    pad = rng.random((nq, k)) < 0.3
    pad[-1, -1] = nq * k > 1
    ids[pad], keys[pad] = INVALID_ID, INVALID_KEY
    ent = merger.pack(ids, keys)
    merger.torch.cuda.synchronize()
    got = ent.cpu().numpy()
    want = sharded.pack_entries(ids, keys)
    assert got.shape == want.shape == (nq, k, 2) and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes()
    back_ids, back_keys = sharded.unpack_entries(got)
    assert np.array_equal(back_ids, ids) and np.array_equal(back_keys, keys)


# ---- the missing-shard mask -----------------------------------------------------------------------------------------------

def _missing_sets(parts):
    sets = [set(), {0}, {31, 32}, {MASK_BITS - 1}, {0, MASK_BITS - 1}, set(range(parts)) - {parts // 2}, set(range(parts)) - {0}]
    out = []
    for s in sets:
        if all(p < parts for p in s) and s not in out:
            out.append(s)
    return out


@pytest.mark.parametrize("parts,k", [(1, 10), (2, 10), (MASK_BITS, 10), (MASK_BITS, K_STAGE // MASK_BITS + 1)])
def test_missing_mask_equals_the_missing_set(merger, parts, k):
    """Every bit of the mask, at 1, 2 and 64 parts, staged and unstaged (64 x 33): the mask is the set of parts that sent
    0xff bytes, the answer the merge of the others; a part that scanned and found nothing is NOT missing."""
    nq = 3
    rng = np.random.default_rng(_seed(parts, k, 77))
    ids, keys = realistic(rng, parts, nq, k)
    if parts > 1:
        assert np.any(np.all(keys == np.uint32(INVALID_KEY), axis=(1, 2)))    # an empty part that did answer
    sets = _missing_sets(parts)
    assert set() in sets and (parts < MASK_BITS or {31, 32} in sets)
    for missing in sets:
        present = [p for p in range(parts) if p not in missing]
        w_ids, w_keys, w_cnt = ref.merge_lists(ids[present], keys[present], k) if present else \
            ref.merge_lists(np.full((1, nq, k), INVALID_ID, np.uint64), np.full((1, nq, k), INVALID_KEY, np.uint32), k)
        for kind in KINDS:
            got = merger.packed(kind, ids, keys, missing=missing, ex=True)
            assert got[4] == sum(1 << p for p in missing), (sorted(missing), hex(got[4]))
            check(got, (w_ids, w_keys, w_cnt), kind, (parts, k, sorted(missing)))


# ---- arguments ----------------------------------------------------------------------------------------------------------------

def test_merge_argument_statuses(merger):
    """Every status below is returned before anything is launched (index.hip ucfp_topk_merge_dev, shard.hip
    ucfp_topk_pack_dev / ucfp_topk_merge_packed_ex_dev: the checks precede the first launch_* call)."""
    t, lib, h = merger.torch, merger.lib, merger.ctx.handle
    parts, nq, k = 3, 2, 4
    ids, keys = realistic(np.random.default_rng(1), parts, nq, k)
    d_ids, d_keys = _dev(t, ids), _dev(t, keys)
    ent = merger.pack(ids, keys)
    big = t.zeros((MASK_BITS + 1) * MAX_K * 2, dtype=t.int64, device="cuda")   # room for any shape named below
    o_ids, o_sc, o_keys, o_cnt = outs = merger.outputs(nq, MAX_K + 1)
    mask = t.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=t.int64, device="cuda")
    p = [x.data_ptr() for x in outs]
    st = merger.stream()

    def lists(kind=ref.HAMMING64, a=d_ids.data_ptr(), b=d_keys.data_ptr(), parts=parts, nq=nq, k=k, oi=p[0], ok=p[2], oc=p[3]):
        return lib.ucfp_topk_merge_dev(h, kind, a, b, parts, nq, k, oi, p[1], ok, oc, st)

    def packed(kind=ref.HAMMING64, e=ent.data_ptr(), parts=parts, nq=nq, k=k, oi=p[0], ok=p[2], oc=p[3], m=None):
        return lib.ucfp_topk_merge_packed_ex_dev(h, kind, e, parts, nq, k, oi, p[1], ok, oc, m, st)

    assert lists(k=MAX_K + 1) == E_INVALID and packed(k=MAX_K + 1) == E_INVALID
    assert lists(a=None) == E_INVALID and lists(b=None) == E_INVALID
    assert lists(oi=None) == E_INVALID and lists(ok=None) == E_INVALID and lists(oc=None) == E_INVALID
    assert packed(e=None) == E_INVALID and packed(oi=None) == E_INVALID and packed(ok=None) == E_INVALID
    assert packed(oc=None) == E_INVALID
    assert lib.ucfp_topk_pack_dev(h, None, d_keys.data_ptr(), nq, k, ent.data_ptr(), st) == E_INVALID
    assert lib.ucfp_topk_pack_dev(h, d_ids.data_ptr(), None, nq, k, ent.data_ptr(), st) == E_INVALID
    assert lib.ucfp_topk_pack_dev(h, d_ids.data_ptr(), d_keys.data_ptr(), nq, k, None, st) == E_INVALID
    for kind in (0, 3, -1):
        assert lists(kind=kind) == E_UNSUPPORTED and packed(kind=kind) == E_UNSUPPORTED
        assert lib.ucfp_topk_merge_packed_dev(h, kind, ent.data_ptr(), parts, nq, k, p[0], p[1], p[2], p[3], st) == E_UNSUPPORTED
    # a packed merge beyond 64 parts needs its candidates in the LDS stage: 65 x 32 = 2080 > kStage
    assert packed(e=big.data_ptr(), parts=MASK_BITS + 1, k=K_STAGE // MASK_BITS) == E_UNSUPPORTED
    assert packed(e=big.data_ptr(), parts=MASK_BITS + 1, k=MAX_K) == E_UNSUPPORTED
    # the mask holds 64 parts, also where the merge itself would take more (65 x 10 <= kStage)
    assert packed(e=big.data_ptr(), parts=MASK_BITS + 1, k=10, m=mask.data_ptr()) == E_UNSUPPORTED
    # nothing to do: OK, and nothing is written
    assert lists(nq=0) == 0 and lists(k=0) == 0 and packed(nq=0) == 0 and packed(k=0) == 0
    assert packed(nq=0, m=mask.data_ptr()) == 0
    assert lib.ucfp_topk_pack_dev(h, d_ids.data_ptr(), d_keys.data_ptr(), 0, k, big.data_ptr(), st) == 0
    assert lib.ucfp_topk_pack_dev(h, d_ids.data_ptr(), d_keys.data_ptr(), nq, 0, big.data_ptr(), st) == 0
    t.cuda.synchronize()
    g_ids, g_sc, g_keys, g_cnt = merger.host(outs)
    assert np.all(g_ids == np.uint64(0x5A5A5A5A5A5A5A5A)) and np.all(g_keys == np.uint32(0x5A5A5A5A))
    assert np.all(g_cnt == np.uint32(0x5A5A5A5A)) and np.all(g_sc.view(np.float32) == np.float32(12345.0))
    assert int(mask.cpu().numpy().view(np.uint64)[0]) == 0x5A5A5A5A5A5A5A5A and not big.any().item()
    # scores are optional
    assert lib.ucfp_topk_merge_dev(h, ref.HAMMING64, d_ids.data_ptr(), d_keys.data_ptr(), parts, nq, k, p[0], None, p[2],
                                   p[3], st) == 0
    t.cuda.synchronize()
    w_ids, w_keys, w_cnt = ref.merge_lists(ids, keys, k)
    g_ids, g_sc, g_keys, g_cnt = merger.host(outs)
    assert np.array_equal(g_ids.reshape(-1)[:nq * k].reshape(nq, k), w_ids) and np.array_equal(g_cnt, w_cnt)
    assert np.all(g_sc.view(np.float32) == np.float32(12345.0))


def test_merge_of_nothing_but_empty_lists(merger):
    """One query, every part empty: count 0 and padding everywhere."""
    for parts, k in [(1, 1), (8, 10), (17, MAX_K)]:
        ids = np.full((parts, 1, k), INVALID_ID, np.uint64)
        keys = np.full((parts, 1, k), INVALID_KEY, np.uint32)
        want = check_all_entries(merger, ids, keys, (parts, k))
        assert want[2][0] == 0


# ---- streams -----------------------------------------------------------------------------------------------------------------

def test_merge_on_a_side_stream(merger):
    """The work is enqueued on the stream that is passed: synchronising that stream alone makes the answer visible."""
    t, lib, h = merger.torch, merger.lib, merger.ctx.handle
    parts, nq, k = 17, 65, MAX_K                                          # the unstaged loop: the longest of the merges
    rng = np.random.default_rng(17)
    ids, keys = realistic(rng, parts, nq, k)
    d_ids, d_keys = _dev(t, ids), _dev(t, keys)
    outs_l, outs_p = merger.outputs(nq, k), merger.outputs(nq, k)
    ent = t.empty((parts, nq, k, 2), dtype=t.int64, device="cuda")
    t.cuda.synchronize()                                                  # the inputs and the patterns are in place
    side = t.cuda.Stream()
    assert side.cuda_stream != t.cuda.current_stream().cuda_stream
    assert lib.ucfp_topk_merge_dev(h, ref.COSINE_F32, d_ids.data_ptr(), d_keys.data_ptr(), parts, nq, k, outs_l[0].data_ptr(),
                                   outs_l[1].data_ptr(), outs_l[2].data_ptr(), outs_l[3].data_ptr(), side.cuda_stream) == 0
    assert lib.ucfp_topk_pack_dev(h, d_ids.data_ptr(), d_keys.data_ptr(), parts * nq, k, ent.data_ptr(), side.cuda_stream) == 0
    assert lib.ucfp_topk_merge_packed_dev(h, ref.HAMMING64, ent.data_ptr(), parts, nq, k, outs_p[0].data_ptr(),
                                          outs_p[1].data_ptr(), outs_p[2].data_ptr(), outs_p[3].data_ptr(),
                                          side.cuda_stream) == 0
    side.synchronize()
    want = ref.merge_lists(ids, keys, k)
    check(merger.host(outs_l), want, ref.COSINE_F32, "lists")
    check(merger.host(outs_p), want, ref.HAMMING64, "packed")
