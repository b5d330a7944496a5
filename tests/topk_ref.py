"""Plain numpy statement of the top-k contract of ucfp_hip.h (the merge entry points and the key images they carry).

Nothing here knows how the kernels work.  Keys are u32, smaller is better, 0xffffffff marks "no entry"; ids are u64;
the order everywhere is (key ascending, id ascending), both unsigned."""
import numpy as np

INVALID_KEY = 0xFFFFFFFF
INVALID_ID = 0xFFFFFFFFFFFFFFFF
HAMMING64, COSINE_F32 = 1, 2      # ucfp_index_kind


def merge_lists(ids, keys, k):
    """ids [parts, nq, k_in] u64, keys [parts, nq, k_in] u32 -> (ids [nq, k] u64, keys [nq, k] u32, counts [nq] u32).

    Per query: the set of distinct (key, id) pairs whose key is not 0xffffffff, sorted by (key, id), the first k of
    them, padded with (2^64 - 1, 0xffffffff)."""
    ids = np.asarray(ids, np.uint64)
    keys = np.asarray(keys, np.uint32)
    assert ids.ndim == 3 and ids.shape == keys.shape
    nq = ids.shape[1]
    o_ids = np.full((nq, k), INVALID_ID, np.uint64)
    o_keys = np.full((nq, k), INVALID_KEY, np.uint32)
    o_cnt = np.zeros(nq, np.uint32)
    for q in range(nq):
        kq, iq = keys[:, q, :].reshape(-1), ids[:, q, :].reshape(-1)
        live = kq != np.uint32(INVALID_KEY)
        kq, iq = kq[live], iq[live]
        order = np.lexsort((iq, kq))                             # by key, then by id: both unsigned
        kq, iq = kq[order], iq[order]
        first = np.ones(kq.size, bool)
        first[1:] = (kq[1:] != kq[:-1]) | (iq[1:] != iq[:-1])    # each distinct (key, id) pair once
        kq, iq = kq[first][:k], iq[first][:k]
        o_ids[q, :iq.size] = iq
        o_keys[q, :kq.size] = kq
        o_cnt[q] = kq.size
    return o_ids, o_keys, o_cnt


def hamming_scores(keys):
    """f32 similarity 1 - d / 64 of a Hamming distance; -1.0 where there is no entry."""
    keys = np.asarray(keys, np.uint32)
    s = np.float32(1.0) - keys.astype(np.float32) * np.float32(1.0 / 64.0)
    return np.where(keys == np.uint32(INVALID_KEY), np.float32(-1.0), s).astype(np.float32)


def cosine_key(score):
    """f32 score -> u32 key: the ascending order image of the float (sign bit set for positives, all bits flipped for
    negatives), inverted so that a larger score is a smaller key."""
    u = np.asarray(score, np.float32).view(np.uint32)
    neg = (u & np.uint32(0x80000000)) != 0
    return ~np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def cosine_score(key):
    """The inverse of cosine_key, bit for bit."""
    u = ~np.asarray(key, np.uint32)
    pos = (u & np.uint32(0x80000000)) != 0
    return np.where(pos, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def cosine_scores(keys):
    """f32 score of every key; -2.0 where there is no entry."""
    keys = np.asarray(keys, np.uint32)
    return np.where(keys == np.uint32(INVALID_KEY), np.float32(-2.0), cosine_score(keys)).astype(np.float32)


def scores(kind, keys):
    return hamming_scores(keys) if kind == HAMMING64 else cosine_scores(keys)


# The floats of the spec test and of the cosine merge cases, ascending: both zeros, both smallest denormals, +-1 and
# their neighbours on either side, both infinities.
def edge_floats():
    one = np.float32(1.0)
    inf = np.float32(np.inf)
    den = np.float32(1.401298464324817e-45)
    f = [-inf, np.nextafter(-one, -inf), -one, np.nextafter(-one, np.float32(0)), np.float32(-0.5), -den,
         np.float32(-0.0), np.float32(0.0), den, np.float32(0.5), np.nextafter(one, np.float32(0)), one,
         np.nextafter(one, inf), inf]
    return np.array(f, np.float32)
