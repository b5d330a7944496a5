"""CPU restatement of TLSH 128/1: digest, L value, distance and an exact top-k by (distance, id).

Pure numpy / Python, written from the spec text, independent of the HIP kernels.  A digest is 35 bytes in the order of
the published hex string: swap(checksum), swap(L), (Q1 << 4) | Q2, code[31] .. code[0]."""
import math

import numpy as np

V = [
    1, 87, 49, 12, 176, 178, 102, 166, 121, 193, 6, 84, 249, 230, 44, 163, 14, 197, 213, 181, 161, 85, 218, 80, 64, 239, 24, 226, 236, 142, 38, 200,
    110, 177, 104, 103, 141, 253, 255, 50, 77, 101, 81, 18, 45, 96, 31, 222, 25, 107, 190, 70, 86, 237, 240, 34, 72, 242, 20, 214, 244, 227, 149, 235,
    97, 234, 57, 22, 60, 250, 82, 175, 208, 5, 127, 199, 111, 62, 135, 248, 174, 169, 211, 58, 66, 154, 106, 195, 245, 171, 17, 187, 182, 179, 0, 243,
    132, 56, 148, 75, 128, 133, 158, 100, 130, 126, 91, 13, 153, 246, 216, 219, 119, 68, 223, 78, 83, 88, 201, 99, 122, 11, 92, 32, 136, 114, 52, 10,
    138, 30, 48, 183, 156, 35, 61, 26, 143, 74, 251, 94, 129, 162, 63, 152, 170, 7, 115, 167, 241, 206, 3, 150, 55, 59, 151, 220, 90, 53, 23, 131,
    125, 173, 15, 238, 79, 95, 89, 16, 105, 137, 225, 224, 217, 160, 37, 123, 118, 73, 2, 157, 46, 116, 9, 145, 134, 228, 207, 212, 202, 215, 69, 229,
    27, 188, 67, 124, 168, 252, 42, 4, 29, 108, 21, 247, 19, 205, 39, 203, 233, 40, 186, 147, 198, 192, 155, 33, 164, 191, 98, 204, 165, 180, 117, 76,
    140, 36, 210, 172, 41, 54, 159, 8, 185, 232, 113, 196, 231, 47, 146, 120, 51, 65, 28, 144, 254, 221, 93, 189, 194, 139, 112, 43, 71, 109, 184, 209,
]
V_SHA256 = "aa5a5e7ca4804ae04607f40d749f988a83aa2bc2a5ad80ce8ffc18ea44fe478e"
_VN = np.array(V, np.uint8)

TLSH_BYTES = 35
MAX_DISTANCE = 2473
MIN_LEN = 50
SALTS = (2, 3, 5, 7, 11, 13)


def bm(s, x, y, z):
    return V[V[V[V[s] ^ x] ^ y] ^ z]


def lcap(n: int) -> int:
    """The length class before it is cut to a byte (float64, as the published implementation computes it)."""
    ln = math.log(n)
    if n <= 656:
        return math.floor(ln / 0.4054651)
    if n <= 3199:
        return math.floor(ln / 0.26236426 - 8.72777)
    return math.floor(ln / 0.095310180 - 62.5472)


def lvalue(n: int) -> int:
    return lcap(n) & 255


def swap(b: int) -> int:
    return ((b & 15) << 4) | (b >> 4)


def buckets(data: bytes):
    """-> (counts int64 [128], checksum).  Vectorised over the window positions; the checksum chain stays a loop."""
    d = np.frombuffer(bytes(data), np.uint8)
    n = d.size
    if n < 5:
        return np.zeros(128, np.int64), 0
    a0, a1, a2, a3, a4 = d[4:], d[3:-1], d[2:-2], d[1:-3], d[:-4]

    def h(s, x, y, z):
        return _VN[_VN[_VN[np.uint8(V[s]) ^ x] ^ y] ^ z]

    cnt = np.zeros(256, np.int64)
    for s, x, y, z in ((2, a0, a1, a2), (3, a0, a1, a3), (5, a0, a2, a3), (7, a0, a2, a4), (11, a0, a1, a4), (13, a0, a3, a4)):
        cnt += np.bincount(h(s, x, y, z), minlength=256)
    t = _VN[_VN[np.uint8(1) ^ a0] ^ a1].tolist()
    ck = 0
    for ti in t:
        ck = V[ti ^ ck]
    return cnt[:128], ck


def nonzero_buckets(data: bytes) -> int:
    return int(np.count_nonzero(buckets(data)[0]))


def digest(data: bytes):
    """-> 35 bytes, or None when the document is refused (shorter than 50 bytes, or at most 64 non-zero buckets)."""
    n = len(data)
    if n < MIN_LEN:
        return None
    cnt, ck = buckets(data)
    if np.count_nonzero(cnt) <= 64:
        return None
    s = np.sort(cnt)
    q1, q2, q3 = int(s[31]), int(s[63]), int(s[95])
    cls = (cnt > q1).astype(np.uint8) + (cnt > q2) + (cnt > q3)
    code = [int(cls[4 * i]) | int(cls[4 * i + 1]) << 2 | int(cls[4 * i + 2]) << 4 | int(cls[4 * i + 3]) << 6 for i in range(32)]
    qa, qb = (q1 * 100 // q3) % 16, (q2 * 100 // q3) % 16
    return bytes([swap(ck), swap(lvalue(n)), (qa << 4) | qb] + code[::-1])


def digest_batch(docs):
    """-> (uint8 [n, 35], int32 [n]): status 0 or -1, a refused record all zero."""
    out = np.zeros((len(docs), TLSH_BYTES), np.uint8)
    st = np.zeros(len(docs), np.int32)
    for i, d in enumerate(docs):
        g = digest(d)
        if g is None:
            st[i] = -1
        else:
            out[i] = np.frombuffer(g, np.uint8)
    return out, st


def hexdigest(dig: bytes) -> str:
    return "T1" + bytes(dig).hex().upper()


def _md(x, y, r):
    d = abs(x - y)
    return min(d, r - d)


def distance(a: bytes, b: bytes) -> int:
    a, b = bytes(a), bytes(b)
    d = 0
    ln = _md(swap(a[1]), swap(b[1]), 256)
    d += ln if ln <= 1 else 12 * ln
    for qa, qb in ((a[2] >> 4, b[2] >> 4), (a[2] & 15, b[2] & 15)):
        q = _md(qa, qb, 16)
        d += q if q <= 1 else 12 * (q - 1)
    d += 1 if a[0] != b[0] else 0
    for x, y in zip(a[3:], b[3:]):
        for j in range(4):
            e = abs(((x >> 2 * j) & 3) - ((y >> 2 * j) & 3))
            d += 6 if e == 3 else e
    return d


_PAIR = np.array([[6 if abs(a - b) == 3 else abs(a - b) for b in range(4)] for a in range(4)], np.int64)
_BYTE = np.zeros((256, 256), np.int64)
for _j in range(4):
    _x = (np.arange(256) >> 2 * _j) & 3
    _BYTE += _PAIR[_x[:, None], _x[None, :]]


def distance_matrix(queries: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """uint16 [nq, n] of distance(query, row): the same arithmetic as `distance`, one table look-up per body byte pair."""
    q = np.ascontiguousarray(queries, np.uint8).reshape(-1, TLSH_BYTES)
    r = np.ascontiguousarray(rows, np.uint8).reshape(-1, TLSH_BYTES)
    sw = lambda x: ((x & 15).astype(np.int64) << 4) | (x >> 4)   # noqa: E731
    out = np.zeros((q.shape[0], r.shape[0]), np.uint16)
    ln = np.abs(sw(q[:, 1])[:, None] - sw(r[:, 1])[None, :])
    ln = np.minimum(ln, 256 - ln)
    out += np.where(ln <= 1, ln, 12 * ln).astype(np.uint16)
    for f in (lambda x: (x >> 4).astype(np.int64), lambda x: (x & 15).astype(np.int64)):
        d = np.abs(f(q[:, 2])[:, None] - f(r[:, 2])[None, :])
        d = np.minimum(d, 16 - d)
        out += np.where(d <= 1, d, 12 * (d - 1)).astype(np.uint16)
    out += (q[:, 0][:, None] != r[:, 0][None, :])
    tab = _BYTE.astype(np.uint16).ravel()
    for c in range(3, TLSH_BYTES):
        out += tab[(q[:, c].astype(np.uint16)[:, None] << 8) | r[:, c][None, :]]
    return out


def topk_from_distances(ids, dm, k: int, max_distance=None):
    """Exact top-k by (distance, id) from a distance matrix [nq, n].  -> (ids uint64 [nq, k], dist uint32 [nq, k],
    scores float32 [nq, k], n uint32 [nq]); unused slots: id 2^64 - 1, dist 2^32 - 1, score -1."""
    ids = np.asarray(ids, np.uint64).reshape(-1)
    nq = dm.shape[0]
    o_ids = np.full((nq, k), 0xFFFFFFFFFFFFFFFF, np.uint64)
    o_d = np.full((nq, k), 0xFFFFFFFF, np.uint32)
    o_s = np.full((nq, k), -1.0, np.float32)
    o_n = np.zeros(nq, np.uint32)
    if ids.size == 0 or k == 0:
        return o_ids, o_d, o_s, o_n
    for i in range(nq):
        d = dm[i].astype(np.int64)
        keep = np.flatnonzero(d <= max_distance) if max_distance is not None else np.arange(d.size)
        if keep.size > k:   # everything up to the k-th distance can still be in the answer
            kth = np.partition(d[keep], k - 1)[k - 1]
            keep = keep[d[keep] <= kth]
        order = keep[np.lexsort((ids[keep], d[keep]))][:k]
        m = order.size
        o_ids[i, :m] = ids[order]
        o_d[i, :m] = d[order]
        o_s[i, :m] = (np.float32(MAX_DISTANCE) - d[order].astype(np.float32)) / np.float32(MAX_DISTANCE)
        o_n[i] = m
    return o_ids, o_d, o_s, o_n


def topk(ids, rows, queries, k: int, max_distance=None):
    """Exact top-k by (distance, id) of `rows` for every query digest; see topk_from_distances."""
    q = np.ascontiguousarray(queries, np.uint8).reshape(-1, TLSH_BYTES)
    r = np.ascontiguousarray(rows, np.uint8).reshape(-1, TLSH_BYTES)
    return topk_from_distances(ids, distance_matrix(q, r), k, max_distance)
