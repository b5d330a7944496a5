"""Numpy restatement of MinHash search: a record is 1032 bytes, 8 header bytes that take no part and 128 u64
LE slots; agree(q, r) = the number of slot positions at which the two records hold the same 64 bits; hits are the rows with
agree >= min_agree in the order (agree descending, id ascending), the first k; score = float32(agree) / 128."""
import numpy as np

RECORD_BYTES = 1032
SLOTS = 128
INVALID_ID = 0xFFFFFFFFFFFFFFFF
EMPTY32 = 0xFFFFFFFF


def slots_of(records) -> np.ndarray:
    """uint8 [n, 1032] -> uint64 [n, 128]."""
    r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
    return np.ascontiguousarray(r[:, 8:]).view("<u8").reshape(-1, SLOTS)


def records_of(slots, header=None) -> np.ndarray:
    """uint64 [n, 128] -> uint8 [n, 1032] with the header the reference writes (schema 1, 6 zero bytes) or `header`."""
    s = np.ascontiguousarray(slots, dtype="<u8").reshape(-1, SLOTS)
    out = np.zeros((s.shape[0], RECORD_BYTES), np.uint8)
    out[:, 0] = 1
    if header is not None:
        out[:, :8] = header
    out[:, 8:] = s.view(np.uint8).reshape(-1, SLOTS * 8)
    return out


def agree_matrix(queries, rows) -> np.ndarray:
    """uint8 [nq, 1032], uint8 [n, 1032] -> int64 [nq, n]."""
    q, r = slots_of(queries), slots_of(rows)
    out = np.zeros((q.shape[0], r.shape[0]), np.int64)
    for i in range(q.shape[0]):
        out[i] = (r == q[i][None, :]).sum(axis=1)
    return out


def topk_from_agree(ids, A, k, min_agree=1):
    """-> (ids u64 [nq, k], agree u32 [nq, k], scores f32 [nq, k], counts u32 [nq]); unused places carry 2^64 - 1,
    2^32 - 1 and -1."""
    ids = np.asarray(ids, np.uint64).reshape(-1)
    A = np.asarray(A, np.int64)
    if A.ndim == 1:
        A = A[None, :]
    nq = A.shape[0]
    o_ids = np.full((nq, k), INVALID_ID, np.uint64)
    o_ag = np.full((nq, k), EMPTY32, np.uint32)
    o_sc = np.full((nq, k), -1.0, np.float32)
    o_n = np.zeros(nq, np.uint32)
    for q in range(nq):
        hit = np.flatnonzero(A[q] >= min_agree)
        order = hit[np.lexsort((ids[hit], -A[q, hit]))][:k]
        m = order.size
        o_ids[q, :m] = ids[order]
        o_ag[q, :m] = A[q, order].astype(np.uint32)
        o_sc[q, :m] = A[q, order].astype(np.float32) / np.float32(128.0)
        o_n[q] = m
    return o_ids, o_ag, o_sc, o_n
