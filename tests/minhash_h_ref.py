"""Plain-Python restatement of MinHash with any slot count H and of the search over such records.

    minhash_tokens_h(tokens, k, h)   T3-T5 continued to h slots: slot i = min over the shingles of h1 + i * h2 mod 2^64
                                                                        -> (8 + 8 h bytes, status)
    agree_h(a, b, h)                 the number of i < h with slot_i(a) == slot_i(b); the headers take no part
    slots_of / records_of            uint8 [n, 8 + 8 h] <-> uint64 [n, h]
    topk_h(ids, rows, queries, h, k, min_agree)   hits agree >= min_agree, order (agree desc, id asc), first k,
                                                   score = float32(agree) / float32(h)

The shingles and XXH3 are those of tests/text_grapheme_ref.py; nothing here knows the kernels.
"""
from typing import Sequence, Tuple

import numpy as np

from text_grapheme_ref import E_MODALITY, _mix_h2, shingles, xxh3

INVALID_ID = 0xFFFFFFFFFFFFFFFF
EMPTY32 = 0xFFFFFFFF
VALID_H = tuple(range(16, 1025, 16))


def record_bytes(h: int) -> int:
    return 8 + 8 * h


def minhash_tokens_h(tokens: Sequence[bytes], k: int, h: int) -> Tuple[bytes, int]:
    sh = shingles(tokens, k)
    if not sh:
        return bytes(record_bytes(h)), E_MODALITY
    with np.errstate(over="ignore"):
        h1 = np.array([xxh3(s) for s in sh], np.uint64)
        h2 = _mix_h2(h1)
        slots = (h1[:, None] + np.arange(h, dtype=np.uint64)[None, :] * h2[:, None]).min(axis=0)
    rec = np.zeros(record_bytes(h), np.uint8)
    rec[0] = 1
    rec[8:] = slots.astype("<u8").view(np.uint8)
    return rec.tobytes(), 0


def slots_of(records, h: int) -> np.ndarray:
    r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, record_bytes(h))
    return np.ascontiguousarray(r[:, 8:]).view("<u8").reshape(-1, h)


def records_of(slots, h: int, header=None) -> np.ndarray:
    s = np.ascontiguousarray(slots, dtype="<u8").reshape(-1, h)
    out = np.zeros((s.shape[0], record_bytes(h)), np.uint8)
    out[:, 0] = 1
    if header is not None:
        out[:, :8] = header
    out[:, 8:] = s.view(np.uint8).reshape(-1, 8 * h)
    return out


def agree_h(a, b, h: int) -> int:
    sa = slots_of(np.frombuffer(bytes(a), np.uint8), h)[0]
    sb = slots_of(np.frombuffer(bytes(b), np.uint8), h)[0]
    return int((sa == sb).sum())


def agree_matrix(queries, rows, h: int) -> np.ndarray:
    q, r = slots_of(queries, h), slots_of(rows, h)
    out = np.zeros((q.shape[0], r.shape[0]), np.int64)
    for i in range(q.shape[0]):
        out[i] = (r == q[i][None, :]).sum(axis=1)
    return out


def topk_from_agree(ids, A, h: int, k: int, min_agree: int = 1):
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
        o_sc[q, :m] = A[q, order].astype(np.float32) / np.float32(h)
        o_n[q] = m
    return o_ids, o_ag, o_sc, o_n


def topk_h(ids, rows, queries, h: int, k: int, min_agree: int = 1):
    return topk_from_agree(ids, agree_matrix(queries, rows, h), h, k, min_agree)
