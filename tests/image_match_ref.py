"""numpy restatement of the image match spec: the reference the C function and the GPU index are
compared with, bit for bit.  Every f32 product and sum is one numpy float32 operation, in the order M2-M3 fix."""
from dataclasses import dataclass

import numpy as np

INVALID_ID = 0xFFFFFFFFFFFFFFFF
F = np.float32


@dataclass
class Cfg:
    """M4, with its defaults."""
    ahash_weight: float = 0.1
    phash_weight: float = 0.6
    dhash_weight: float = 0.3
    global_weight: float = 0.4
    block_weight: float = 0.6
    block_distance_threshold: int = 32
    min_score: float = 0.0


def codes(records) -> np.ndarray:
    """M1: uint8 [n, 168] -> uint64 [n, 1, 17]; uint8 [n, 536] -> uint64 [n, 3, 17] (ahash, phash, dhash); code 0 is the
    global hash, codes 1 .. 16 the blocks."""
    r = np.ascontiguousarray(records, dtype=np.uint8)
    if r.ndim == 1:
        r = r[None]
    n, size = r.shape
    if size == 168:
        starts = [32]
    elif size == 536:
        starts = [64, 232, 400]
    else:
        raise ValueError(f"not an image record: {size} bytes")
    out = np.empty((n, len(starts), 17), np.uint64)
    for a, s in enumerate(starts):
        out[:, a, :] = np.ascontiguousarray(r[:, s:s + 136]).view("<u8")
    return out


def _popcount(x: np.ndarray) -> np.ndarray:
    """Bits set in every uint64 (the sideways addition of pairs, nibbles, bytes), as uint32."""
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.uint32)


def score_matrix(queries, rows, cfg: Cfg = None) -> np.ndarray:
    """M2-M3: float32 [nq, n]."""
    cfg = cfg or Cfg()
    cq, cr = codes(queries), codes(rows)
    if cq.shape[1] != cr.shape[1]:
        raise ValueError("queries and rows are records of different sizes")
    T = np.uint32(cfg.block_distance_threshold)
    wg, wb = F(cfg.global_weight), F(cfg.block_weight)
    s = []
    for a in range(cq.shape[1]):
        d = _popcount(cq[:, None, a, :] ^ cr[None, :, a, :])            # [nq, n, 17]
        g = d[..., 0]
        db = d[..., 1:]
        S = np.where(db <= T, np.uint32(64) - db, np.uint32(0)).sum(axis=-1, dtype=np.uint32)
        sg = (np.uint32(64) - g).astype(F) * F(0.015625)
        sb = S.astype(F) * F(0.0009765625)
        s.append((wg * sg) + (wb * sb))
    if len(s) == 1:
        return s[0].astype(F)
    wa, wp, wd = F(cfg.ahash_weight), F(cfg.phash_weight), F(cfg.dhash_weight)
    return (((wa * s[0]) + (wp * s[1])) + (wd * s[2])).astype(F)


def topk(ids, scores, k: int, min_score: float = 0.0):
    """M5 for one query: scores float32 [n] against ids [n] -> (ids uint64 [k], scores float32 [k], count); rows with
    score >= min_score, ordered (score desc, id asc); unused places carry INVALID_ID and -1."""
    ids = np.asarray(ids, np.uint64)
    scores = np.asarray(scores, F)
    keep = np.nonzero(scores >= F(min_score))[0]
    order = keep[np.lexsort((ids[keep], -scores[keep].astype(np.float64)))][:k]
    out_ids = np.full(k, INVALID_ID, np.uint64)
    out_sc = np.full(k, -1.0, F)
    out_ids[:order.size] = ids[order]
    out_sc[:order.size] = scores[order]
    return out_ids, out_sc, int(order.size)


def search(ids, rows, queries, k: int, cfg: Cfg = None):
    """The whole query: (ids [nq, k], scores [nq, k], counts [nq])."""
    cfg = cfg or Cfg()
    sm = score_matrix(queries, rows, cfg)
    res = [topk(ids, sm[q], k, cfg.min_score) for q in range(sm.shape[0])]
    return (np.array([r[0] for r in res], np.uint64).reshape(-1, k), np.array([r[1] for r in res], F).reshape(-1, k),
            np.array([r[2] for r in res], np.uint32))
