"""Plain-Python restatement of TF.IDF SimHash, in Python ints only.

    log2_q16(x)                      T9.4's L: integer log2 in Q16 (this function IS the definition)
    weight_q16(n_docs, df)           T9.4: 0x10000 + L(N + 1) - L(df + 1)
    key(token)                       T9.1: XXH3-64 of the canonical token bytes
    fit(docs_tokens)                 T9.4: (N, {key: df}) over documents given as token lists (None: status != 0, adds nothing)
    weights_of(N, dfs)               -> ({key: weight}, default)
    simhash_weighted(tokens, weights, default)   T9.3 -> (8 bytes, status)
    words(doc, mode) / graphemes(doc, mode)      the token lists of the device routes, from what the tree already has

Tokens come from oracle.text_canon (mode 0 words), text_canon_ref (mode 2 words) and text_grapheme_ref.device_clusters.
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import oracle

import text_canon_ref as canon_ref
import text_grapheme_ref as gref

RAW_ASCII, PRETOKENIZED, RAW_UTF8 = 0, 1, 2
E_MODALITY = -1
Q16_ONE = 0x10000
MAX_WINDOW_BYTES = 1405


def log2_q16(x: int) -> int:                 # 1 <= x < 2**64
    n = x.bit_length() - 1
    y = x << (63 - n)            # Q1.63 in [2**63, 2**64)
    r = n << 16
    for i in range(16):
        y = (y * y) >> 63
        if y >> 64:
            y >>= 1
            r |= 1 << (15 - i)
    return r


def weight_q16(n_docs: int, df: int) -> int:
    return (Q16_ONE + log2_q16(n_docs + 1) - log2_q16(df + 1)) & 0xFFFFFFFF


def key(token: bytes) -> int:
    return gref.xxh3(bytes(token))


def fit(docs_tokens: Iterable[Optional[Sequence[bytes]]]) -> Tuple[int, Dict[int, int]]:
    """N = documents with at least one token; df per key.  None (or no token) = a document whose status is not 0."""
    n, df = 0, {}
    for toks in docs_tokens:
        toks = [bytes(t) for t in (toks or []) if len(t)]
        if not toks:
            continue
        n += 1
        for k in {key(t) for t in toks}:
            df[k] = df.get(k, 0) + 1
    return n, df


def weights_of(n_docs: int, dfs: Dict[int, int]) -> Tuple[Dict[int, int], int]:
    return {k: weight_q16(n_docs, d) for k, d in dfs.items()}, weight_q16(n_docs, 0)


def simhash_weighted(tokens: Sequence[bytes], weights: Dict[int, int], default: int) -> Tuple[bytes, int]:
    toks = [bytes(t) for t in tokens if len(t)]
    if not toks:
        return bytes(8), E_MODALITY
    pos, tot = [0] * 64, 0
    for t in toks:
        k = key(t)
        w = weights.get(k, default)
        tot += w
        for b in range(64):
            if (k >> b) & 1:
                pos[b] += w
    if tot == 0:
        return bytes(8), E_MODALITY
    bits = 0
    for b in range(64):
        if 2 * pos[b] > tot:
            bits |= 1 << b
    return bits.to_bytes(8, "little"), 0


def words(doc: bytes, mode: int) -> Optional[List[bytes]]:
    """The word tokens of a document on the device route `mode`, None when it is handed back."""
    if mode == PRETOKENIZED:
        return [t for t in doc.split(b" ") if t]
    if mode == RAW_ASCII:
        if any(b >= 0x80 for b in doc):
            return None
        stream, nt = oracle.text_canon(doc, 0)
        return [t for t in stream.split(b" ") if t] if nt > 0 else []
    stream, st = canon_ref.canon_bytes(doc)
    return None if st != 0 else [t for t in stream.split(b" ") if t]


def graphemes(doc: bytes, mode: int) -> Optional[List[bytes]]:
    return gref.device_clusters(doc, mode)
