"""Plain-Python restatement of the BM25 terms rule, shared by the BM25 terms tests.

    is_word(b)            A23.1: the byte is in [0-9A-Za-z]
    tokens(doc)           the maximal runs of word bytes, A-Z lower-cased -- a byte loop, not terms.tokenize
    key(token)            A23.2: XXH3_64 of the token's bytes, seed 0 (text_grapheme_ref.xxh3)
    doc_terms(doc, form)  A23.3/4 for one document: (status, keys, tfs); a dict counts, the keys are then sorted
    batch(docs, form)     what ucfp_bm25_terms_batch gives for a list of documents: (keys, tfs, pair_offsets, status)
    batch_offsets(blob, offsets, n_bytes, form)   the same for an offset table as the entry takes it, bad offsets included
"""
from typing import List, Tuple

import numpy as np

from text_grapheme_ref import xxh3

COUNTS, SEQUENCE = 0, 1
NEEDS_HOST, E_UNSUPPORTED, E_INVALID = 1, -2, -4
MAX_WINDOW_BYTES = 1405          # UCFP_TEXT_MAX_WINDOW_BYTES


def is_word(b: int) -> bool:
    return 0x30 <= b <= 0x39 or 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A


def tokens(doc: bytes) -> List[bytes]:
    out, cur = [], bytearray()
    for b in doc:
        if is_word(b):
            cur.append(b + 32 if 0x41 <= b <= 0x5A else b)
        elif cur:
            out.append(bytes(cur))
            cur = bytearray()
    if cur:
        out.append(bytes(cur))
    return out


def key(token: bytes) -> int:
    return xxh3(token)


def doc_terms(doc: bytes, form: int, long_status: int = E_UNSUPPORTED) -> Tuple[int, List[int], List[int]]:
    """long_status: what a document with a token above MAX_WINDOW_BYTES gets (the entry may give 0 or -2)."""
    if any(b >= 0x80 for b in doc):
        return NEEDS_HOST, [], []
    toks = tokens(doc)
    if long_status and any(len(t) > MAX_WINDOW_BYTES for t in toks):
        return long_status, [], []
    ks = [key(t) for t in toks]
    if form == SEQUENCE:
        return 0, ks, []
    counts = {}
    for k in ks:
        counts[k] = counts.get(k, 0) + 1
    ks = sorted(counts)
    return 0, ks, [counts[k] for k in ks]


def _pack(rows, form):
    keys, tfs, po, status = [], [], [0], []
    for st, ks, ts in rows:
        status.append(st)
        keys += ks
        tfs += ts
        po.append(len(keys))
    return (np.array(keys, np.uint64), np.array(tfs if form == COUNTS else [], np.uint32), np.array(po, np.uint64),
            np.array(status, np.int32))


def batch(docs, form: int, long_status: int = E_UNSUPPORTED):
    return _pack([doc_terms(d, form, long_status) for d in docs], form)


def batch_offsets(blob: bytes, offsets, n_bytes: int, form: int):
    """A23.4: document i is refused (-4) when its offsets decrease, reach past n_bytes or begin below an earlier offset."""
    rows, pmax = [], 0
    for i in range(len(offsets) - 1):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        pmax = max(pmax, o0)
        rows.append((E_INVALID, [], []) if (pmax != o0 or o1 < o0 or o1 > n_bytes) else doc_terms(blob[o0:o1], form))
    return _pack(rows, form)
