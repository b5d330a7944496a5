"""Plain-Python restatement of the grapheme tokeniser and of caller-segmented tokens.

    host_clusters(s)            the host route: Canonicalizer().apply, then \\X            -> list of token bytes
    device_clusters(doc, mode)  the device rule: G1 canonical stream, one cluster per canonical code point, CR LF one,
                                the G3 hand-back                                            -> list of token bytes, or None
    minhash_tokens(tokens, k)   G5 + T4 + T5 over any token list (G7: empty tokens are none) -> (1032 bytes, status)
    simhash_tokens(tokens)      T6                                                          -> (8 bytes, status)
    grapheme_minhash / grapheme_simhash(doc, mode[, k])   what ucfp_text_*_batch_ex(GRAPHEME) gives for one document

Hashes come from `xxhash` where it is installed and from the oracle's XXH3 otherwise; slots and bits are numpy.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np

import oracle
from ucfp_amd import _lib
from ucfp_amd.text import Canonicalizer

import text_canon_ref as canon_ref

RAW_ASCII, PRETOKENIZED, RAW_UTF8 = 0, 1, 2
TOK_WORD, TOK_GRAPHEME = 0, 1
NEEDS_HOST, E_MODALITY, E_UNSUPPORTED, E_INVALID = 1, -1, -2, -4
MINHASH_BYTES, SIMHASH_BYTES = 1032, 8
EXCLUDED_GCB = ("Prepend", "L", "V", "T")

try:
    import xxhash
    _xxh3 = xxhash.xxh3_64_intdigest
except ImportError:                                   # pragma: no cover
    _xxh3 = oracle.xxh3_64


def xxh3(b: bytes) -> int:
    return _xxh3(bytes(b))


def covered(cp: int) -> bool:
    """ucfp_text_grapheme_covered: host code, no device."""
    return bool(_lib.load().ucfp_text_grapheme_covered(cp))


def host_clusters(s: str, canon: Optional[Canonicalizer] = None) -> List[bytes]:
    import regex
    return [g.encode("utf-8", "surrogatepass") for g in regex.findall(r"\X", (canon or Canonicalizer()).apply(s))]


def canonical_stream(doc: bytes, mode: int) -> Optional[List[int]]:
    """G1: the canonical code points, or None when the document is handed back (G3)."""
    if mode == RAW_ASCII:
        if any(b >= 0x80 for b in doc):
            return None
        return [b + 32 if 0x41 <= b <= 0x5A else b for b in doc]
    try:
        s = doc.decode("utf-8", "strict")             # U2
    except UnicodeDecodeError:
        return None
    out = []
    for ch in s:
        if not covered(ord(ch)):
            return None
        out.extend(canon_ref.lookup(ord(ch))[0])      # U3: M(c) through the compiled table
    return out


def device_clusters(doc: bytes, mode: int) -> Optional[List[bytes]]:
    """G2 over the device set: one cluster per canonical code point, CR immediately followed by LF one cluster."""
    x = canonical_stream(doc, mode)
    if x is None:
        return None
    out, i = [], 0
    while i < len(x):
        if x[i] == 0x0D and i + 1 < len(x) and x[i + 1] == 0x0A:
            out.append(b"\r\n")
            i += 2
        else:
            out.append(chr(x[i]).encode("utf-8"))
            i += 1
    return out


def _mix_h2(h1: np.ndarray) -> np.ndarray:
    z = h1 + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return (z ^ (z >> np.uint64(31))) | np.uint64(1)


def shingles(tokens: Sequence[bytes], k: int) -> List[bytes]:
    """G5 / T3: k consecutive tokens joined by one 0x20; fewer than k tokens: one shingle of all of them."""
    toks = [bytes(t) for t in tokens if len(t)]       # G7: an empty token is not a token
    if not toks:
        return []
    if len(toks) < k:
        return [b" ".join(toks)]
    return [b" ".join(toks[i:i + k]) for i in range(len(toks) - k + 1)]


def minhash_tokens(tokens: Sequence[bytes], k: int) -> Tuple[bytes, int]:
    sh = shingles(tokens, k)
    if not sh:
        return bytes(MINHASH_BYTES), E_MODALITY
    with np.errstate(over="ignore"):
        h1 = np.array([xxh3(s) for s in sh], np.uint64)
        h2 = _mix_h2(h1)
        slots = (h1[:, None] + np.arange(128, dtype=np.uint64)[None, :] * h2[:, None]).min(axis=0)
    rec = np.zeros(MINHASH_BYTES, np.uint8)
    rec[0] = 1
    rec[8:] = slots.astype("<u8").view(np.uint8)
    return rec.tobytes(), 0


def simhash_tokens(tokens: Sequence[bytes]) -> Tuple[bytes, int]:
    toks = [bytes(t) for t in tokens if len(t)]
    if not toks:
        return bytes(SIMHASH_BYTES), E_MODALITY
    h = np.array([xxh3(t) for t in toks], np.uint64)
    ones = ((h[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).sum(axis=0)
    bits = 0
    for b in range(64):
        if 2 * int(ones[b]) > len(toks):
            bits |= 1 << b
    return bits.to_bytes(8, "little"), 0


def grapheme_minhash(doc: bytes, mode: int, k: int) -> Tuple[bytes, int]:
    t = device_clusters(doc, mode)
    return (bytes(MINHASH_BYTES), NEEDS_HOST) if t is None else minhash_tokens(t, k)


def grapheme_simhash(doc: bytes, mode: int) -> Tuple[bytes, int]:
    t = device_clusters(doc, mode)
    return (bytes(SIMHASH_BYTES), NEEDS_HOST) if t is None else simhash_tokens(t)


def pack_tokens(docs: Sequence[Sequence[bytes]]):
    """-> (blob uint8, tok_offsets uint64 [T + 1], doc_tokens uint64 [n + 1])."""
    toks = [bytes(t) for d in docs for t in d]
    to = np.zeros(len(toks) + 1, np.uint64)
    np.cumsum([len(t) for t in toks], out=to[1:])
    dt = np.zeros(len(docs) + 1, np.uint64)
    np.cumsum([len(d) for d in docs], out=dt[1:])
    return np.frombuffer(b"".join(toks) + b"\0" * 16, np.uint8).copy(), to, dt


_gcb_pats = None


def gcb_excluded(ch: str) -> bool:
    """Grapheme_Cluster_Break of ch in {Prepend, L, V, T}, probed from `regex`."""
    global _gcb_pats
    import regex
    if _gcb_pats is None:
        _gcb_pats = regex.compile(r"[\p{GCB=Prepend}\p{GCB=L}\p{GCB=V}\p{GCB=T}]")
    return bool(_gcb_pats.match(ch))
