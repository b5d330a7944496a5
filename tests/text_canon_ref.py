"""Plain-Python restatement of text mode RAW_UTF8: strict decode, M(c) and the classes through the
COMPILED table (ucfp_text_utab_lookup: host code, no device), the four-neighbour boundary rule, tokens.

    canon_bytes(doc: bytes) -> (token bytes, status)      what ucfp_text_canon_batch gives for one document
    tokens(s: str)          -> list of tokens, or None    None: the document goes back to the host (NEEDS_HOST)
"""
import ctypes as C
from typing import List, Optional, Tuple

from ucfp_amd import _lib

NEEDS_HOST = 1
(OTHER, ALETTER, HEBREW, NUMERIC, KATAKANA, EXTNUMLET, MIDLETTER, MIDNUM, MIDNUMLET, SQUOTE, DQUOTE) = range(11)
AHL = {ALETTER, HEBREW}
MIDL = {MIDLETTER, MIDNUMLET, SQUOTE}
MIDN = {MIDNUM, MIDNUMLET, SQUOTE}
APOSTROPHES = {0x27, 0x2019}

_cache = {}


def lookup(cp: int):
    """-> None for an uncovered code point, else (M(cp) as a tuple of code points, flags); flags (class | alnum << 4 |
    vowel << 5) describe M(cp) when it is one code point."""
    r = _cache.get(cp, 0)
    if r == 0:
        out = (C.c_uint32 * 8)()
        n, fl = C.c_uint32(0), C.c_uint32(0)
        r = (tuple(out[:n.value]), fl.value) if _lib.load().ucfp_text_utab_lookup(cp, out, C.byref(n), C.byref(fl)) else None
        _cache[cp] = r
    return r


def table_versions() -> Tuple[str, str]:
    """(unicodedata version, regex version) the compiled table is bound to."""
    w = _lib.load().ucfp_text_utab_versions().decode().split()
    return w[1], w[3]


def canonical(cps) -> Optional[List[Tuple[int, int]]]:
    """U3: the canonical stream as (code point, flags); None if a code point is not covered."""
    out = []
    for cp in cps:
        r = lookup(cp)
        if r is None:
            return None
        m, fl = r
        if len(m) == 1:
            out.append((m[0], fl))
        else:
            for x in m:
                mx, fx = lookup(x)
                assert mx == (x,)          # M is idempotent on its outputs
                out.append((x, fx))
    return out


def _joined(x, i) -> bool:
    """U4: no boundary before x[i] (i >= 1)."""
    def cls(j):
        return x[j][1] & 15 if 0 <= j < len(x) else None
    aa, a, b, bb = cls(i - 2), cls(i - 1), cls(i), cls(i + 1)
    return ((a in AHL and b in AHL)
            or (a in AHL and b in MIDL and bb in AHL)
            or (aa in AHL and a in MIDL and b in AHL)
            or (a == HEBREW and b == SQUOTE)
            or (a == HEBREW and b == DQUOTE and bb == HEBREW)
            or (aa == HEBREW and a == DQUOTE and b == HEBREW)
            or (a == NUMERIC and b == NUMERIC)
            or (a in AHL and b == NUMERIC)
            or (a == NUMERIC and b in AHL)
            or (aa == NUMERIC and a in MIDN and b == NUMERIC)
            or (a == NUMERIC and b in MIDN and bb == NUMERIC)
            or (a == KATAKANA and b == KATAKANA)
            or (a in AHL | {NUMERIC, KATAKANA, EXTNUMLET} and b == EXTNUMLET)
            or (a == EXTNUMLET and b in AHL | {NUMERIC, KATAKANA})
            or (x[i - 1][0] in APOSTROPHES and bool(x[i][1] & 32)))


def stream_tokens(x) -> List[str]:
    """U5: the segments of the canonical stream that hold an alphanumeric."""
    out, cur, alnum = [], [], False
    for i, (cp, fl) in enumerate(x):
        if i and not _joined(x, i):
            if alnum:
                out.append("".join(map(chr, cur)))
            cur, alnum = [], False
        cur.append(cp)
        alnum = alnum or bool(fl & 16)
    if alnum:
        out.append("".join(map(chr, cur)))
    return out


def tokens(s: str) -> Optional[List[str]]:
    x = canonical(map(ord, s))
    return None if x is None else stream_tokens(x)


def canon_bytes(doc: bytes) -> Tuple[bytes, int]:
    try:
        s = doc.decode("utf-8", "strict")      # U2: overlong forms, surrogates, > 0x10FFFF, stray and cut sequences all raise
    except UnicodeDecodeError:
        return b"", NEEDS_HOST
    t = tokens(s)
    if t is None:
        return b"", NEEDS_HOST
    return " ".join(t).encode("utf-8"), 0


# ---- the random documents of the tests: a quarter everyday ASCII and quotes, the rest uniform over the CLASSES ----
EVERYDAY = "abeZ09 _.,':;\"-\n\u2019\u00e9"
_pools = None


def class_pools():
    """Covered code points grouped by the class of the first code point of M(c) ("empty" for the deleted ones)."""
    global _pools
    if _pools is None:
        pools = {}
        for cp in range(0x20000):
            r = lookup(cp)
            if r is None:
                continue
            m, fl = r
            key = "empty" if not m else (fl & 15 if len(m) == 1 else lookup(m[0])[1] & 15)
            pools.setdefault(key, []).append(cp)
        _pools = [pools[k] for k in sorted(pools, key=str)]
    return _pools


def random_string(rng, lo: int, hi: int) -> str:
    """`rng` is a random.Random; lo .. hi code points."""
    pools = class_pools()
    out = []
    for _ in range(rng.randint(lo, hi)):
        if rng.random() < 0.25:
            out.append(rng.choice(EVERYDAY))
        else:
            out.append(chr(rng.choice(rng.choice(pools))))
    return "".join(out)
