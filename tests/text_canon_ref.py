"""Plain-Python restatement of text mode RAW_UTF8: strict decode, M(c) and the classes through the
COMPILED table (ucfp_text_utab_lookup: host code, no device), the four-neighbour boundary rule, tokens.

    canon_bytes(doc: bytes) -> (token bytes, status)      what ucfp_text_canon_batch gives for one document
    tokens(s: str)          -> list of tokens, or None    None: the document goes back to the host (NEEDS_HOST)

and, for the sweeps of tests/test_text_canon_sweep_gpu.py: the contexts that read out a table entry, the expanders found
in the table, the dense documents built from them, and decide_map: in which step and round the kernels decide a code point.
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


# ---- the sweeps of tests/test_text_canon_sweep_gpu.py: contexts that read out a table entry, dense steps ----
# `c` alone, between letters, digits, Hebrew letters and Katakana, behind both apostrophes, before one, between `_`; the
# last two tell a digit from a letter (`1,c` joins only Numeric) and an apostrophe from both (`ac` joins all but it)
CONTEXTS = ("{c}", "a{c}a", "1{c}1", "'{c}", "’{c}", "א{c}'", "א{c}א", "カ{c}カ", "_{c}_", "1,{c}", "a{c}")


def context_document(c: str) -> bytes:
    """One document that reads out every field of c's table entry: the contexts joined by two spaces."""
    return "  ".join(t.replace("{c}", c) for t in CONTEXTS).encode("utf-8")


def context_signature(flags: int, cp: int = 0xE000) -> Tuple:
    """The tokens of every context for a stand-in canonical code point with these flags (class | alnum << 4 | vowel << 5):
    what the contexts can tell about an entry apart from the code point itself."""
    sig = []
    for t in CONTEXTS:
        x = []
        for ch in t.replace("{c}", "\0"):
            x.append((cp, flags) if ch == "\0" else (ord(ch), lookup(ord(ch))[1]))
        sig.append(tuple(stream_tokens(x)))
    return tuple(sig)


def canonical_flags() -> List[int]:
    """Every (class, alnum, vowel) that occurs among the table's canonical code points."""
    seen = set()
    for cp in range(0x20000):
        r = lookup(cp)
        if r is not None:
            seen.update(lookup(x)[1] for x in r[0])
    return sorted(seen)


_expanders = _quiet = None


def expanders() -> List[int]:
    """The covered code points that make the most canonical code points per source byte, found in the table: for every
    UTF-8 width the lowest code point with the most, the lowest at every count above the width, and the lowest with the
    most per byte among those whose canonical code points are all non-alphanumeric.  Densest first."""
    global _expanders, _quiet
    if _expanders is None:
        first, quiet = {}, None
        for cp in range(0x80, 0x20000):
            r = lookup(cp)
            if r is None or not r[0]:
                continue
            m, w = r[0], len(chr(cp).encode("utf-8", "surrogatepass"))
            first.setdefault((w, len(m)), cp)
            if not any(lookup(x)[1] & 16 for x in m) and (quiet is None or len(m) * quiet[1] > quiet[0] * w):
                quiet = (len(m), w, cp)
        top = {w: max(n for ww, n in first if ww == w) for w in (2, 3, 4)}
        picked = {cp for (w, n), cp in first.items() if n == top[w] or n > w} | {quiet[2]}
        _quiet = quiet[2]
        _expanders = sorted(picked, key=lambda cp: (-len(lookup(cp)[0]) / len(chr(cp).encode("utf-8")), cp))
    return _expanders


def quiet_expander() -> int:
    """The one of expanders() whose canonical code points are all non-alphanumeric."""
    expanders()
    return _quiet


def joining_expander() -> int:
    """The densest covered code point whose canonical code points are all letters or digits that join: copies of it are
    one token."""
    best = None
    for cp in range(0x80, 0x20000):
        r = lookup(cp)
        if r is None or len(r[0]) < 2 or not all(lookup(x)[1] & 15 == ALETTER and lookup(x)[1] & 16 for x in r[0]):
            continue
        d = len(r[0]) / len(chr(cp).encode("utf-8"))
        if best is None or d > best[0]:
            best = (d, cp)
    return best[1]


def decide_map(doc: bytes):
    """Where the canon kernels decide each canonical code point of a covered document: a step is 64 source bytes, a step
    decides the code point the step before left undecided and all of its own but the last (the last step: all), 64 a
    round.  -> [(step, index within the step's decided code points, boundary before it, its segment is a token, alphanumeric)]."""
    s = doc.decode("utf-8", "strict")
    x, made, at = [], {}, 0
    for ch in s:
        m, fl = lookup(ord(ch))
        for cp in m:
            x.append((cp, fl if len(m) == 1 else lookup(cp)[1]))
        made[at // 64] = made.get(at // 64, 0) + len(m)
        at += len(ch.encode("utf-8"))
    last = (len(doc) - 1) // 64
    where, done, seen = [], 0, 0          # done: decided before this step; seen: made up to and including it
    for step in range(last + 1):
        seen += made.get(step, 0)
        upto = seen if step == last else max(seen - 1, 0)
        where += [(step, g - done) for g in range(done, upto)]
        done = upto
    bnd = [i == 0 or not _joined(x, i) for i in range(len(x))]
    kept, i = [False] * len(x), 0
    while i < len(x):
        j = i + 1
        while j < len(x) and not bnd[j]:
            j += 1
        kept[i:j] = [any(fl & 16 for _, fl in x[i:j])] * (j - i)
        i = j
    return [(st, idx, bnd[g], kept[g], bool(x[g][1] & 16)) for g, (st, idx) in enumerate(where)]


def dense_copies(cp: int) -> List[bytes]:
    """n copies of an expander, alone and behind 1 .. 63 bytes of `x `: 64 source bytes make up to 132 canonical code points."""
    e = chr(cp).encode("utf-8")
    return [(b"x " * 32)[:lead] + e * n for n in (21, 22, 43, 44, 100, 400) for lead in range(64)]


def dense_dots() -> List[bytes]:
    """Runs of the densest non-alphanumeric expander closed by a letter: every code point a dropped segment, then one token."""
    e = chr(quiet_expander()).encode("utf-8")
    return [e * n + tail for n in list(range(1, 71)) + [100, 200] for tail in (b"a", b" a")]


def dense_open_segments(form: int) -> List[bytes]:
    """p expanders, r underscores, then ` x`, `a` or nothing: the run of `_` is a segment without an alphanumeric that opens in
    one round of a step and closes, as a token (`a`) or dropped, in a later round or in the next step.  form 0: the
    non-alphanumeric expander before it; 1: the densest and a space; 2: the densest, whose last digit the run joins."""
    e = chr(quiet_expander() if form == 0 else expanders()[0]).encode("utf-8")
    sep = b" " if form == 1 else b""
    return [e * p + sep + b"_" * r + tail for p in range(23) for r in range(1, 71) for tail in (b" x", b"a", b"")]


def dense_mixed(n: int = 48, seed: int = 9) -> List[bytes]:
    """Expanders (at least half of the source bytes), ASCII words, CJK and Cf runs, drawn at random."""
    import random
    rng = random.Random(seed)
    ex = [chr(cp) for cp in expanders()]
    other = ["word", "it's", " ", "  ", "_", "__ ", "1,5", "a.b", "日本", "カタ", "漢",
             "​‍", "­" * 5, "א\"ב", "’e", "x"]
    docs = []
    for _ in range(n):
        parts, dense, total = [], 0, 0
        for _ in range(rng.randint(8, 90)):
            if 2 * dense <= total or rng.random() < 0.6:
                p = rng.choice(ex) * rng.randint(1, 30)
                dense += len(p.encode("utf-8"))
            else:
                p = rng.choice(other)
            parts.append(p)
            total += len(p.encode("utf-8"))
        docs.append("".join(parts).encode("utf-8"))
    return docs
