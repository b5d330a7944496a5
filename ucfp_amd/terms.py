"""BM25 tokenizer -- the reference's `tokenize` (src/index/embedded/bm25.rs:88-97), DESIGN A11.

Split on every char that is not `char::is_alphanumeric()`, drop empty chunks, lower-case each chunk with
`str::to_lowercase`.  Rust's predicate is the Unicode Alphabetic property or a general category of N*; Python's
str.isalnum() misses the Other_Alphabetic characters (U+24B6 'Ⓐ', U+0903 'ः', ...), so the split uses the committed
range table of _alnum_table.py (tools/gen_alnum_table.py).

Unicode-version skew: the table follows the Unicode version of the `regex` module that generated it (16 or later),
while str.lower() follows this Python's unicodedata (13.0 here) and Rust's to_lowercase the toolchain's own.  Letters
added after 13.0 with a lower-case mapping may therefore lower-case differently; every other character agrees.
Both lower-casings apply Final_Sigma ('Σ' at the end of a word becomes 'ς') and map 'İ' to 'i' + U+0307."""
import re
from typing import Iterable, List

from ._alnum_table import RANGES


def _char_class() -> str:
    def esc(cp: int) -> str:
        return f"\\U{cp:08X}"
    return "[" + "".join(esc(a) if a == b else f"{esc(a)}-{esc(b)}" for a, b in RANGES) + "]+"


_WORD = re.compile(_char_class())


def is_alphanumeric(ch: str) -> bool:
    """Rust's char::is_alphanumeric for one character."""
    return _WORD.fullmatch(ch) is not None


def tokenize(s: str) -> List[str]:
    """bm25.rs `tokenize`: the maximal alphanumeric runs of `s`, each lower-cased."""
    return [m.lower() for m in _WORD.findall(s)]


def query_terms(terms: Iterable[str]) -> List[str]:
    """Query terms are re-tokenized and flattened, keeping order and duplicates (bm25.rs:527-533)."""
    out: List[str] = []
    for raw in terms:
        out.extend(tokenize(raw))
    return out


# ---- hashed term keys (DESIGN A23): the device tokenises, hashes and counts ASCII documents ----

COUNTS, SEQUENCE = 0, 1          # UCFP_BM25_TERMS_COUNTS / _SEQUENCE
_FORMS = {"counts": COUNTS, "sequence": SEQUENCE}
NEEDS_HOST, E_UNSUPPORTED = 1, -2


def term_key(term: str) -> int:
    """The key of a (lower-cased) term: XXH3_64 of its UTF-8, seed 0 (ucfp_text_token_key).  Host only."""
    from . import _lib
    b = term.encode("utf-8")
    return int(_lib.load().ucfp_text_token_key(b, len(b)))


def host_pairs(text: str, form: int):
    """What the device entry gives for one document, from `tokenize` and `term_key` on the host: (keys, tfs)."""
    keys = [term_key(t) for t in tokenize(text)]
    if form == SEQUENCE:
        return keys, []
    counts = {}
    for k in keys:
        counts[k] = counts.get(k, 0) + 1
    ks = sorted(counts)
    return ks, [counts[k] for k in ks]


def terms_batch(texts, form: str = "counts", ctx=None, preprocess=None):
    """-> (keys u64, tfs u32, pair_offsets u64 [n + 1], status i32 [n]): document i's terms are
    (keys, tfs)[pair_offsets[i] .. pair_offsets[i + 1]) -- "counts": its distinct keys ascending, each with its count;
    "sequence": one key per token in text order, tfs empty.  The batch runs through ucfp_bm25_terms_batch; a document the
    device hands back (status 1: a byte >= 0x80; -2: a token too long for it) is tokenised on the host and spliced in,
    so the pairs are the same whatever the route.  `status` is the device's: its non-zero entries say which documents
    took the host route.  `preprocess` (TextOpts.preprocess: html | markdown | pdf) is not built into this entry and is
    refused: strip pages first with text.html_to_text_batch."""
    import ctypes as C

    import numpy as np

    from . import _lib
    from .errors import InvalidArgument, UnsupportedError
    if preprocess is not None:
        raise UnsupportedError(f"preprocess `{preprocess}` is not built into the BM25 ingest: strip the pages first "
                               "(text.html_to_text_batch)")
    if form not in _FORMS:
        raise InvalidArgument(f"unknown terms form {form!r}: 'counts' or 'sequence'")
    f = _FORMS[form]
    ctx = ctx or _lib.current_context()
    lib = _lib.load()
    blobs = [t.encode("utf-8") for t in texts]
    n = len(blobs)
    offs = np.zeros(n + 1, np.uint64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    blob = b"".join(blobs)
    cap = int(lib.ucfp_bm25_terms_max_pairs(len(blob), n))
    keys = np.zeros(max(cap, 1), np.uint64)
    tfs = np.zeros(max(cap, 1), np.uint32)
    po = np.zeros(n + 1, np.uint64)
    status = np.zeros(max(n, 1), np.int32)
    buf = (C.c_char * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
    _lib.check(lib.ucfp_bm25_terms_batch(ctx.handle, C.addressof(buf), offs.ctypes.data, n, f, keys.ctypes.data,
                                         tfs.ctypes.data if f == COUNTS else None, cap, po.ctypes.data, status.ctypes.data))
    status = status[:n]
    total = int(po[n])
    keys, tfs = keys[:total], (tfs[:total] if f == COUNTS else np.zeros(0, np.uint32))
    host = np.flatnonzero((status == NEEDS_HOST) | (status == E_UNSUPPORTED))
    if host.size == 0:
        return keys, tfs, po, status
    # splice the host's documents in: the device left them empty ranges
    kparts, tparts, counts, at = [], [], np.diff(po).astype(np.int64), 0
    for i in host:
        i = int(i)
        hk, ht = host_pairs(texts[i], f)
        p = int(po[i])
        kparts += [keys[at:p], np.array(hk, np.uint64)]
        tparts += [tfs[at:p] if f == COUNTS else tfs, np.array(ht, np.uint32)]
        counts[i] = len(hk)
        at = p
    kparts.append(keys[at:])
    tparts.append(tfs[at:] if f == COUNTS else tfs)
    po2 = np.zeros(n + 1, np.uint64)
    np.cumsum(counts, out=po2[1:])
    return np.concatenate(kparts), np.concatenate(tparts), po2, status
