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
