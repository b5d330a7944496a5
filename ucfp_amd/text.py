"""Text fingerprinting -- host-side mirror of src/modality/text.rs.

    fingerprint_minhash(text, tenant_id, record_id)                 text.rs:172-174
    fingerprint_minhash_with(text, opts, tenant_id, record_id)      text.rs:182-236  (any opts.h)
    fingerprint_simhash_tf / fingerprint_simhash_idf                text.rs:328-362
    fingerprint_lsh                                                 text.rs:437-446
    fingerprint_tlsh                                                text.rs:452-484  (TLSH 128/1, DESIGN A15)

    StreamingMinHashSession(opts, tenant_id, record_id)             text.rs:645-730  (DESIGN T7)
    StreamingSimHashSession(opts, tenant_id, record_id, idf=)       text.rs:328-421 as a session (DESIGN T11)
    ingest_stream_ndjson(body, opts, tenant_id, record_id)          handlers.rs:590-626

plus the batched form (`minhash_batch` / `simhash_batch` / `tlsh_batch`) and the stream sets (`MinHashStreams`,
`SimHashStreams`).  Hashing runs in the HIP library.
ASCII documents go to the GPU raw (it lower-cases and segments them).  A document with non-ASCII characters goes
to the GPU as UTF-8 (mode RAW_UTF8: the default canonicaliser -- NFKC + case fold + Bidi/Cf stripping,
text.rs:112-114 -- and the UAX#29 word tokeniser as tables).  Only what the device hands back
(combining marks, Hangul jamo, regional indicators, malformed text) or what it does not build (another
canonicaliser) is canonicalised and segmented here on the host (`_prepare`, via the `regex` module) and submitted
pre-tokenised; both routes give the same record.  Streams follow the same routing chunk by chunk: a
`MinHashStreams(utf8=True)` set canonicalises and tokenises RAW_UTF8 chunks on the device, cut anywhere.

`TextOpts(tokenizer="grapheme")` routes the same way through the entries that take a tokeniser: every
UAX#29 extended grapheme cluster of the canonical text is a token, found on the device for ASCII and for the grapheme
set of UTF-8; what the device hands back and every other canonicaliser is cut into clusters here (`regex`, \\X) and
hashed through the token entries, which `minhash_tokens` / `simhash_tokens` also open to any tokeniser the caller runs
itself (the reference's cjk-jp / cjk-ko).  Streams and the micro-batcher are built for the `word` tokeniser only.

`IdfTable` is the table `fingerprint_simhash_idf` takes: token key -> Q16.16 weight in device memory,
supplied (`from_weights`, `load`) or fitted to a corpus on the GPU (`fit`), applied by `simhash_batch(.., idf=)` and
`simhash_tokens(.., idf=)` through the same routes, and by `SimHashStreams(.., idf=)` chunk by chunk.
The micro-batcher takes no table.

`TextOpts(preprocess="html")` (text.rs:85-96, 751-767 behind handlers.rs:628-699) makes the texts of the
batch entries and the `fingerprint_*` builders HTML pages: `html_to_text_batch` strips them on the device
(ucfp_text_html_batch) and the routing above runs on the stripped text, which is also what a record's `text` holds.
`markdown` and `pdf` are not built and are refused; streams, the micro-batcher and the IDF fit take no `preprocess` yet.
"""
import ctypes as C
import math
import threading
import unicodedata
from dataclasses import dataclass, field, replace
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._streams import StreamSet, slot_arrays
from .core import Modality, Record
from .errors import InvalidArgument, ModalityError, UnsupportedError

DEFAULT_K = 5        # text.rs:39
DEFAULT_H = 128      # text.rs:41
ALGORITHM_MINHASH_128 = "minhash-h128"
ALGORITHM_SIMHASH_TF = "simhash-b64-tf"
ALGORITHM_SIMHASH_IDF = "simhash-b64-idf"
ALGORITHM_LSH = "minhash-lsh-h128"
ALGORITHM_TLSH = "tlsh-128-1"
FORMAT_VERSION = 1   # txtfp::FORMAT_VERSION as stored by text.rs:227
# MinHash / LSH records: the slot derivation (DESIGN T5) is KNOWN not to be txtfp 0.2.0's (the reference's
# golden slot 0, src/server/tests.rs:1153-1157, is not reproduced), so these records carry their own
# format_version: a corpus mixing them with upstream-produced `minhash-h128` records is then rejected as
# incompatible instead of yielding meaningless Jaccard estimates.  Layout, schema word and tag are upstream's.
FORMAT_VERSION_MINHASH_HIP = 0x48500001

RAW_ASCII, PRETOKENIZED, RAW_UTF8 = 0, 1, 2
TOK_WORD, TOK_GRAPHEME = 0, 1        # UCFP_TEXT_TOK_*: the tokeniser of the ucfp_text_*_batch_ex entries
NEEDS_HOST = 1
MINHASH_BYTES, SIMHASH_BYTES = 1032, 8
MINHASH_H_MIN, MINHASH_H_MAX, MINHASH_H_STEP = 16, 1024, 16   # UCFP_MINHASH_H_*: the slot counts built
TLSH_BYTES = 35             # UCFP_TLSH_BYTES: swap(checksum), swap(L), Q1 << 4 | Q2, code[31] .. code[0]
TLSH_MAX_DISTANCE = 2473    # UCFP_TLSH_MAX_DISTANCE
TLSH_MIN_BYTES = 50         # shorter documents are refused (the reference's README.md:96)
# UCFP_TEXT_MAX_WINDOW_BYTES (include/ucfp_hip.h, derived there): a document is always hashed when every window of k
# consecutive tokens (the whole document below k tokens, the single token for SimHash) has at most this many
# canonical bytes, separators included; longer windows may get status -2.
MAX_WINDOW_BYTES = 1405
STREAMS_UTF8 = 1                     # UCFP_TEXT_STREAMS_UTF8: the set also opens RAW_UTF8 streams
# UCFP_TEXT_STREAM_OPEN_SEGMENT_BYTES: canonical bytes of a segment without an alphanumeric a RAW_UTF8 stream can carry
# from one push to the next; more at a push boundary and the stream is handed back (NEEDS_HOST).
STREAM_OPEN_SEGMENT_BYTES = 256
# UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES (derived in include/ucfp_hip.h): a SimHash stream carries FEWER bytes than this,
# which keeps its token count below 2^31 on every route; a push that would reach it is refused.
SIMHASH_STREAM_LIMIT_BYTES = 1 << 30

# txtfp::config_hash is not available offline and could not be reconstructed (DESIGN section 2 lists what was
# tried).  The ONE value the reference's tests show (src/server/tests.rs:1158-1161: default canonicalizer,
# "shingle-k=5/word-uax29", "minhash-h128") is CARRIED here as a constant -- it is not computed, so it pins nothing.
_CARRIED_CONFIG_HASH = {("nfkc", True, True, True, "shingle-k=5/word-uax29", ALGORITHM_MINHASH_128):
                        2_212_816_233_060_047_056}


@dataclass
class Canonicalizer:
    """txtfp::Canonicalizer knobs as exposed by handlers.rs:547-586."""
    normalization: str = "nfkc"     # nfc | nfkc | none
    case_fold: bool = True
    strip_bidi: bool = True
    strip_format: bool = True

    def apply(self, s: str) -> str:
        if self.normalization == "nfkc":
            s = unicodedata.normalize("NFKC", s)
        elif self.normalization == "nfc":
            s = unicodedata.normalize("NFC", s)
        if self.case_fold:
            s = s.casefold()
            if self.normalization in ("nfkc", "nfc"):
                s = unicodedata.normalize(self.normalization.upper(), s)
        if self.strip_bidi or self.strip_format:
            s = "".join(ch for ch in s if unicodedata.category(ch) != "Cf")
        return s

    def is_default(self) -> bool:
        return self == Canonicalizer()


@dataclass
class TextOpts:
    """text.rs:116-147."""
    canonicalizer: Canonicalizer = field(default_factory=Canonicalizer)
    tokenizer: str = "word"          # word | grapheme | cjk-jp | cjk-ko (text.rs:71-82)
    k: int = DEFAULT_K
    h: int = DEFAULT_H
    preprocess: Optional[str] = None  # "html": stripped on the device; markdown | pdf: not built

    def tokenizer_tag(self) -> str:   # text.rs:152-159
        return {"word": f"shingle-k={self.k}/word-uax29", "grapheme": f"shingle-k={self.k}/grapheme-uax29",
                "cjk-jp": f"shingle-k={self.k}/cjk-jp", "cjk-ko": f"shingle-k={self.k}/cjk-ko"}[self.tokenizer]


def config_hash(canon: Canonicalizer, tokenizer_tag: str, algorithm: str) -> int:
    """txtfp::config_hash (text.rs:221): only the default MinHash configuration's value is known (carried as a
    constant from the reference's test); for any other configuration the reference's value cannot be produced,
    so this raises instead of inventing one."""
    key = (canon.normalization, canon.case_fold, canon.strip_bidi, canon.strip_format, tokenizer_tag, algorithm)
    if key in _CARRIED_CONFIG_HASH:
        return _CARRIED_CONFIG_HASH[key]
    raise UnsupportedError(f"txtfp::config_hash of {key} is unknown: only the default MinHash configuration's value "
                           "is carried (src/server/tests.rs:1158-1161)")


def _host_tokens(s: str) -> List[str]:
    import regex  # UAX#29 default word boundaries
    return [t for t in regex.split(r"(?w)\b", s, flags=regex.V1) if any(ch.isalnum() for ch in t)]


def _host_graphemes(s: str) -> List[str]:
    import regex  # UAX#29 extended grapheme clusters
    return regex.findall(r"\X", s)


def _unsupported_tokenizer(opts: "TextOpts") -> UnsupportedError:
    if opts.tokenizer in ("cjk-jp", "cjk-ko"):
        return UnsupportedError(f"tokenizer `{opts.tokenizer}` is not built into the HIP path: there is no segmenter here.  Run it "
                                "on the host and pass its tokens to text.minhash_tokens / text.simhash_tokens "
                                "(ucfp_text_minhash_tokens_batch / ucfp_text_simhash_tokens_batch)")
    return UnsupportedError(f"tokenizer `{opts.tokenizer}` is not built into the HIP path")


def _prepare(text: str, opts: TextOpts) -> Tuple[bytes, int]:
    """-> (bytes for the GPU, mode); the `word` tokeniser's host route."""
    if opts.tokenizer != "word":
        raise _unsupported_tokenizer(opts)
    c = opts.canonicalizer
    if text.isascii() and c.case_fold:
        return text.encode("ascii"), RAW_ASCII
    toks = _host_tokens(c.apply(text))
    return " ".join(toks).encode("utf-8"), PRETOKENIZED


def minhash_bytes(h: int = DEFAULT_H) -> int:
    """The bytes of a MinHash record of `h` slots (UCFP_MINHASH_RECORD_BYTES): 8 + 8 h."""
    return 8 + 8 * _check_h(h)


def _check_h(h) -> int:
    """the manifest's range (algorithms_manifest.rs:280-328), a multiple of 16 in [16, 1024]."""
    if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or h < MINHASH_H_MIN or h > MINHASH_H_MAX or h % MINHASH_H_STEP:
        raise InvalidArgument(f"MinHash slot count h must be a multiple of {MINHASH_H_STEP} in [{MINHASH_H_MIN}, {MINHASH_H_MAX}] "
                              f"(got {h!r})")
    return int(h)


def minhash_slots(record) -> int:
    """The slot count of a MinHash record, told by its length (every H carries the tag `minhash-h128`, text.rs:221-228)."""
    n = len(record)
    if n < 8 or (n - 8) % 8:
        raise InvalidArgument(f"{n} bytes are not a MinHash record (8 + 8 h)")
    return _check_h((n - 8) // 8)


def _rec_bytes(kind: str, h: int) -> int:
    return SIMHASH_BYTES if kind == "simhash" else 8 + 8 * h


def _pack(docs: Sequence[bytes]):
    offs = np.zeros(len(docs) + 1, np.uint64)
    np.cumsum([len(d) for d in docs], out=offs[1:])
    blob = np.frombuffer(b"".join(docs) + b"\0" * 16, np.uint8)
    return blob, offs


def _run(kind: str, docs: Sequence[bytes], mode: int, k: int, ctx=None, h: int = DEFAULT_H):
    """MinHash with h != 128 slots goes through the entries that take a slot count."""
    ctx = ctx or _lib.current_context()
    lib = _lib.load()
    blob, offs = _pack(docs)
    n = len(docs)
    out = np.zeros((n, _rec_bytes(kind, h)), np.uint8)
    status = np.zeros(n, np.int32)
    if kind == "simhash":
        _lib.check(lib.ucfp_text_simhash_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode,
                                               out.ctypes.data, status.ctypes.data))
    elif h != DEFAULT_H:
        _lib.check(lib.ucfp_text_minhash_h_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, TOK_WORD, k, h,
                                                 out.ctypes.data, status.ctypes.data))
    else:
        _lib.check(lib.ucfp_text_minhash_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, k,
                                               out.ctypes.data, status.ctypes.data))
    return out, status


def _device_utf8(text: str, opts: TextOpts) -> bool:
    """The document goes to the GPU as UTF-8 (mode RAW_UTF8): not ASCII (mode RAW_ASCII is cheaper and keeps its own
    documented `_` rule, DESIGN U6), default canonicaliser, `word` tokeniser."""
    return opts.tokenizer == "word" and opts.canonicalizer.is_default() and not text.isascii()


def canon_batch(docs: Sequence[bytes], ctx=None) -> Tuple[List[bytes], np.ndarray]:
    """UTF-8 documents -> (their canonical tokens joined by single spaces, status int32 [n]) on the GPU
    (ucfp_text_canon_batch).  Status NEEDS_HOST and an empty string for a document the device does not cover: for
    every other document the bytes are the ones `_prepare` makes on the host."""
    n = len(docs)
    status = np.zeros(n, np.int32)
    if n == 0:
        return [], status
    ctx = ctx or _lib.current_context()
    lib = _lib.load()
    blob, offs = _pack(docs)
    cap = int(lib.ucfp_text_canon_bound(int(offs[n])))
    toks = np.zeros(max(cap, 1), np.uint8)
    toff = np.zeros(n + 1, np.uint64)
    _lib.check(lib.ucfp_text_canon_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, toks.ctypes.data, cap,
                                         toff.ctypes.data, status.ctypes.data))
    return [toks[int(toff[i]):int(toff[i + 1])].tobytes() for i in range(n)], status


def _run_ex(kind: str, docs: Sequence[bytes], mode: int, tokenizer: int, k: int, ctx=None, h: int = DEFAULT_H):
    """`_run` through the entries that take a tokeniser (ucfp_text_*_batch_ex; ucfp_text_minhash_h_batch for h != 128)."""
    ctx = ctx or _lib.current_context()
    lib = _lib.load()
    blob, offs = _pack(docs)
    n = len(docs)
    out = np.zeros((n, _rec_bytes(kind, h)), np.uint8)
    status = np.zeros(n, np.int32)
    if kind == "simhash":
        _lib.check(lib.ucfp_text_simhash_batch_ex(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, tokenizer,
                                                  out.ctypes.data, status.ctypes.data))
    elif h != DEFAULT_H:
        _lib.check(lib.ucfp_text_minhash_h_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, tokenizer, k, h,
                                                 out.ctypes.data, status.ctypes.data))
    else:
        _lib.check(lib.ucfp_text_minhash_batch_ex(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, tokenizer, k,
                                                  out.ctypes.data, status.ctypes.data))
    return out, status


def _pack_tokens(docs: Sequence[Sequence[bytes]]):
    """-> (blob uint8, tok_offsets uint64 [T + 1], doc_tokens uint64 [n + 1]) of the caller-segmented form."""
    toks = [bytes(t) for d in docs for t in d]
    tok_offs = np.zeros(len(toks) + 1, np.uint64)
    np.cumsum([len(t) for t in toks], out=tok_offs[1:])
    doc_toks = np.zeros(len(docs) + 1, np.uint64)
    np.cumsum([len(d) for d in docs], out=doc_toks[1:])
    blob = np.frombuffer(b"".join(toks) + b"\0" * 16, np.uint8)
    return blob, tok_offs, doc_toks


def _run_tokens(kind: str, docs: Sequence[Sequence[bytes]], k: int, ctx=None, h: int = DEFAULT_H):
    ctx = ctx or _lib.current_context()
    lib = _lib.load()
    blob, tok_offs, doc_toks = _pack_tokens(docs)
    n = len(docs)
    out = np.zeros((n, _rec_bytes(kind, h)), np.uint8)
    status = np.zeros(n, np.int32)
    if kind == "simhash":
        _lib.check(lib.ucfp_text_simhash_tokens_batch(ctx.handle, blob.ctypes.data, tok_offs.ctypes.data, doc_toks.ctypes.data, n,
                                                      out.ctypes.data, status.ctypes.data))
    elif h != DEFAULT_H:
        _lib.check(lib.ucfp_text_minhash_tokens_h_batch(ctx.handle, blob.ctypes.data, tok_offs.ctypes.data, doc_toks.ctypes.data, n,
                                                        k, h, out.ctypes.data, status.ctypes.data))
    else:
        _lib.check(lib.ucfp_text_minhash_tokens_batch(ctx.handle, blob.ctypes.data, tok_offs.ctypes.data, doc_toks.ctypes.data, n,
                                                      k, out.ctypes.data, status.ctypes.data))
    return out, status


def minhash_tokens(docs: Sequence[Sequence[bytes]], k: int = DEFAULT_K, ctx=None, h: int = DEFAULT_H):
    """MinHash of documents the caller has tokenised: `docs` is a sequence of token sequences, a
    token any `bytes`, spaces and NULs included, hashed as it is; an empty token is not a token.  The route for any
    tokeniser the caller runs itself (the reference's cjk-jp / cjk-ko).  `h` is the slot count.
    -> (records uint8 [n, 8 + 8 h], status int32 [n])."""
    return _run_tokens("minhash", docs, k, ctx, _check_h(h))


def simhash_tokens(docs: Sequence[Sequence[bytes]], ctx=None, idf: Optional["IdfTable"] = None):
    """SimHash-64 of caller-tokenised documents (see `minhash_tokens`).  -> (records uint8 [n, 8], status int32 [n]).
    With `idf` (a final `IdfTable`) every token weighs what the table says."""
    if idf is not None:
        return idf._simhash_tokens(docs, ctx)
    return _run_tokens("simhash", docs, 1, ctx)


def _batch_grapheme(kind: str, texts: Sequence[str], opts: TextOpts, ctx=None, is_ascii=None):
    """The `grapheme` tokeniser: ASCII documents go raw (RAW_ASCII, when the canonicaliser folds case),
    other documents as UTF-8 when the canonicaliser is the default one (RAW_UTF8); what the device hands back and every
    other canonicaliser is canonicalised and cut into clusters here (`Canonicalizer.apply`, then \\X) and goes to the
    token entries.  All three routes give the same record."""
    h = _check_h(opts.h) if kind == "minhash" else DEFAULT_H
    out = np.zeros((len(texts), _rec_bytes(kind, h)), np.uint8)
    status = np.zeros(len(texts), np.int32)
    c = opts.canonicalizer
    host = []
    groups = {RAW_ASCII: [], RAW_UTF8: []}
    for i, t in enumerate(texts):
        asc = is_ascii[i] if is_ascii is not None else t.isascii()
        if asc and c.case_fold:
            groups[RAW_ASCII].append(i)
        elif not asc and c.is_default():
            groups[RAW_UTF8].append(i)
        else:
            host.append(i)
    for mode, idx in groups.items():
        if not idx:
            continue
        o, s = _run_ex(kind, [texts[i].encode("utf-8", "surrogatepass") for i in idx], mode, TOK_GRAPHEME, opts.k, ctx, h)
        out[idx] = o
        status[idx] = s
        host += [i for i, st in zip(idx, s) if st == NEEDS_HOST]
    if host:
        host.sort()
        docs = [[g.encode("utf-8", "surrogatepass") for g in _host_graphemes(c.apply(texts[i]))] for i in host]
        o, s = _run_tokens(kind, docs, opts.k, ctx, h)
        out[host] = o
        status[host] = s
    return out, status


def _batch(kind: str, texts: Sequence[str], opts: TextOpts, ctx=None, is_ascii=None):
    """Split into the raw-ASCII, the raw-UTF-8 and the host-pretokenised group, one launch each; the documents the
    UTF-8 launch hands back join the host group.  `is_ascii` (per text, from the HTML strip's flags) picks the UTF-8 group
    under the default canonicaliser without `_device_utf8`'s look at each text; `_prepare` still looks at the rest."""
    if opts.tokenizer == "grapheme":
        return _batch_grapheme(kind, texts, opts, ctx, is_ascii)
    h = _check_h(opts.h) if kind == "minhash" else DEFAULT_H
    out = np.zeros((len(texts), _rec_bytes(kind, h)), np.uint8)
    status = np.zeros(len(texts), np.int32)
    if is_ascii is not None and opts.tokenizer == "word" and opts.canonicalizer.is_default():
        dev = [i for i, a in enumerate(is_ascii) if not a]
    else:
        dev = [i for i, t in enumerate(texts) if _device_utf8(t, opts)]
    if dev:
        o, s = _run(kind, [texts[i].encode("utf-8", "surrogatepass") for i in dev], RAW_UTF8, opts.k, ctx, h)
        out[dev] = o
        status[dev] = s
    done = {i for i, st in zip(dev, status[dev]) if st != NEEDS_HOST}
    prepared = [None if i in done else _prepare(t, opts) for i, t in enumerate(texts)]
    for mode in (RAW_ASCII, PRETOKENIZED):
        idx = [i for i, p in enumerate(prepared) if p is not None and p[1] == mode]
        if not idx:
            continue
        o, s = _run(kind, [prepared[i][0] for i in idx], mode, opts.k, ctx, h)
        out[idx] = o
        status[idx] = s
    return out, status


HTML_NON_ASCII, HTML_OPEN_MARKUP = 1, 2      # UCFP_TEXT_HTML_*: the flag bits of html_to_text_batch


def html_to_text_batch(docs: Sequence, ctx=None) -> Tuple[List[bytes], np.ndarray]:
    """HTML pages -> (their text, flags uint32 [n]) on the GPU (ucfp_text_html_batch; DESIGN.md T12, rules M1-M8): markup,
    comments and script / style bodies dropped, character references decoded, white space folded.  `docs` are `bytes` or
    `str` (encoded as UTF-8).  Every page has a text -- there is no status and no hand-back; flag bit 0
    (HTML_NON_ASCII): the text holds a byte >= 0x80; bit 1 (HTML_OPEN_MARKUP): the page ended inside markup."""
    docs = [d.encode("utf-8", "surrogatepass") if isinstance(d, str) else bytes(d) for d in docs]
    n = len(docs)
    flags = np.zeros(n, np.uint32)
    if n == 0:
        return [], flags
    ctx = ctx or _lib.current_context()
    lib = _lib.load()
    blob, offs = _pack(docs)
    cap = int(lib.ucfp_text_html_bound(int(offs[n])))
    text = np.zeros(max(cap, 1), np.uint8)
    toff = np.zeros(n + 1, np.uint64)
    _lib.check(lib.ucfp_text_html_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, text.ctypes.data, cap,
                                        toff.ctypes.data, flags.ctypes.data))
    return [text[int(toff[i]):int(toff[i + 1])].tobytes() for i in range(n)], flags


def _no_preprocess(opts: Optional[TextOpts], what: str) -> None:
    """The entries that take no `preprocess` yet refuse it: ignoring it would fingerprint the markup."""
    if opts is not None and opts.preprocess is not None:
        raise UnsupportedError(f"preprocess `{opts.preprocess}` is not built into {what}: strip the pages first "
                               "(text.html_to_text_batch), or use the batch entries, which take preprocess=\"html\"")


def _check_preprocess(opts: Optional[TextOpts]) -> None:
    """The batch entries build `preprocess="html"` alone: markdown, pdf and anything unknown are refused."""
    if opts is not None and opts.preprocess not in (None, "html"):
        raise UnsupportedError(f"preprocess `{opts.preprocess}` is not built into the HIP path (only `html` is)")


def _preprocessed(texts: Sequence[str], opts: TextOpts, ctx=None):
    """TextOpts.preprocess (text.rs:85-96, 751-767) in front of the batch entries.  -> (texts, opts, is_ascii): with
    preprocess="html" the pages stripped on the device and decoded, the options with `preprocess` cleared, and per text
    whether it is ASCII (flag bit 0 of the strip: the routing needs no look at the text); without, everything as it came
    and is_ascii None.  Any other value is refused: markdown and pdf are not built.  The pages are `str`; a `bytes` page
    is taken too when what the strip leaves of it is UTF-8, and refused with InvalidArgument otherwise (markup between the
    bytes of one character: `\xc3<p>\xa9`) -- `html_to_text_batch` and `tlsh_batch` take any bytes."""
    _check_preprocess(opts)
    if opts.preprocess is None:
        return texts, opts, None
    stripped, flags = html_to_text_batch(texts, ctx)
    try:
        decoded = [b.decode("utf-8", "surrogatepass") for b in stripped]
    except UnicodeDecodeError as e:
        raise InvalidArgument(f"the text of a page is not UTF-8 after the markup is stripped ({e}): pass `str` pages, or strip "
                              "with text.html_to_text_batch and decode as you see fit") from None
    return decoded, replace(opts, preprocess=None), [not f & HTML_NON_ASCII for f in flags.tolist()]


def minhash_batch(texts: Sequence[str], opts: Optional[TextOpts] = None, ctx=None):
    """-> (records uint8 [n, 8 + 8 opts.h], status int32 [n]); opts.h is the slot count (1032 bytes at the
    default 128).  With opts.preprocess = "html" the texts are pages, stripped on the device first."""
    texts, opts, is_ascii = _preprocessed(texts, opts or TextOpts(), ctx)
    return _batch("minhash", texts, opts, ctx, is_ascii)


def simhash_batch(texts: Sequence[str], opts: Optional[TextOpts] = None, ctx=None, idf: Optional["IdfTable"] = None):
    """-> (records uint8 [n, 8], status int32 [n]).  With `idf` (a final `IdfTable`) the TF.IDF record of DESIGN.md T9.
    With opts.preprocess = "html" the texts are pages, stripped on the device first."""
    texts, opts, is_ascii = _preprocessed(texts, opts or TextOpts(), ctx)
    if idf is not None:
        return idf._simhash(texts, opts, ctx, is_ascii)
    return _batch("simhash", texts, opts, ctx, is_ascii)


def _route(texts: Sequence[str], opts: TextOpts, run, run_tokens, rec_bytes: int, is_ascii=None):
    """The routing of `_batch` / `_batch_grapheme` around other runners (the IDF table's): ASCII documents raw, other
    documents as UTF-8 under the default canonicaliser, what the device hands back and every other canonicaliser through
    the host (PRETOKENIZED for `word`, the token form for `grapheme`).  run(docs, mode, tokenizer) and run_tokens(docs)
    return (records or None, status)."""
    if opts.tokenizer not in ("word", "grapheme"):
        raise _unsupported_tokenizer(opts)
    grapheme = opts.tokenizer == "grapheme"
    tok = TOK_GRAPHEME if grapheme else TOK_WORD
    out = np.zeros((len(texts), rec_bytes), np.uint8)
    status = np.zeros(len(texts), np.int32)
    c = opts.canonicalizer
    host = []
    groups = {RAW_ASCII: [], RAW_UTF8: []}
    for i, t in enumerate(texts):
        asc = is_ascii[i] if is_ascii is not None else t.isascii()
        if asc and c.case_fold:
            groups[RAW_ASCII].append(i)
        elif not asc and c.is_default():
            groups[RAW_UTF8].append(i)
        else:
            host.append(i)

    def put(idx, o, s):
        if o is not None:
            out[idx] = o
        status[idx] = s

    for mode, idx in groups.items():
        if idx:
            o, s = run([texts[i].encode("utf-8", "surrogatepass") for i in idx], mode, tok)
            put(idx, o, s)
            host += [i for i, st in zip(idx, s) if st == NEEDS_HOST]
    if host:
        host.sort()
        if grapheme:
            o, s = run_tokens([[g.encode("utf-8", "surrogatepass") for g in _host_graphemes(c.apply(texts[i]))] for i in host])
        else:
            o, s = run([" ".join(_host_tokens(c.apply(texts[i]))).encode("utf-8") for i in host], PRETOKENIZED, TOK_WORD)
        put(host, o, s)
    return out, status


def _quantize_weight(w) -> int:
    """a float weight -> Q16.16, floor(w * 65536 + 0.5) in float64."""
    w = float(w)
    if not (w >= 0.0) or w >= 65536.0:          # NaN fails the first comparison
        raise InvalidArgument(f"an IDF weight must be in [0, 65536) (got {w!r})")
    q = int(math.floor(w * 65536.0 + 0.5))
    if q > 0xFFFFFFFF:
        raise InvalidArgument(f"an IDF weight must quantise below 2^32 (got {w!r})")
    return q


class IdfTable:
    """A device-resident IDF table (ucfp_idf_table_*): token key -> Q16.16 weight, fitted to a corpus on
    the GPU (`add` / `add_tokens`, then `finalize`; `fit` does both) or supplied (`from_weights`, `load`).  A final table
    goes to `simhash_batch(.., idf=table)`, `simhash_tokens(.., idf=table)` and `fingerprint_simhash_idf`.  A token's key
    is XXH3-64 of its canonical bytes, so one table serves every tokeniser and route.  One thread mutates a table at a
    time; a final one may be read by any number."""

    def __init__(self, opts: Optional[TextOpts] = None, ctx=None, capacity_hint: int = 1 << 16, piece_tokens: int = 0):
        self.opts = opts or TextOpts()
        self.ctx = ctx or _lib.current_context()
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_idf_table_create(self.ctx.handle, int(capacity_hint), int(piece_tokens), 0, C.byref(h)))
        self.handle = h

    # ---- the corpus side
    def _add_docs(self, docs: Sequence[bytes], mode: int, tokenizer: int):
        blob, offs = _pack(docs)
        status = np.zeros(len(docs), np.int32)
        _lib.check(self._lib.ucfp_idf_table_add_batch(self.handle, blob.ctypes.data, offs.ctypes.data, len(docs), mode, tokenizer,
                                                      status.ctypes.data))
        return None, status

    def _add_tokens(self, docs: Sequence[Sequence[bytes]]):
        blob, tok_offs, doc_toks = _pack_tokens(docs)
        status = np.zeros(len(docs), np.int32)
        _lib.check(self._lib.ucfp_idf_table_add_tokens_batch(self.handle, blob.ctypes.data, tok_offs.ctypes.data,
                                                             doc_toks.ctypes.data, len(docs), status.ctypes.data))
        return None, status

    def add(self, texts: Sequence[str]) -> np.ndarray:
        """Count the documents' tokens (routed as `simhash_batch` routes them: raw ASCII, UTF-8 on the device, the host's
        tokens for what the device hands back; `cjk-*` has no segmenter here -- pass its tokens to `add_tokens`).
        -> status int32 [n]; a document whose final status is not 0 adds nothing.  The table is not final afterwards."""
        _no_preprocess(self.opts, "the IDF table's fit")
        return _route(texts, self.opts, self._add_docs, self._add_tokens, 0)[1]

    def add_tokens(self, docs: Sequence[Sequence[bytes]]) -> np.ndarray:
        return self._add_tokens(docs)[1]

    def finalize(self) -> "IdfTable":
        """Weights from the counts (T9.4); the call waits for them, so a SimHash call on any stream sees them.  The fit
        scratch is given back."""
        _lib.check(self._lib.ucfp_idf_table_finalize(self.handle, None))
        return self

    def fit(self, texts: Sequence[str]) -> "IdfTable":
        self.add(texts)
        return self.finalize()

    # ---- supplied weights
    def key(self, token) -> int:
        """T9.1: a `str` is canonicalised with opts.canonicalizer first, `bytes` are keyed as they are, an `int` is a key."""
        if isinstance(token, (int, np.integer)):
            k = int(token)
            if not 0 <= k < 1 << 64:
                raise InvalidArgument(f"a raw key is a u64 (got {k})")
            return k
        if isinstance(token, str):
            token = self.opts.canonicalizer.apply(token).encode("utf-8", "surrogatepass")
        b = bytes(token)
        return int(self._lib.ucfp_text_token_key(b, len(b)))

    def set_weights(self, mapping_or_pairs, default: float = 1.0) -> "IdfTable":
        pairs = list(mapping_or_pairs.items()) if hasattr(mapping_or_pairs, "items") else list(mapping_or_pairs)
        keys = np.array([self.key(k) for k, _ in pairs], np.uint64)
        wts = np.array([_quantize_weight(w) for _, w in pairs], np.uint32)
        return self._set_q16(keys, wts, _quantize_weight(default))

    def _set_q16(self, keys: np.ndarray, wts: np.ndarray, default_q16: int) -> "IdfTable":
        keys = np.ascontiguousarray(keys, np.uint64)
        wts = np.ascontiguousarray(wts, np.uint32)
        _lib.check(self._lib.ucfp_idf_table_set_weights(self.handle, keys.ctypes.data if keys.size else None,
                                                        wts.ctypes.data if wts.size else None, keys.size, int(default_q16)))
        return self

    @classmethod
    def from_weights(cls, mapping_or_pairs, default: float = 1.0, opts: Optional[TextOpts] = None, ctx=None) -> "IdfTable":
        pairs = mapping_or_pairs.items() if hasattr(mapping_or_pairs, "items") else mapping_or_pairs
        pairs = list(pairs)
        t = cls(opts, ctx, capacity_hint=max(16, len(pairs)))
        try:
            return t.set_weights(pairs, default)
        except Exception:
            t.close()
            raise

    # ---- reading
    def _size(self):
        nd, nk, fin = C.c_uint64(0), C.c_size_t(0), C.c_int(0)
        _lib.check(self._lib.ucfp_idf_table_size(self.handle, C.byref(nd), C.byref(nk), C.byref(fin)))
        return int(nd.value), int(nk.value), bool(fin.value)

    @property
    def n_docs(self) -> int:
        return self._size()[0]

    @property
    def is_final(self) -> bool:
        return self._size()[2]

    def __len__(self) -> int:
        return self._size()[1]

    def __bool__(self) -> bool:
        nd, nk, _ = self._size()
        return nk > 0 or nd > 0

    def export(self) -> dict:
        """-> {"keys" u64, "dfs" u32, "weights" u32 (Q16.16), "default" int, "n_docs" int}, sorted by key: what a host
        persists.  `IdfTable.load` makes a supplied table of it (weights and default; counts are not restored)."""
        nd, nk, _ = self._size()
        keys, dfs, wts = np.zeros(nk, np.uint64), np.zeros(nk, np.uint32), np.zeros(nk, np.uint32)
        n, dq = C.c_size_t(0), C.c_uint32(0)
        _lib.check(self._lib.ucfp_idf_table_export(self.handle, keys.ctypes.data if nk else None, dfs.ctypes.data if nk else None,
                                                   wts.ctypes.data if nk else None, nk, C.byref(n), C.byref(dq)))
        order = np.argsort(keys[:n.value], kind="stable")
        return {"keys": keys[order], "dfs": dfs[order], "weights": wts[order], "default": int(dq.value), "n_docs": nd}

    @classmethod
    def load(cls, arrays: dict, opts: Optional[TextOpts] = None, ctx=None) -> "IdfTable":
        t = cls(opts, ctx, capacity_hint=max(16, len(arrays["keys"])))
        try:
            return t._set_q16(np.asarray(arrays["keys"]), np.asarray(arrays["weights"]), int(arrays["default"]))
        except Exception:
            t.close()
            raise

    def weight(self, token) -> float:
        """The weight a token has in the final table (the default when its key is absent)."""
        e = self.export()
        k = np.uint64(self.key(token))
        i = int(np.searchsorted(e["keys"], k))
        q = int(e["weights"][i]) if i < e["keys"].size and e["keys"][i] == k else e["default"]
        return q / 65536.0

    @property
    def digest(self) -> int:
        """XXH3-64 over the key-sorted (key, weight) pairs and the default, little-endian: names the table that made a record."""
        e = self.export()
        body = b"".join(int(k).to_bytes(8, "little") + int(w).to_bytes(4, "little") for k, w in zip(e["keys"], e["weights"]))
        body += int(e["default"]).to_bytes(4, "little")
        return int(self._lib.ucfp_text_token_key(body, len(body)))

    # ---- the record side
    def _simhash_docs(self, ctx, docs: Sequence[bytes], mode: int, tokenizer: int):
        blob, offs = _pack(docs)
        out = np.zeros((len(docs), SIMHASH_BYTES), np.uint8)
        status = np.zeros(len(docs), np.int32)
        _lib.check(self._lib.ucfp_text_simhash_idf_batch(ctx.handle, self.handle, blob.ctypes.data, offs.ctypes.data, len(docs), mode,
                                                         tokenizer, out.ctypes.data, status.ctypes.data))
        return out, status

    def _simhash_tokens(self, docs: Sequence[Sequence[bytes]], ctx=None):
        ctx = ctx or self.ctx
        blob, tok_offs, doc_toks = _pack_tokens(docs)
        out = np.zeros((len(docs), SIMHASH_BYTES), np.uint8)
        status = np.zeros(len(docs), np.int32)
        _lib.check(self._lib.ucfp_text_simhash_idf_tokens_batch(ctx.handle, self.handle, blob.ctypes.data, tok_offs.ctypes.data,
                                                                doc_toks.ctypes.data, len(docs), out.ctypes.data, status.ctypes.data))
        return out, status

    def _simhash(self, texts: Sequence[str], opts: TextOpts, ctx=None, is_ascii=None):
        ctx = ctx or self.ctx
        return _route(texts, opts, lambda d, m, t: self._simhash_docs(ctx, d, m, t), lambda d: self._simhash_tokens(d, ctx),
                      SIMHASH_BYTES, is_ascii)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_idf_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TextStreams(StreamSet):
    """What the text stream sets share (ucfp_text_streams_*): `open`, and a push whose final entries emit one record of
    `record_bytes` bytes each (ucfp_text_streams_record_bytes)."""
    _abi = "ucfp_text_streams"
    record_bytes = MINHASH_BYTES

    def _created(self, max_streams: int, utf8: bool, max_push_bytes: int) -> None:
        self.max_streams = max_streams
        self.utf8, self.max_push_bytes = bool(utf8), int(max_push_bytes) if utf8 else 0
        self.record_bytes = int(self._lib.ucfp_text_streams_record_bytes(self.handle))

    def open(self, mode: int = RAW_ASCII) -> int:
        return super().open(mode)

    def push_dev(self, slots, counts, d_bytes, d_out, d_status, final=(), stream: int = 0) -> None:
        """Device variant (no sync): `d_bytes` the chunks of `slots` concatenated (uint8 tensor, any alignment), `d_out` a
        uint8 [len(slots), record_bytes] tensor -- 1032 for MinHash, 8 for SimHash -- (row i is written only when slots[i]
        is in `final`; None when nothing is final), `d_status` an int32 [len(slots)] tensor."""
        sl, ns, fi = slot_arrays(slots, counts, final)
        _lib.check(self._lib.ucfp_text_streams_push_dev(
            self.handle, sl.ctypes.data, ns.ctypes.data, fi.ctypes.data, sl.size,
            d_bytes.data_ptr() if d_bytes is not None and d_bytes.numel() else None,
            d_out.data_ptr() if d_out is not None else None, d_status.data_ptr() if d_status is not None else None,
            stream or None))

    def push(self, chunks: dict, final=()) -> dict:
        """{slot: bytes} -> {slot: (record bytes or None, status)}; slots in `final` end (and free their slot) and
        return their record (1032 bytes for MinHash, 8 for SimHash)."""
        import torch
        final = set(final)
        slots = list(chunks)
        if not slots:
            return {}
        blobs = [bytes(chunks[s]) for s in slots]
        dev = f"cuda:{self.ctx.device}"
        blob = b"".join(blobs)
        d_bytes = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev) if blob else None
        d_out = torch.zeros((len(slots), self.record_bytes), dtype=torch.uint8, device=dev) if final else None
        d_st = torch.zeros(len(slots), dtype=torch.int32, device=dev)
        self.push_dev(slots, [len(b) for b in blobs], d_bytes, d_out, d_st, final,
                      torch.cuda.current_stream().cuda_stream)
        st = d_st.cpu().numpy()
        out = d_out.cpu().numpy() if final else None
        return {s: (out[i].tobytes() if s in final else None, int(st[i])) for i, s in enumerate(slots)}


class MinHashStreams(_TextStreams):
    """A set of live MinHash streams on the device (ucfp_text_streams_*): `push` advances any subset of
    them by one chunk each with one launch.  A stream's final record and status are those of `ucfp_text_minhash_batch`
    on the concatenation of its chunks, however they were cut.  Modes: RAW_ASCII and PRETOKENIZED; with `utf8=True`
    also RAW_UTF8 (the device canonicalises and tokenises, cuts inside a UTF-8 sequence included), and the RAW_UTF8
    chunks of one push may then have `max_push_bytes` bytes in all (the set's scratch is sized for them once)."""

    def __init__(self, max_streams: int, k: int = DEFAULT_K, ctx=None, utf8: bool = False, max_push_bytes: int = 1 << 20):
        self._create(ctx, "create_ex", k, max_streams, STREAMS_UTF8 if utf8 else 0, max_push_bytes if utf8 else 0)
        self.k = k
        self._created(max_streams, utf8, max_push_bytes)


class SimHashStreams(_TextStreams):
    """A set of live SimHash streams on the device (ucfp_text_streams_create_sim): the `open`, `push_dev`
    and `push` of `MinHashStreams`, with 8-byte records.  A stream's final record and status are those of
    `ucfp_text_simhash_batch` -- with `idf`, a final `IdfTable`, of `ucfp_text_simhash_idf_batch` -- on the concatenation
    of its chunks, however they were cut.  A falsy `idf` gives TF records.  The set reads the table at every push and
    keeps a reference to it; a push while the table is not final is refused.  A stream carries fewer than
    SIMHASH_STREAM_LIMIT_BYTES bytes."""

    def __init__(self, max_streams: int, ctx=None, utf8: bool = False, max_push_bytes: int = 1 << 20, idf=None):
        if idf and not isinstance(idf, IdfTable):
            raise UnsupportedError("only a ucfp_amd.text.IdfTable is built into the HIP path")
        self.idf = idf if idf else None           # held: the device reads the table until the set is destroyed
        self._create(ctx, "create_sim", max_streams, STREAMS_UTF8 if utf8 else 0, max_push_bytes if utf8 else 0,
                     self.idf.handle if self.idf is not None else None)
        self._created(max_streams, utf8, max_push_bytes)


_CUT_AT = " \n\t\r"
_SESSION_PUSH_BYTES = 256 << 10      # RAW_UTF8 bytes a session gives the device at once (its set holds 4 x this of scratch)


def _stream_cut(s: str) -> Tuple[str, str]:
    """-> (head, tail): `s` cut just before its last ASCII whitespace character (head is empty when there is none).
    A streaming session canonicalises and tokenises `head` now and keeps `tail`.  The cut is safe because an ASCII
    whitespace character is a starter that never composes with what precedes it (normalisation of A + B is
    normalisation of A + normalisation of B when B begins with one), case folding and Cf stripping work per character,
    and UAX#29 always breaks before it after a non-space: tokens(A + B) = tokens(A) ++ tokens(B)."""
    at = max(s.rfind(ch) for ch in _CUT_AT)
    return (s[:at], s[at:]) if at > 0 else ("", s)


class _StreamingSession:
    """The routing that `StreamingMinHashSession` and `StreamingSimHashSession` share, on a one-slot stream set that
    `_make_set(utf8)` creates; `_record(fingerprint)` makes the record `finalize` returns.  Routing follows `_prepare`:
      - while every byte so far is ASCII and the canonicaliser folds case, chunks go raw to a RAW_ASCII stream; the
        session keeps these ASCII bytes on the host (no more than the reference buffers), because
      - at the first byte >= 0x80 the document is one the DEVICE canonicalises when the canonicaliser is the default
        one (the condition of `_device_utf8`): the session drops that stream, opens a RAW_UTF8 one, replays the kept
        bytes into it and goes on pushing raw chunks, cut wherever they are cut -- text without ASCII whitespace
        advances like any other.  It keeps the bytes, as the ASCII route does, because
      - if a push reports NEEDS_HOST (a combining mark, malformed UTF-8 ...) the session falls back,
        once, to the host route and replays them there; with another canonicaliser (or without case folding, from the
        start) the host route is taken directly.  `route` names the one in use: "ascii", "utf8" or "host";
      - host route: a PRETOKENIZED stream; UTF-8 is decoded incrementally, the text seen so far is cut just before its last ASCII whitespace
        character (`_stream_cut`), the head is canonicalised and tokenised and pushed, the tail stays on the host.
        Text without ASCII whitespace is therefore held whole until `finalize` -- on this route only."""

    def __init__(self, opts: Optional[TextOpts], tenant_id: int, record_id: int, config_hash_value: Optional[int] = None):
        import codecs
        self.opts = opts or TextOpts()
        if self.opts.tokenizer != "word":
            raise UnsupportedError(f"tokenizer `{self.opts.tokenizer}` is not built into the HIP path")
        _no_preprocess(self.opts, "the text streams")
        self._check_opts()
        self.tenant_id, self.record_id = tenant_id, record_id
        self._config_hash_value = config_hash_value
        self._utf8_ok = self.opts.canonicalizer.is_default()
        self._set = self._make_set(self._utf8_ok)
        self._dec = codecs.getincrementaldecoder("utf-8")("strict")
        self._tail = ""
        self._bad = None                  # the first UTF-8 error: reported by finalize
        self._done = False
        self.route = "ascii" if self.opts.canonicalizer.case_fold else "host"
        self._kept = bytearray()          # ASCII and UTF-8 routes: the bytes so far, for the replay
        self._slot = self._set.open(RAW_ASCII if self.route == "ascii" else PRETOKENIZED)

    def _check_opts(self) -> None:
        pass

    def _make_set(self, utf8: bool) -> "_TextStreams":
        raise NotImplementedError

    def _record(self, fingerprint: bytes) -> Record:
        raise NotImplementedError

    def _dev_push(self, data: bytes, final: bool):
        out = (C.c_uint8 * self._set.record_bytes)()
        st = C.c_int32(0)
        _lib.check(self._set._lib.ucfp_text_streams_push(self._set.handle, self._slot, data if data else None, len(data),
                                                         1 if final else 0, out if final else None, C.byref(st)))
        return bytes(out), int(st.value)

    def _utf8_push(self, data: bytes, final: bool):
        """A RAW_UTF8 push in pieces the set's scratch was sized for; stops at the first piece the device hands back."""
        at = 0
        while True:
            piece = data[at:at + _SESSION_PUSH_BYTES]
            at += len(piece)
            last = at >= len(data)
            rec, status = self._dev_push(piece, final and last)
            if last or status == NEEDS_HOST:
                return rec, status, final and last

    def _host_push(self, data: bytes, final: bool):
        if self._bad is None:
            try:
                self._tail += self._dec.decode(data, final)
            except UnicodeDecodeError as e:
                self._bad = e
        if self._bad is not None:
            if final:
                self._set.close(self._slot)
                raise ModalityError(f"streamed text is not valid UTF-8: {self._bad}")
            return None
        head, tail = (self._tail, "") if final else _stream_cut(self._tail)
        self._tail = tail
        toks = _host_tokens(self.opts.canonicalizer.apply(head)) if head else []
        if final:
            return self._dev_push(" ".join(toks).encode("utf-8"), True)
        if toks:
            self._dev_push((" ".join(toks) + " ").encode("utf-8"), False)
        return None

    def _feed(self, chunk: bytes, final: bool):
        if self._done:
            raise ModalityError("streaming session already finalized")
        chunk = bytes(chunk)
        if self.route == "ascii":
            if chunk.isascii():
                self._kept += chunk
                return self._dev_push(chunk, final)
            self.route = "utf8" if self._utf8_ok else "host"
            self._set.close(self._slot)
            self._slot = self._set.open(RAW_UTF8 if self._utf8_ok else PRETOKENIZED)
            chunk = bytes(self._kept) + chunk
            self._kept = bytearray()
        if self.route == "utf8":
            self._kept += chunk
            rec, status, ended = self._utf8_push(chunk, final)
            if status != NEEDS_HOST:
                return rec, status
            self.route = "host"               # what the device does not cover: once, with everything seen so far
            if not ended:
                self._set.close(self._slot)
            self._slot = self._set.open(PRETOKENIZED)
            chunk = bytes(self._kept)
            self._kept = bytearray()
        return self._host_push(chunk, final)

    def push(self, chunk: bytes) -> List[Record]:
        self._feed(chunk, False)
        return []

    def finalize(self) -> List[Record]:
        try:
            rec, status = self._feed(b"", True)
        finally:
            if not self._done:
                self._done = True
                self._kept = bytearray()
                self._set.destroy()
        _raise_for(status)
        return [self._record(rec)]


class StreamingMinHashSession(_StreamingSession):
    """Push/finalize wrapper (text.rs:655-730) on a one-slot MinHashStreams.  The reference's session buffers the whole
    document; here every chunk advances the stream on the device.  `push` returns no records (as the reference's);
    `finalize` returns the one record, equal to `minhash_batch([whole text], opts)` however the text was cut into
    chunks, cuts inside a UTF-8 sequence included.  The routing ("ascii", "utf8", "host") is `_StreamingSession`'s."""

    def _check_opts(self) -> None:
        if self.opts.h != DEFAULT_H:
            raise UnsupportedError(f"streaming MinHash is built for H = {DEFAULT_H} only, as the reference's session is (got "
                                   f"H = {self.opts.h}); minhash_batch takes any H")

    def _make_set(self, utf8: bool) -> MinHashStreams:
        return MinHashStreams(1, self.opts.k, utf8=utf8, max_push_bytes=_SESSION_PUSH_BYTES)

    def _record(self, fingerprint: bytes) -> Record:
        o = self.opts
        return Record(tenant_id=self.tenant_id, record_id=self.record_id, modality=Modality.Text,
                      format_version=FORMAT_VERSION_MINHASH_HIP, algorithm=ALGORITHM_MINHASH_128,
                      config_hash=_record_config_hash(o, o.tokenizer_tag(), ALGORITHM_MINHASH_128, self._config_hash_value),
                      fingerprint=fingerprint, embedding=None, model_id=None, metadata=b"", text=None)


class StreamingSimHashSession(_StreamingSession):
    """The session of `StreamingMinHashSession` on a one-slot SimHashStreams: `finalize` returns the one
    record that `fingerprint_simhash_tf(whole text, opts, ..)` builds -- with `idf`, a final `IdfTable`, and
    `algorithm=ALGORITHM_SIMHASH_IDF`, the one `fingerprint_simhash_idf(whole text, opts, idf, ..)` builds -- however the
    text was cut into chunks (`text` is None, as in the MinHash session).  A falsy `idf` weighs every token 1.0 under
    either tag, as `fingerprint_simhash_idf` does.  The reference has no SimHash session; the routing is the shared one."""

    def __init__(self, opts: Optional[TextOpts], tenant_id: int, record_id: int, idf=None,
                 algorithm: str = ALGORITHM_SIMHASH_TF, config_hash_value: Optional[int] = None):
        if algorithm not in (ALGORITHM_SIMHASH_TF, ALGORITHM_SIMHASH_IDF):
            raise UnsupportedError(f"a SimHash session makes `{ALGORITHM_SIMHASH_TF}` or `{ALGORITHM_SIMHASH_IDF}` records "
                                   f"(got `{algorithm}`)")
        if idf and not isinstance(idf, IdfTable):
            raise UnsupportedError("only a ucfp_amd.text.IdfTable is built into the HIP path")
        if idf and algorithm != ALGORITHM_SIMHASH_IDF:
            raise InvalidArgument(f"a table makes `{ALGORITHM_SIMHASH_IDF}` records: pass algorithm=ALGORITHM_SIMHASH_IDF")
        self.algorithm = algorithm
        self._idf = idf if idf else None
        super().__init__(opts, tenant_id, record_id, config_hash_value)

    def _make_set(self, utf8: bool) -> SimHashStreams:
        return SimHashStreams(1, utf8=utf8, max_push_bytes=_SESSION_PUSH_BYTES, idf=self._idf)

    def _record(self, fingerprint: bytes) -> Record:
        return Record(tenant_id=self.tenant_id, record_id=self.record_id, modality=Modality.Text,
                      format_version=FORMAT_VERSION, algorithm=self.algorithm,
                      config_hash=_record_config_hash(self.opts, "word-uax29", self.algorithm, self._config_hash_value),
                      fingerprint=fingerprint, embedding=None, model_id=None, metadata=b"", text=None)


def _ndjson_chunks(body: bytes) -> List[bytes]:
    """The lines of an NDJSON stream body (handlers.rs:603-612): split on LF, one trailing CR stripped, empty lines
    skipped, every other line a JSON string."""
    import json
    chunks = []
    for line in bytes(body).split(b"\n"):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        try:
            v = json.loads(line)
        except (ValueError, UnicodeDecodeError) as e:
            raise ModalityError(f"NDJSON line: {e}") from None
        if not isinstance(v, str):
            raise ModalityError(f"NDJSON line: invalid type: {type(v).__name__}, expected a string")
        chunks.append(v.encode("utf-8", "surrogatepass"))
    return chunks


def ingest_stream_ndjson(body: bytes, opts: Optional[TextOpts], tenant_id: int, record_id: int,
                         algorithm: Optional[str] = None, idf=None) -> Record:
    """The body loop of POST /v1/ingest/text/{tid}/{rid}/stream (handlers.rs:603-617): every line is a JSON string
    carrying a chunk; push each, finalise, return the record.  The body is parsed before any device work.
    `algorithm` is this library's own (the reference's route only knows MinHash): None gives the MinHash record,
    "simhash-tf" / "simhash-idf" the record of a `StreamingSimHashSession`, the latter weighted by `idf`."""
    if algorithm not in (None, "simhash-tf", "simhash-idf"):
        raise UnsupportedError(f"stream ingest makes MinHash (None), `simhash-tf` or `simhash-idf` records (got `{algorithm}`)")
    chunks = _ndjson_chunks(body)
    if not chunks:
        raise ModalityError("streaming session produced no record")
    if algorithm is None:
        session = StreamingMinHashSession(opts, tenant_id, record_id)
    else:
        session = StreamingSimHashSession(opts, tenant_id, record_id, idf=idf if algorithm == "simhash-idf" else None,
                                          algorithm=ALGORITHM_SIMHASH_TF if algorithm == "simhash-tf" else ALGORITHM_SIMHASH_IDF)
    try:
        for c in chunks:
            session.push(c)
    except Exception:
        session._set.destroy()
        raise
    records = session.finalize()
    if not records:
        raise ModalityError("streaming session produced no record")
    return records[-1]


ALGO_MINHASH, ALGO_SIMHASH = 1, 2


class TextBatcher:
    """Host micro-batcher (handlers.rs:304-460 fingerprints one document per request): many request
    threads call `submit` concurrently, the library packs them into one GPU launch.  Three C batchers sit behind this
    object -- one for raw ASCII documents, one for raw UTF-8 documents, one for the documents the host had to
    canonicalise and tokenise (the ones the UTF-8 batcher handed back among them)."""

    def __init__(self, kind: str = "minhash", opts: Optional[TextOpts] = None, *, max_batch: int = 4096,
                 max_bytes: int = 8 << 20, max_delay_us: int = 200, ctx=None):
        if kind not in ("minhash", "simhash"):
            raise UnsupportedError(f"text batcher kind `{kind}`")
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.opts = opts or TextOpts()
        _no_preprocess(self.opts, "the text micro-batcher")
        if kind == "minhash" and self.opts.h != DEFAULT_H:
            raise UnsupportedError(f"the text micro-batcher is built for H = {DEFAULT_H} only (got H = {self.opts.h}); "
                                   "minhash_batch takes any H")
        self.kind = kind
        self.rec = MINHASH_BYTES if kind == "minhash" else SIMHASH_BYTES
        algo = ALGO_MINHASH if kind == "minhash" else ALGO_SIMHASH
        self._handles = {}
        self._handed_back = 0
        self._mu = threading.Lock()
        for mode in (RAW_ASCII, PRETOKENIZED, RAW_UTF8):
            h = C.c_void_p()
            _lib.check(self._lib.ucfp_text_batcher_create(self.ctx.handle, algo, mode, self.opts.k, max_batch, max_bytes,
                                                          max_delay_us, C.byref(h)))
            self._handles[mode] = h

    def submit(self, text: str):
        """-> (record bytes, status).  Blocks until this document's record is ready."""
        out = (C.c_uint8 * self.rec)()
        st = C.c_int32(0)
        if _device_utf8(text, self.opts):
            doc = text.encode("utf-8", "surrogatepass")
            _lib.check(self._lib.ucfp_text_batcher_submit(self._handles[RAW_UTF8], doc, len(doc), out, C.byref(st)))
            if int(st.value) != NEEDS_HOST:
                return bytes(out), int(st.value)
            with self._mu:
                self._handed_back += 1
        doc, mode = _prepare(text, self.opts)
        _lib.check(self._lib.ucfp_text_batcher_submit(self._handles[mode], doc, len(doc), out, C.byref(st)))
        return bytes(out), int(st.value)

    def stats(self):
        """-> (launches, documents) summed over the modes; a document handed back by the device counts once."""
        tb = ti = 0
        for h in self._handles.values():
            b, i = C.c_uint64(0), C.c_uint64(0)
            _lib.check(self._lib.ucfp_text_batcher_stats(h, C.byref(b), C.byref(i)))
            tb, ti = tb + int(b.value), ti + int(i.value)
        return tb, ti - self._handed_back

    def close(self):
        for h in getattr(self, "_handles", {}).values():
            self._lib.ucfp_text_batcher_destroy(h)
        self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _raise_for(status: int):
    if status == -1:
        raise ModalityError("text has no tokens after canonicalisation")
    if status == -2:
        raise UnsupportedError(f"k - 1 tokens plus the token being read do not fit the LDS batch: every window of k "
                               f"consecutive tokens of up to {MAX_WINDOW_BYTES} bytes (separators included) is supported")
    if status != 0:
        raise ModalityError(f"text fingerprint failed with status {status}")


CONFIG_HASH_UNKNOWN = 0


def _record_config_hash(opts: TextOpts, tokenizer_tag: str, algorithm: str, supplied: Optional[int]) -> int:
    """`config_hash` of a record.  In the drop-in the Rust host keeps calling txtfp::config_hash itself (a host-side
    function of the configuration, text.rs:221,406 -- not on the hot path) and passes the value in (`supplied`).
    Without it only the carried default-MinHash constant is known; every other configuration gets
    CONFIG_HASH_UNKNOWN (0), never an invented value."""
    if supplied is not None:
        return int(supplied)
    try:
        return config_hash(opts.canonicalizer, tokenizer_tag, algorithm)
    except UnsupportedError:
        return CONFIG_HASH_UNKNOWN


def fingerprint_minhash(text: str, tenant_id: int, record_id: int) -> Record:
    return fingerprint_minhash_with(text, TextOpts(), tenant_id, record_id)


def fingerprint_minhash_with(text: str, opts: TextOpts, tenant_id: int, record_id: int,
                             config_hash_value: Optional[int] = None) -> Record:
    """text.rs:182-236 at any slot count opts.h.  Every H carries the tag `minhash-h128`, as in the
    reference (text.rs:221-228): the fingerprint's length, 8 + 8 h, tells H.  With opts.preprocess = "html" `text` is a
    page; the record's `text` is the stripped text (text.rs:751-767)."""
    (text,), opts, _ = _preprocessed([text], opts)
    recs, status = minhash_batch([text], opts)
    _raise_for(int(status[0]))
    return Record(tenant_id=tenant_id, record_id=record_id, modality=Modality.Text,
                  format_version=FORMAT_VERSION_MINHASH_HIP, algorithm=ALGORITHM_MINHASH_128,
                  config_hash=_record_config_hash(opts, opts.tokenizer_tag(), ALGORITHM_MINHASH_128, config_hash_value),
                  fingerprint=recs[0].tobytes(), embedding=None, model_id=None, metadata=b"", text=text)


def _simhash(text: str, opts: TextOpts, tag: str, tenant_id: int, record_id: int,
             config_hash_value: Optional[int] = None) -> Record:
    (text,), opts, _ = _preprocessed([text], opts)
    recs, status = simhash_batch([text], opts)
    _raise_for(int(status[0]))
    tok_tag = {"word": "word-uax29", "grapheme": "grapheme-uax29", "cjk-jp": "cjk-jp", "cjk-ko": "cjk-ko"}[opts.tokenizer]
    return Record(tenant_id=tenant_id, record_id=record_id, modality=Modality.Text, format_version=FORMAT_VERSION,
                  algorithm=tag, config_hash=_record_config_hash(opts, tok_tag, tag, config_hash_value),
                  fingerprint=recs[0].tobytes(), embedding=None, model_id=None, metadata=b"", text=text)


def fingerprint_simhash_tf(text: str, opts: TextOpts, tenant_id: int, record_id: int,
                           config_hash_value: Optional[int] = None) -> Record:
    return _simhash(text, opts, ALGORITHM_SIMHASH_TF, tenant_id, record_id, config_hash_value)


def fingerprint_simhash_idf(text: str, opts: TextOpts, idf, tenant_id: int, record_id: int,
                            config_hash_value: Optional[int] = None) -> Record:
    """text.rs:344-362.  The server always passes IdfTable::default() (handlers.rs:410): an empty table weights every
    token 1.0, i.e. TF weighting, and so does a falsy `idf` here.  A final `IdfTable` (fitted on the GPU or supplied)
    gives the weighted record of DESIGN.md T9 under the same tag; its arithmetic is this library's own (txtfp's is
    not available), bit-exact against tests/simhash_idf_ref.py.  Any other table object is refused."""
    if not idf:
        return _simhash(text, opts, ALGORITHM_SIMHASH_IDF, tenant_id, record_id, config_hash_value)
    if not isinstance(idf, IdfTable):
        raise UnsupportedError("only a ucfp_amd.text.IdfTable is built into the HIP path")
    (text,), opts, _ = _preprocessed([text], opts)
    recs, status = simhash_batch([text], opts, idf=idf)
    _raise_for(int(status[0]))
    tok_tag = {"word": "word-uax29", "grapheme": "grapheme-uax29", "cjk-jp": "cjk-jp", "cjk-ko": "cjk-ko"}[opts.tokenizer]
    return Record(tenant_id=tenant_id, record_id=record_id, modality=Modality.Text, format_version=FORMAT_VERSION,
                  algorithm=ALGORITHM_SIMHASH_IDF, config_hash=_record_config_hash(opts, tok_tag, ALGORITHM_SIMHASH_IDF, config_hash_value),
                  fingerprint=recs[0].tobytes(), embedding=None, model_id=None, metadata=b"", text=text)


def fingerprint_lsh(text: str, opts: TextOpts, tenant_id: int, record_id: int,
                    config_hash_value: Optional[int] = None) -> Record:
    rec = fingerprint_minhash_with(text, opts, tenant_id, record_id, config_hash_value)
    rec.algorithm = ALGORITHM_LSH
    return rec


def _tlsh_input(doc, opts: TextOpts) -> bytes:
    """What TLSH hashes: bytes as they are; a string's UTF-8 after canonicalisation (the reference's tokenizer tag
    "tlsh-bytes": no tokens, so non-ASCII text needs no host segmentation)."""
    if isinstance(doc, (bytes, bytearray, memoryview)):
        return bytes(doc)
    return opts.canonicalizer.apply(doc).encode("utf-8")


def tlsh_batch(texts_or_bytes: Sequence, opts: Optional[TextOpts] = None, ctx=None):
    """TLSH 128/1 of every document, one wave each (ucfp_text_tlsh_batch).
    -> (digests uint8 [n, 35], status int32 [n]): status -1 and a zero digest for a document TLSH refuses (shorter than
    50 bytes, or at most 64 of its 128 buckets non-zero)."""
    opts = opts or TextOpts()
    if opts.preprocess is not None:
        # pages: stripped on the device; a `bytes` page stays bytes, a `str` page is canonicalised after
        _check_preprocess(opts)
        texts_or_bytes = list(texts_or_bytes)
        stripped, _ = html_to_text_batch(texts_or_bytes, ctx)
        texts_or_bytes = [b.decode("utf-8", "surrogatepass") if isinstance(d, str) else b
                          for d, b in zip(texts_or_bytes, stripped)]
        opts = replace(opts, preprocess=None)
    docs = [_tlsh_input(d, opts) for d in texts_or_bytes]
    n = len(docs)
    out = np.zeros((n, TLSH_BYTES), np.uint8)
    status = np.zeros(n, np.int32)
    if n == 0:
        return out, status
    ctx = ctx or _lib.current_context()
    blob, offs = _pack(docs)
    _lib.check(_lib.load().ucfp_text_tlsh_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, out.ctypes.data,
                                                status.ctypes.data))
    return out, status


def tlsh_hex(digest) -> bytes:
    """35 digest bytes -> the 72 bytes a record stores: "T1" + 70 upper-case hex digits (text.rs:478, `sig.hex`)."""
    return b"T1" + bytes(digest).hex().upper().encode("ascii")


def tlsh_digest_bytes(d) -> bytes:
    """A digest in any of its forms -> the 35 raw bytes: raw bytes, or the 72 / 70-character hex digest (str or bytes)."""
    if isinstance(d, np.ndarray):
        d = d.astype(np.uint8).tobytes()
    if isinstance(d, (bytes, bytearray, memoryview)):
        d = bytes(d)
        if len(d) == TLSH_BYTES:
            return d
        try:
            d = d.decode("ascii")
        except UnicodeDecodeError:
            raise InvalidArgument("a TLSH digest is 35 raw bytes or 70 hex digits, with or without the T1 prefix") from None
    if not isinstance(d, str):
        raise InvalidArgument("a TLSH digest is bytes or a string")
    if len(d) == 2 * TLSH_BYTES + 2 and d[:2] in ("T1", "t1"):
        d = d[2:]
    if len(d) != 2 * TLSH_BYTES:
        raise InvalidArgument("a TLSH digest is 35 raw bytes or 70 hex digits, with or without the T1 prefix")
    try:
        return bytes.fromhex(d)
    except ValueError:
        raise InvalidArgument("a TLSH digest string must be hexadecimal") from None


def tlsh_distance(a, b) -> int:
    """The TLSH distance of two digests, 0 .. 2473 (host code: ucfp_tlsh_distance needs no device)."""
    a, b = tlsh_digest_bytes(a), tlsh_digest_bytes(b)
    return int(_lib.load().ucfp_tlsh_distance(a, b))


def fingerprint_tlsh(text: str, opts: TextOpts, tenant_id: int, record_id: int,
                     config_hash_value: Optional[int] = None) -> Record:
    """text.rs:452-484: `fingerprint` = the digest string, `text` = the prepared text (with opts.preprocess = "html" the
    text of the page, stripped on the device)."""
    (text,), opts, _ = _preprocessed([text], opts)
    digs, status = tlsh_batch([text], opts)
    if int(status[0]) != 0:
        raise ModalityError(f"TLSH refuses the document: fewer than {TLSH_MIN_BYTES} bytes after canonicalisation, or too "
                            "little variety (at most 64 of the 128 buckets used)")
    return Record(tenant_id=tenant_id, record_id=record_id, modality=Modality.Text, format_version=FORMAT_VERSION,
                  algorithm=ALGORITHM_TLSH,
                  config_hash=_record_config_hash(opts, "tlsh-bytes", ALGORITHM_TLSH, config_hash_value),
                  fingerprint=tlsh_hex(digs[0]), embedding=None, model_id=None, metadata=b"", text=text)


def _dev(a: np.ndarray):
    """Host array -> device tensor (torch is memory plumbing only)."""
    import torch
    if not torch.cuda.is_available():
        raise UnsupportedError("no HIP device: the LSH index only exists on the GPU")
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()


def _records(records) -> np.ndarray:
    """MinHash-128 records for the band index, which is built for H = 128 only (`minhash-lsh-h128`, 16 x 8 bands)."""
    if isinstance(records, (bytes, bytearray)):
        records = np.frombuffer(bytes(records), np.uint8)
    r = np.ascontiguousarray(records, dtype=np.uint8)
    if (r.ndim == 2 and r.shape[1] != MINHASH_BYTES) or r.size % MINHASH_BYTES:
        raise UnsupportedError(f"the LSH index is built for H = {DEFAULT_H} only ({MINHASH_BYTES}-byte records); these are rows of "
                               f"{r.shape[-1] if r.ndim == 2 else r.size} bytes")
    return r.reshape(-1, MINHASH_BYTES)


def lsh_band_keys(records, bands: int = 16, rows: int = 8, ctx=None) -> np.ndarray:
    """Band keys of MinHash-128 records (the reference has no band index).
    -> uint64 [n, bands].  Key spec: DESIGN.md "LSH" (slot-wise FNV fold + splitmix64 finaliser);
    computed by ucfp_text_lsh_band_keys_dev."""
    import torch
    ctx = ctx or _lib.current_context()
    r = _records(records)
    n = r.shape[0]
    d_r = _dev(r)
    d_k = torch.empty((bands, max(n, 1)), dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().ucfp_text_lsh_band_keys_dev(ctx.handle, d_r.data_ptr(), n, bands, rows, d_k.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream or None))
    return d_k[:, :n].t().contiguous().cpu().numpy().view(np.uint64)


def min_agree_for(threshold: float, h: int = DEFAULT_H) -> int:
    """Smallest slot agreement whose Jaccard estimate (agree / h) reaches `threshold`, 0 < threshold <= 1:
    max(1, ceil(threshold * h)); the product is exact in binary floating point when h is a power of two (the default 128)
    and correctly rounded otherwise."""
    t = float(threshold)
    if not 0.0 < t <= 1.0:      # also rejects NaN
        raise InvalidArgument(f"threshold must be in (0, 1] (got {threshold!r})")
    return max(1, math.ceil(t * _check_h(h)))


def minhash_agree(a, b) -> int:
    """The number of equal slots of two MinHash records of the same slot count H, 0 .. H; H is told by the records'
    length (host code: ucfp_minhash_agree_h needs no device; the headers are not compared)."""
    a, b = bytes(a), bytes(b)
    if len(a) != len(b):
        raise InvalidArgument(f"MinHash records of {len(a)} and {len(b)} bytes have different slot counts")
    return int(_lib.load().ucfp_minhash_agree_h(a, b, minhash_slots(a)))


SPAN_ALL = 0xFFFFFFFF   # dedup: every pair of a run of equal band keys


@dataclass
class DedupResult:
    """`LshIndex.dedup`: per row the smallest row of its cluster, that row's record id and whether the row is it."""
    labels: np.ndarray      # uint32 [n]
    rep_ids: np.ndarray     # uint64 [n]
    keep: np.ndarray        # bool [n]
    pairs: int              # candidate pairs over all bands (a pair counts once per band it appears in)
    clusters: int
    duplicates: int
    largest: int


class LshIndex:
    """Banded MinHash LSH shard on the GPU: `build` sorts (band key, row) per band, `query` returns
    the best k candidates by slot agreement (the MinHash Jaccard estimate), `dedup` the near-duplicate
    clusters of the built rows."""

    def __init__(self, bands: int = 16, rows: int = 8, cand_per_band: int = 64, ctx=None):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.bands, self.rows, self.cand_per_band = bands, rows, cand_per_band
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_lsh_create(self.ctx.handle, bands, rows, cand_per_band, C.byref(h)))
        self.handle = h
        self.n = 0

    def build_dev(self, ids_ptr: int, records_ptr: int, n: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_lsh_build_dev(self.handle, ids_ptr or None, records_ptr or None, n, stream or None))
        self.n = n

    def build(self, ids, records) -> None:
        import torch
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        r = _records(records)
        if r.shape[0] != ids.shape[0]:
            raise ModalityError("ids and records disagree on the number of rows")
        if ids.shape[0] == 0:
            self.build_dev(0, 0, 0)
            return
        d_ids, d_r = _dev(ids.view(np.int64)), _dev(r)
        self.build_dev(d_ids.data_ptr(), d_r.data_ptr(), ids.shape[0], torch.cuda.current_stream().cuda_stream)
        torch.cuda.current_stream().synchronize()   # the build copies what it needs; inputs may go now

    def query_dev(self, records_ptr: int, nq: int, k: int, out_ids_ptr: int, out_scores_ptr: int,
                  out_counts_ptr: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_lsh_query_dev(self.handle, records_ptr, nq, k, out_ids_ptr, out_scores_ptr,
                                                out_counts_ptr, stream or None))

    def query(self, records, k: int = 10):
        """-> (ids uint64 [nq, k] (INVALID = 2^64-1), scores float32 [nq, k], counts uint32 [nq])."""
        import torch
        r = _records(records)
        nq = r.shape[0]
        d_r = _dev(r)
        o_ids = torch.empty((max(nq, 1), k), dtype=torch.int64, device="cuda")
        o_sc = torch.empty((max(nq, 1), k), dtype=torch.float32, device="cuda")
        o_ct = torch.empty(max(nq, 1), dtype=torch.int32, device="cuda")
        self.query_dev(d_r.data_ptr(), nq, k, o_ids.data_ptr(), o_sc.data_ptr(), o_ct.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
        return (o_ids[:nq].cpu().numpy().view(np.uint64), o_sc[:nq].cpu().numpy(),
                o_ct[:nq].cpu().numpy().view(np.uint32))

    def dedup_dev(self, min_agree: int, span: int, labels_ptr: int, rep_ids_ptr: int = 0, keep_ptr: int = 0,
                  stats_ptr: int = 0, stream: int = 0) -> None:
        """Stream-ordered: labels uint32 [n] (required), rep_ids uint64 [n], keep uint8 [n], stats uint64 [4]."""
        _lib.check(self._lib.ucfp_lsh_dedup_dev(self.handle, min_agree, span, labels_ptr or None, rep_ids_ptr or None,
                                                keep_ptr or None, stats_ptr or None, stream or None))

    def dedup(self, threshold: float = 0.8, *, min_agree: Optional[int] = None, span: int = 16) -> DedupResult:
        """Near-duplicate clusters of the rows of the last build: rows that share a band key, lie within `span`
        places of each other in that key's run (SPAN_ALL: the whole run) and agree in at least `min_agree` slots
        (default: min_agree_for(threshold)) are joined; clusters are the connected components."""
        import torch
        if min_agree is None:
            min_agree = min_agree_for(threshold)
        n = self.n
        d_lab = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        d_rep = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
        d_keep = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
        d_st = torch.empty(4, dtype=torch.int64, device="cuda")
        self.dedup_dev(min_agree, span, d_lab.data_ptr(), d_rep.data_ptr(), d_keep.data_ptr(), d_st.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
        st = d_st.cpu().numpy().view(np.uint64)
        return DedupResult(d_lab[:n].cpu().numpy().view(np.uint32), d_rep[:n].cpu().numpy().view(np.uint64),
                           d_keep[:n].cpu().numpy().astype(bool), int(st[0]), int(st[1]), int(st[2]), int(st[3]))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_lsh_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dedup_corpus(texts: Sequence[str], threshold: float = 0.8, opts: Optional[TextOpts] = None, bands: int = 16,
                 rows: int = 8, span: int = 16, ctx=None):
    """The de-duplication recipe end to end: MinHash-128 of every document, a band index over the documents that
    hashed (status 0) with their position in `texts` as id, near-duplicate clusters at `threshold`.
    -> (keep bool [n], labels int64 [n] = position of the kept representative, status int32 [n]).
    A document whose status is not 0 (no tokens, oversized token) is its own cluster: kept, its own label, never
    the representative of another."""
    min_agree = min_agree_for(threshold)
    _check_preprocess(opts)                  # whatever the corpus, an empty one included
    if opts is not None and opts.h != DEFAULT_H:
        raise UnsupportedError(f"de-duplication runs on the LSH index, which is built for H = {DEFAULT_H} only (got H = {opts.h})")
    n = len(texts)
    keep = np.ones(n, bool)
    labels = np.arange(n, dtype=np.int64)
    if n == 0:
        return keep, labels, np.zeros(0, np.int32)
    rec, status = minhash_batch(texts, opts, ctx)
    pos = np.flatnonzero(status == 0)
    if pos.size:
        idx = LshIndex(bands, rows, ctx=ctx)
        try:
            idx.build(pos.astype(np.uint64), rec[pos])
            res = idx.dedup(min_agree=min_agree, span=span)
        finally:
            idx.close()
        keep[pos] = res.keep
        labels[pos] = res.rep_ids.astype(np.int64)
    return keep, labels, status
