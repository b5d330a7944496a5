"""Fixtures of the SimHash stream tests, shared by tests/test_simhash_streams_gpu.py and
tests/test_simhash_streams_spec.py so that the documents the GPU tests rely on and the properties the spec test checks
of them cannot drift.  Expected values come from the CPU oracle (TF, modes 0 and 1) and from simhash_idf_ref (weighted,
and every RAW_UTF8 document through text_canon_ref), never from the library under test."""
import numpy as np

import simhash_idf_ref as iref

RAW, PRETOK, UTF8 = 0, 1, 2
NEEDS_HOST, E_MODALITY, E_UNSUPPORTED = 1, -1, -2
Q16_ONE = 0x10000
W_MAX = 0xFFFFFFFF

EDGE_DOC = (b"It's 3.14 here: a:b and x.y. then 1,000;2 _a b_ UPPER Case mixed; don't 'quote' 1.2.3 a..b 4,5, x:y:z "
            b"The Quick brown Fox, jumps over the lazy dog's back 42 times; o'clock 7:30 pm e.g. i.e. U.S.A. end.")

_WORDS = ("the quick brown fox jumps over lazy dog it's 3.14 a:b x.y. 1,000;2 _a Upper CASE end. stream simhash wave "
          "token weight batch flush carry lane k9 0x1f q").split()
_ALNUM = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8)

# Latin with diacritics, Greek, Cyrillic, Hebrew with ' between letters, kana, Han, full-width forms, a ligature, Cf
MIXED = ("Ünï Straße l'été x ’e 1,000;2 a:b _a __ Σίσυφος Привет ש'ל مرحبا ひらがな カタカナ 漢字中文 한국어 ＡＢ１２ "
         "ﬁne so\u00adft ze\u200bro Українська 東京タワー d’un œuvre end.")


def prose(rng, n_bytes, seps=(" ", " ", " ", ", ", ". ", "\n", "  ", "; ")):
    out, size = [], 0
    while size < n_bytes:
        w = _WORDS[int(rng.integers(len(_WORDS)))] + seps[int(rng.integers(len(seps)))]
        out.append(w)
        size += len(w)
    return "".join(out)[:n_bytes].encode("ascii")


def cut(doc, sizes):
    """doc -> chunks of the given sizes in turn (the sizes repeat); never empty for an empty doc."""
    chunks, at, i = [], 0, 0
    while at < len(doc):
        chunks.append(doc[at:at + sizes[i % len(sizes)]])
        at += sizes[i % len(sizes)]
        i += 1
    return chunks or [b""]


def long_token(n, seed=3):
    return bytes(np.random.default_rng(seed).choice(_ALNUM, n))


# ---- the documents of the GPU tests

def flush_docs():
    """-> (docs, chunk lists): eight 8 KiB documents cut at the sizes around the 64-byte step, the 256-byte stage and the
    1536-byte batch and at random sizes, with empty non-final pushes; one 1000-byte token that spans four pushes."""
    rng = np.random.default_rng(2)
    docs, chunked = [], []
    for sizes in ([63], [64], [65], [255], [256], [257], [1535], [int(v) for v in rng.integers(1, 701, 64)]):
        d = prose(rng, 8192)
        c = cut(d, sizes)
        if len(c) > 4:
            c.insert(3, b"")
            c.insert(3, b"")
            c.insert(len(c) - 1, b"")
        docs.append(d)
        chunked.append(c)
    d = b"one two three " + long_token(1000) + b" four five six seven eight"
    docs.append(d)
    chunked.append(cut(d, [300]))
    return docs, chunked


LONG_TOKEN_AT, LONG_TOKEN_BYTES, LONG_TOKEN_CHUNK = 14, 1000, 300

TIE_DOC = b"alpha beta"                                    # two distinct tokens, each once: every differing bit is a tie
ZERO_DOC = b"nil nada zero nil nothing nada"               # every token weighs 0 under ZERO_WEIGHTS
ZERO_WEIGHTS = ({iref.key(t): 0 for t in (b"nil", b"nada", b"zero", b"nothing")}, Q16_ONE)


def wide_doc():
    """A few thousand tokens of a 24-word vocabulary: at weight 0xFFFFFFFF `tot` and most `pos` pass 2^32."""
    rng = np.random.default_rng(6)
    vocab = [w for w in _WORDS if w.isalnum()][:24]
    return " ".join(vocab[int(v)] for v in rng.integers(0, len(vocab), 3000)).encode("ascii")


def window_docs():
    """name -> a document around one long token of that many canonical bytes (1405 is UCFP_TEXT_MAX_WINDOW_BYTES, 1536 the
    LDS batch): `ok` must hash, `over` must be refused, the two between may go either way.  About 800 bytes of prose
    follow the token, so that pushes come after the one that meets its end."""
    tail = b" and some more after it x y z " + prose(np.random.default_rng(5), 800)
    return {name: b"a few short words first " + long_token(n, 30 + i) + tail for i, (name, n) in enumerate(WINDOW_TOKEN_BYTES.items())}


WINDOW_TOKEN_BYTES = {"ok": 1405, "between_lo": 1406, "between_hi": 1536, "over": 1537}
WINDOW_HEAD = len(b"a few short words first ")


def weights_for(docs_tokens, share=0.7, seed=11, heavy=False):
    """A table over the distinct tokens of the documents: about `share` of them get a weight of their own (zero for a
    few, `heavy`: all 0xFFFFFFFF), the others fall to the default 1.0.  -> ({key: weight}, default)."""
    rng = np.random.default_rng(seed)
    toks = sorted({bytes(t) for toks in docs_tokens for t in (toks or [])})
    weights = {}
    for i, t in enumerate(toks):
        if (7 * i + 3) % 10 < round(10 * share):            # `share` of the distinct tokens, spread over the sorted list
            r = rng.random()
            weights[iref.key(t)] = W_MAX if heavy else 0 if r < 0.08 else int(rng.integers(1, 6 * Q16_ONE))
    return weights, Q16_ONE


def weighted_share(docs_tokens, weights):
    occ = [iref.key(t) in weights for toks in docs_tokens for t in (toks or [])]
    return sum(occ) / max(1, len(occ))


# ---- expected records

def expected_ref(docs, mode, weights=None, default=Q16_ONE):
    """simhash_idf_ref's records and statuses of whole documents; weights None: every token weighs 1.0 (the TF record).
    A document the device hands back (words() is None) expects NEEDS_HOST and a zero record."""
    rec = np.zeros((len(docs), 8), np.uint8)
    st = np.zeros(len(docs), np.int32)
    for i, d in enumerate(docs):
        toks = iref.words(d, mode)
        if toks is None:
            st[i] = NEEDS_HOST
            continue
        r, s = iref.simhash_weighted(toks, weights or {}, default)
        rec[i], st[i] = np.frombuffer(r, np.uint8), s
    return rec, st


def expected_tf(oracle, docs, mode):
    """The oracle's TF records for the modes it restates (0 and 1); RAW_UTF8 stands on text_canon_ref through words()."""
    if mode == UTF8:
        return expected_ref(docs, mode)
    return oracle.text_simhash_batch(docs, mode)
