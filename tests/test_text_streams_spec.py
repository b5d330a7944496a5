"""Streaming MinHash without a GPU: the cut rule of the host route against whole-text tokenisation, the
size of a stream's device state, and the checks that run before any device work."""
import ctypes as C
import random

import pytest

from ucfp_amd import _lib
from ucfp_amd import text as T
from ucfp_amd.errors import ModalityError

UCFP_E_MODALITY, UCFP_E_UNSUPPORTED, UCFP_E_INDEX, UCFP_E_INVALID = -1, -2, -3, -4

# what a cut could go wrong on: word-internal punctuation, marks that combine backwards, ignorables, pairs that join
# (regional indicators, jamo), characters whose case fold or NFKC form is longer or context-dependent, non-ASCII spaces
ALPHABET = (list("abcxyzABZ019") + list("_'\u2019.,:;") + ["\u0301", "\u0308", "\u0327", "\u05b0", "\u3099"] +
            ["\u200d", "\u200b", "\u00ad", "\ufeff"] + ["\U0001f1e9", "\U0001f1ea", "\U0001f1eb"] +
            list("\u05d0\u05d1\u05e9") + list("\u30ab\u30bf\u304b\u30fc") + list("\u4e2d\u6587") +
            ["\u1100", "\u1161", "\u11a8", "\ud55c"] + ["\ufb01", "\ufb03", "\u00df", "\u0130", "\u03a3", "\u03c2"] +
            ["\uff21", "\uff11", "\u3000", "\u00a0", "\u2003", "\u2028", "\u0085"])
SPACES = [" ", "\n", "\t", "\r"]


def _stream_tokens(s, rng, canon):
    """The token list a session builds when `s` arrives in chunks of random size: cut, tokenise the head, keep the tail."""
    toks, tail, at = [], "", 0
    while at < len(s):
        step = rng.randint(1, 9)
        tail += s[at:at + step]
        at += step
        whole = tail
        head, tail = T._stream_cut(whole)
        assert head + tail == whole
        assert head == "" or tail[0] in " \n\t\r"
        if head:
            toks += T._host_tokens(canon.apply(head))
    return toks + T._host_tokens(canon.apply(tail))


def test_stream_cut_keeps_the_token_list():
    pytest.importorskip("regex", reason="the host tokeniser needs the `regex` module")
    rng = random.Random(20241019)
    canons = [T.Canonicalizer(), T.Canonicalizer(normalization="nfc", case_fold=False), T.Canonicalizer(normalization="none")]
    cuts = 0
    for i in range(20000):
        n = rng.randint(1, 40)
        s = "".join(rng.choice(SPACES) if rng.random() < 0.18 else rng.choice(ALPHABET) for _ in range(n))
        canon = canons[i % 3] if i % 5 == 0 else canons[0]
        want = T._host_tokens(canon.apply(s))
        assert _stream_tokens(s, rng, canon) == want, repr(s)
        cuts += sum(s.count(ch) for ch in SPACES)
    assert cuts > 50000     # the strings do hold places to cut at


def test_stream_cut_edges():
    assert T._stream_cut("") == ("", "")
    assert T._stream_cut("abc") == ("", "abc")                  # no whitespace: held whole
    assert T._stream_cut(" abc") == ("", " abc")                # nothing before the only whitespace
    assert T._stream_cut("ab cd\tef") == ("ab cd", "\tef")      # the LAST one, whichever of the four it is
    assert T._stream_cut("ab \r\n") == ("ab \r", "\n")
    assert T._stream_cut("a\u00a0b\u3000c") == ("", "a\u00a0b\u3000c")   # only ASCII whitespace is a cut


def test_state_bytes():
    n = _lib.load().ucfp_text_streams_state_bytes()
    assert 128 * 8 + 1536 < n <= 4096       # the minima and one LDS batch of canonical bytes, within 4 KiB


def test_create_needs_a_device_and_a_valid_k():
    import torch
    lib = _lib.load()
    h = C.c_void_p()
    for k in (0, 65):                       # checked before anything else, with the offline entry's message
        assert lib.ucfp_text_streams_create(None, k, 4, C.byref(h)) == UCFP_E_MODALITY
        assert b"shingle k must be in [1, 64]" in lib.ucfp_last_error()
    rc = lib.ucfp_text_streams_create(None, 5, 4, C.byref(h))
    # no context can exist without a device: there the answer is "no device", with one it is the NULL context
    assert rc == (UCFP_E_INVALID if torch.cuda.is_available() else UCFP_E_INDEX), lib.ucfp_last_error()
    assert not h.value
    # a NULL set: status codes, no crash
    slot = C.c_uint32(0)
    assert lib.ucfp_text_streams_open(None, 0, C.byref(slot)) == UCFP_E_INVALID
    assert lib.ucfp_text_streams_close(None, 0) == UCFP_E_INVALID
    assert lib.ucfp_text_streams_push(None, 0, None, 0, 1, None, None) == UCFP_E_INVALID
    assert lib.ucfp_text_streams_push_dev(None, None, None, None, 0, None, None, None, None) == UCFP_E_INVALID
    lib.ucfp_text_streams_destroy(None)


def test_ndjson_body_is_checked_before_any_device_work():
    opts = T.TextOpts()
    for body in (b'"a b c"\n42\n', b'"a"\n{"x": "y"}\n', b'"a"\r\n["b"]\n', b'"a"\nnull\n', b'"a"\nnot json\n', b'"a"\n"b\n'):
        with pytest.raises(ModalityError, match="NDJSON line"):
            T.ingest_stream_ndjson(body, opts, 1, 2)
    for body in (b"", b"\n\n", b"\r\n\n\r\n"):
        with pytest.raises(ModalityError, match="produced no record"):
            T.ingest_stream_ndjson(body, opts, 1, 2)
    assert T._ndjson_chunks(b'"a"\r\n\n"b \\u00e9"\n') == [b"a", "b \u00e9".encode()]
