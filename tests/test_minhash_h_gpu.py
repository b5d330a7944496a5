"""MinHash with any slot count H on the GPU: every offline route of ucfp_text_minhash_h_batch and
ucfp_text_minhash_tokens_h_batch, byte for byte against the plain-Python restatement (tests/minhash_h_ref.py, itself
checked against the oracle at H = 128 in test_minhash_h_spec.py).  The slot counts leave a partial last register on both
sides of every 64 boundary and include the presets; the documents take every path of the flush.  Every case is a handful
of documents of at most 4 KiB."""
import functools

import numpy as np
import pytest

import minhash_h_ref as ref
import text_canon_ref as canon_ref
import text_grapheme_ref as gref

pytestmark = pytest.mark.gpu

HS = [16, 48, 64, 80, 128, 144, 256, 1008, 1024]
A, P, U = gref.RAW_ASCII, gref.PRETOKENIZED, gref.RAW_UTF8
WORD, GRAPHEME = gref.TOK_WORD, gref.TOK_GRAPHEME
K = 5

_WORDS = [b"alpha", b"Beta", b"gamma7", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"iota", b"kappa", b"x", b"lambda2"]


def _prose(n_tokens, seed):
    rng = np.random.default_rng(seed)
    seps = [b" ", b", ", b". ", b"\n", b" - "]
    out = b""
    for i in range(n_tokens):
        out += _WORDS[int(rng.integers(len(_WORDS)))] + (b"%d" % (i % 7) if i % 5 == 0 else b"") + seps[int(rng.integers(len(seps)))]
    return out


def _prose_bytes(n_bytes, seed):
    d = _prose(n_bytes // 4, seed)[:n_bytes]
    assert len(d) == n_bytes
    return d


# every path of the flush: no token, fewer than k, exactly k, k + 1, more than one LDS batch of 256 tokens, 4 KiB, a window
# over UCFP_TEXT_MAX_WINDOW_BYTES
ASCII_DOCS = [b"", b"alpha", b"one two three four five", b"one two three, four FIVE six", _prose(300, 3), _prose_bytes(4096, 4),
              b"short " + b"a" * 2000 + b" tail"]
ASCII_STATUS = [-1, 0, 0, 0, 0, 0, -2]
BATCHES = [[0, 1, 2, 3, 4], [5, 6, 0, 4, 3], [4]]        # n = 5, 5 and 1: never a multiple of a block's four waves


@functools.lru_cache(maxsize=None)
def _want_one(tokens, k, h, status):
    if status == -2:                                       # refused by the window limit, whatever h
        return bytes(ref.record_bytes(h)), -2
    return ref.minhash_tokens_h(tokens, k, h)


def _want(token_lists, k, h, statuses=None):
    statuses = statuses or [0] * len(token_lists)
    r = [_want_one(tuple(t), k, h, -2 if s == -2 else 0) for t, s in zip(token_lists, statuses)]
    return (np.array([np.frombuffer(b, np.uint8) for b, _ in r]).reshape(len(r), ref.record_bytes(h)),
            np.array([s for _, s in r], np.int32))


def _pack(docs):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.frombuffer(b"".join(docs) + b"\0" * 16, np.uint8).copy(), offs


def _gpu(ctx, docs, mode, tokenizer, k, h):
    from ucfp_amd import _lib
    blob, offs = _pack(docs)
    n = len(docs)
    out, st = np.full((n, ref.record_bytes(h)), 0xAB, np.uint8), np.full(n, 77, np.int32)
    _lib.check(_lib.load().ucfp_text_minhash_h_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, tokenizer, k, h,
                                                     out.ctypes.data, st.ctypes.data))
    return out, st


def _gpu_tokens(ctx, docs, k, h):
    from ucfp_amd import _lib
    blob, to, dt = gref.pack_tokens(docs)
    n = len(docs)
    out, st = np.full((n, ref.record_bytes(h)), 0xAB, np.uint8), np.full(n, 77, np.int32)
    _lib.check(_lib.load().ucfp_text_minhash_tokens_h_batch(ctx.handle, blob.ctypes.data, to.ctypes.data, dt.ctypes.data, n, k, h,
                                                            out.ctypes.data, st.ctypes.data))
    return out, st


def _same(got, want, what):
    (o, s), (wo, ws) = got, want
    assert list(s) == list(ws), what
    assert np.array_equal(o, wo), (what, [i for i in range(len(wo)) if not np.array_equal(o[i], wo[i])])


@pytest.fixture(scope="module")
def ascii_tokens(oracle):
    """The word tokens of ASCII_DOCS by the oracle's canonical stream.  The oracle's statuses do not depend on h; it has no
    LDS batch, so the window limit (-2) is the one status it does not give."""
    toks = []
    for d in ASCII_DOCS:
        stream, nt = oracle.text_canon(d, 0)
        toks.append(stream.split(b" ") if nt > 0 else [])
    _, st = oracle.text_minhash_batch(ASCII_DOCS, mode=0, k=K)
    assert [int(s) for s in st] == [0 if s == -2 else s for s in ASCII_STATUS]
    assert len(b" ".join(toks[6])) > 1405 and len(toks[6]) < K      # one window, longer than UCFP_TEXT_MAX_WINDOW_BYTES
    return toks


@pytest.mark.parametrize("h", HS)
def test_word_ascii_and_pretokenized(gpu_ctx, ascii_tokens, h):
    pre = [b" ".join(t) for t in ascii_tokens]
    for idx in BATCHES:
        toks, sts = [ascii_tokens[i] for i in idx], [ASCII_STATUS[i] for i in idx]
        _same(_gpu(gpu_ctx, [ASCII_DOCS[i] for i in idx], A, WORD, K, h), _want(toks, K, h, sts), ("ascii", h, idx))
        _same(_gpu(gpu_ctx, [pre[i] for i in idx], P, WORD, K, h), _want(toks, K, h, sts), ("pretokenized", h, idx))


LATIN = "Éric a dîné à l'Öl-café: «naïve» façade, Ångström straße ĳ ﬁn. " * 9
HAN = "日本語の文章 漢字仮名交じり文 東京都 一二三 " * 12
UTF8_DOCS = [LATIN, HAN, "é", "", LATIN[:70] + HAN[:40]]


@pytest.mark.parametrize("h", HS)
def test_word_utf8(gpu_ctx, h):
    toks = [[t.encode("utf-8") for t in canon_ref.tokens(s)] for s in UTF8_DOCS]
    assert all(len(toks[i]) > K for i in (0, 1))
    docs = [s.encode("utf-8") for s in UTF8_DOCS]
    _same(_gpu(gpu_ctx, docs, U, WORD, K, h), _want(toks, K, h), ("utf8", h))
    _same(_gpu(gpu_ctx, docs[1:2], U, WORD, 3, h), _want(toks[1:2], 3, h), ("utf8 n = 1", h))


@pytest.mark.parametrize("h", HS)
def test_graphemes(gpu_ctx, h):
    docs_a = [b"", b"ab", b"abcde", b"abc\r\ndef", ASCII_DOCS[4][:700]]          # 700 clusters: three LDS batches
    docs_u = [s.encode("utf-8") for s in (LATIN[:300], HAN[:150], "é", "", "a\r\n日")]
    for docs, mode in ((docs_a, A), (docs_u, U)):
        toks = [gref.device_clusters(d, mode) for d in docs]
        assert all(t is not None for t in toks)
        _same(_gpu(gpu_ctx, docs, mode, GRAPHEME, K, h), _want(toks, K, h), ("grapheme", mode, h))
        _same(_gpu(gpu_ctx, docs[4:], mode, GRAPHEME, 2, h), _want(toks[4:], 2, h), ("grapheme n = 1", mode, h))


@pytest.mark.parametrize("h", HS)
def test_caller_tokens(gpu_ctx, h):
    docs = [[b"new york", b"is", b"a", b"city", b"\x00", b"of two words"], [], [b"one"], [b"a b", b"", b"c"],
            [b"t%d x" % i for i in range(300)]]
    _same(_gpu_tokens(gpu_ctx, docs, K, h), _want(docs, K, h), ("tokens", h))
    _same(_gpu_tokens(gpu_ctx, docs[:1], 2, h), _want(docs[:1], 2, h), ("tokens n = 1", h))


def test_128_is_the_old_entry_and_smaller_h_is_a_prefix(gpu_ctx):
    from ucfp_amd import _lib
    lib = _lib.load()
    blob, offs = _pack(ASCII_DOCS)
    n = len(ASCII_DOCS)
    old, old_st = np.zeros((n, 1032), np.uint8), np.zeros(n, np.int32)
    _lib.check(lib.ucfp_text_minhash_batch(gpu_ctx.handle, blob.ctypes.data, offs.ctypes.data, n, A, K, old.ctypes.data,
                                           old_st.ctypes.data))
    r128, s128 = _gpu(gpu_ctx, ASCII_DOCS, A, WORD, K, 128)
    r64, s64 = _gpu(gpu_ctx, ASCII_DOCS, A, WORD, K, 64)
    r256, s256 = _gpu(gpu_ctx, ASCII_DOCS, A, WORD, K, 256)
    assert list(old_st) == list(s128) == list(s64) == list(s256) == ASCII_STATUS
    assert np.array_equal(r128, old)
    assert np.array_equal(r64[:, 8:], old[:, 8:520]) and np.array_equal(r64[:, :8], old[:, :8])
    assert np.array_equal(r256[:, 8:520], r64[:, 8:]) and np.array_equal(r256[:, 8:1032], old[:, 8:])


@pytest.mark.parametrize("h", [16, 80, 1008])
def test_dev_entry_unaligned_output_and_canary(gpu_ctx, torch_cuda, ascii_tokens, h):
    """The _dev entry writes rows 8 + 8 h bytes apart into a buffer that is only 4-byte aligned, and nothing behind the last
    record: the lanes whose slot is not below h store nothing."""
    from ucfp_amd import _lib
    torch = torch_cuda
    idx = [4, 1, 6, 0, 5]
    docs = [ASCII_DOCS[i] for i in idx]
    blob, offs = _pack(docs)
    n, rec = len(docs), ref.record_bytes(h)
    d_blob, d_offs = torch.from_numpy(blob).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    canary = 4096
    buf = torch.full((4 + n * rec + canary,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 8 == 0
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().ucfp_text_minhash_h_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, A, WORD, K, h,
                                                         buf.data_ptr() + 4, st.data_ptr(), stream or None))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:4] == 0xAB).all() and (got[4 + n * rec:] == 0xAB).all()
    want = _want([ascii_tokens[i] for i in idx], K, h, [ASCII_STATUS[i] for i in idx])
    _same((got[4:4 + n * rec].reshape(n, rec), st.cpu().numpy()), want, ("dev", h))


def test_invalid_h_is_refused_by_the_c_abi(gpu_ctx):
    from ucfp_amd import _lib
    from ucfp_amd.errors import InvalidArgument
    for h in (0, 8, 17, 1040):
        with pytest.raises(InvalidArgument):
            _gpu(gpu_ctx, [b"a b c"], A, WORD, K, h)
        with pytest.raises(InvalidArgument):
            _gpu_tokens(gpu_ctx, [[b"a"]], K, h)


def test_presets_through_fingerprint_minhash_with(gpu_ctx, ascii_tokens):
    """The reference's presets high-recall (k = 3, h = 256) and fast (k = 7, h = 64), algorithms_manifest.rs:280-328."""
    from ucfp_amd import text
    doc = ASCII_DOCS[5].decode("ascii")
    for k, h, size in ((3, 256, 2056), (7, 64, 520)):
        r = text.fingerprint_minhash_with(doc, text.TextOpts(k=k, h=h), 1, 2)
        assert len(r.fingerprint) == size and r.algorithm == "minhash-h128"      # the reference tags every H so (text.rs:221-228)
        assert r.fingerprint == ref.minhash_tokens_h(ascii_tokens[5], k, h)[0]
        assert text.minhash_slots(r.fingerprint) == h
        lsh = text.fingerprint_lsh(doc, text.TextOpts(k=k, h=h), 1, 2)
        assert lsh.fingerprint == r.fingerprint and lsh.algorithm == "minhash-lsh-h128"
    # every route of minhash_batch honours opts.h: raw ASCII, device UTF-8, host hand-backs (a non-default canonicaliser)
    texts = [doc, LATIN, HAN]
    for tokenizer in ("word", "grapheme"):
        o, s = text.minhash_batch(texts, text.TextOpts(tokenizer=tokenizer, h=80), gpu_ctx)
        assert o.shape == (3, 648) and not s.any()
        canon = text.Canonicalizer(normalization="nfc")
        o2, s2 = text.minhash_batch(texts[1:], text.TextOpts(canonicalizer=canon, tokenizer=tokenizer, h=80), gpu_ctx)
        assert o2.shape == (2, 648) and not s2.any()
        o3, _ = text.minhash_batch(texts[1:], text.TextOpts(canonicalizer=canon, tokenizer=tokenizer, h=144), gpu_ctx)
        assert np.array_equal(o3[:, :648], o2)                                   # the prefix property across two kernels
