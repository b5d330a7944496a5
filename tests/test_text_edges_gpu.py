"""GPU parity at the edges of text_hash_kernel (ucfp_amd/csrc/text.hip) vs the CPU oracle, bit-exact on records and status.

tests/test_text_gpu.py feeds the kernel short-word prose only: its longest shingle is 83 bytes, its LDS batches fill by
token count, and the only refused document is one 5000-byte token.  This file drives what that leaves out:

  1  every length class of the XXH3 that reads the canonical stream from LDS (xxh3_lds), at every alignment of the
     shingle / token start (`sh = address & 3` of xxh3_lds_rd64 / _rd32), raw and pre-tokenised;
  2  batches that fill by BYTES, so flushes carry long byte ranges to the front of the batch;
  3  both sides of the UCFP_E_UNSUPPORTED (-2) limit, UCFP_TEXT_MAX_WINDOW_BYTES, at all 64 step phases;
  4  mid-letter / mid-number punctuation on the 64-byte step and 256-byte stage boundaries and at a document's end;
  5  a NUL byte inside a pre-tokenised token.

Every test first asserts, from oracle.text_canon alone, that its inputs have the property it is about, so an edit to a
generator cannot lose the coverage unnoticed.  All inputs are deterministic (one fixed byte pool, no other randomness).
"""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAW, PRETOK = 0, 1
LIMIT = 1405          # UCFP_TEXT_MAX_WINDOW_BYTES; test_limit_constant_is_quoted pins it to the header and text.py
CANON_CAP = 1536      # kCanonCap of text.hip: no window longer than the LDS batch can ever be hashed
TOK_FLUSH = 224       # the token cap flushes a batch at 224 tokens (ntok + 33 > 256)

# xxh3_lds: 1-3 / 4-8 / 9-16 / 17-128 with its branches at 32, 64 and 96 / 129-240 / > 240 without and with a full
# 1024-byte block (the scramble).  Length 0 is unreachable: a token has at least one byte.
CLASSES = [(1, 3), (4, 8), (9, 16), (17, 32), (33, 64), (65, 96), (97, 128), (129, 240), (241, 1024), (1025, LIMIT)]
LENGTHS = list(range(1, 261)) + [511, 512, 513, 1023, 1024, 1025, 1087, 1088, 1089, 1400]

_ALNUM = b"abcdefghijklmnopqrstuvwxyz0123456789"
_POOL = None


def _word(n, salt):
    """n varied lower-case letters and digits; deterministic in (n, salt)."""
    global _POOL
    if _POOL is None:
        idx = np.random.default_rng(20240611).integers(0, len(_ALNUM), 1 << 18)
        _POOL = np.frombuffer(_ALNUM, np.uint8)[idx].tobytes()
    at = (salt * 2654435761 + 12345) % (len(_POOL) - n)
    return _POOL[at:at + n]


def _high_bytes(doc):
    """The same tokens with every 7th byte (spaces excepted) moved to 0x80..0xff: only legal PRETOKENIZED."""
    a = np.frombuffer(doc, np.uint8).copy()
    m = (np.arange(a.size) % 7 == 3) & (a != 32)
    a[m] |= 0x80
    return a.tobytes()


def _class_of(n):
    for i, (lo, hi) in enumerate(CLASSES):
        if lo <= n <= hi:
            return i
    raise AssertionError(f"length {n} is in no class")


def _spans(oracle, doc, mode):
    """-> (token starts, token lengths, stream length) of the oracle's canonical stream."""
    cs, nt = oracle.text_canon(doc, mode)
    assert nt >= 0
    if nt == 0:
        assert cs == b""
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    lens = np.array([len(t) for t in cs.split(b" ")], np.int64)
    assert lens.size == nt and lens.min() > 0
    starts = np.concatenate(([0], np.cumsum(lens + 1)[:-1]))
    return starts, lens, len(cs)


def _windows(starts, lens, k):
    """(start, length) in the canonical stream of every item the kernel hashes: k-token shingles, the whole document
    when it has fewer than k tokens; k = 1 gives SimHash's single tokens."""
    n = lens.size
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    ends = starts + lens
    if n < k:
        return starts[:1], ends[-1:] - starts[:1]
    return starts[:n - k + 1], ends[k - 1:] - starts[:n - k + 1]


def _no_flush(stream_len, ntok):
    """The kernel flushes mid-document only when `cbase + ntok` (stream length in use + 1) exceeds LIMIT + 1 or 224
    tokens are open; a document below both is hashed from one batch, where LDS offset = canonical-stream offset (the
    stream starts 4-byte aligned in LDS), so `sh` of a read is its stream offset & 3."""
    return stream_len <= LIMIT and ntok < TOK_FLUSH


def _gpu(kind, docs, mode, k):
    from ucfp_amd import text
    return text._run(kind, docs, mode, k)


def _ref(oracle, kind, docs, mode, k):
    if kind == "simhash":
        return oracle.text_simhash_batch(docs, mode=mode)
    return oracle.text_minhash_batch(docs, mode=mode, k=k)


def _assert_exact(oracle, kind, docs, mode, k, want_status=None):
    g, gs = _gpu(kind, docs, mode, k)
    o, os_ = _ref(oracle, kind, docs, mode, k)
    if want_status is not None:
        assert (os_ == want_status).all()
    bad_st = np.flatnonzero(gs != os_)
    assert bad_st.size == 0, f"{kind} k={k} mode={mode}: status of docs {bad_st[:8].tolist()}: {gs[bad_st[:8]].tolist()} != {os_[bad_st[:8]].tolist()}"
    bad = np.flatnonzero((g != o).any(axis=1))
    assert bad.size == 0, f"{kind} k={k} mode={mode}: {bad.size} records differ, first docs {bad[:8].tolist()}"


def test_limit_constant_is_quoted():
    from ucfp_amd import text
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ucfp_hip.h")).read()
    m = re.search(r"^#define UCFP_TEXT_MAX_WINDOW_BYTES (\d+)$", hdr, re.M)
    assert m and int(m.group(1)) == LIMIT == text.MAX_WINDOW_BYTES
    with pytest.raises(text.UnsupportedError, match=str(LIMIT)):
        text._raise_for(-2)
    assert f"= {LIMIT} =" in open(os.path.join(root, "DESIGN.md")).read()


# ---------------------------------------------------------------------------------------------------------------------
# 1. XXH3-over-LDS length classes
# ---------------------------------------------------------------------------------------------------------------------

def _split(total, k, salt):
    """k token lengths whose joined length (k - 1 separators) is `total`: k - 1 short ones and the rest in one."""
    short = []
    room = total - (k - 1) - k          # token bytes beyond one per token
    for j in range(k - 1):
        extra = min(room, (salt + j) % 3)
        short.append(1 + extra)
        room -= extra
    big = total - (k - 1) - sum(short)
    return short + [big] if salt % 2 else [big] + short


def _simhash_docs():
    """3 tokens; the middle one has length L and starts at stream offset 2..5, i.e. at every offset mod 4."""
    docs = []
    for L in LENGTHS:
        for v in range(4):
            docs.append(b" ".join([_word(1 + v, L + v), _word(L, 7 * L + v), _word(1 + (L + v) % 5, L + 11)]))
    return docs


def _minhash_docs(k):
    """1..4 leading bytes of another token, then k tokens of joined length L: the second shingle has length L and
    starts at stream offset 2..5.  L < 2k - 1 cannot be the length of k tokens."""
    docs = []
    for L in LENGTHS:
        if L < 2 * k - 1:
            continue
        for p in range(1, 5):
            toks = [_word(p, L + p)] + [_word(n, 13 * L + 5 * p + j) for j, n in enumerate(_split(L, k, L + p))]
            docs.append(b" ".join(toks))
    return docs


def _census(oracle, docs, mode, k, min_class):
    """Every (length class >= min_class, start & 3) of a hashed item occurs, counting only single-batch documents."""
    seen = np.zeros((len(CLASSES), 4), np.int64)
    lengths = set()
    for d in docs:
        starts, lens, slen = _spans(oracle, d, mode)
        if not _no_flush(slen, lens.size):
            continue
        ws, wl = _windows(starts, lens, k)
        for s, n in zip(ws.tolist(), wl.tolist()):
            seen[_class_of(n), s & 3] += 1
            lengths.add(n)
    missing = [(CLASSES[c], sh) for c in range(min_class, len(CLASSES)) for sh in range(4) if not seen[c, sh]]
    assert not missing, f"k={k} mode={mode}: (class, sh) never hashed: {missing}"
    return lengths


@pytest.mark.parametrize("mode", [RAW, PRETOK], ids=["raw", "pretok"])
def test_xxh3_lds_length_classes_simhash(gpu_ctx, oracle, mode):
    docs = _simhash_docs()
    if mode == PRETOK:
        docs = [_high_bytes(d) for d in docs]
        assert sum(max(d) >= 0x80 for d in docs) > 0.9 * len(docs)
    assert all(_spans(oracle, d, mode)[1].size == 3 for d in docs)
    assert set(LENGTHS) <= _census(oracle, docs, mode, 1, 0)
    _assert_exact(oracle, "simhash", docs, mode, 1, want_status=0)


@pytest.mark.parametrize("mode", [RAW, PRETOK], ids=["raw", "pretok"])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_xxh3_lds_length_classes_minhash(gpu_ctx, oracle, k, mode):
    """k = 1 and k = 2 reach every class; k tokens are at least 2k - 1 bytes, so k = 5 starts at class 9-16."""
    docs = _minhash_docs(k)
    if mode == PRETOK:
        docs = [_high_bytes(d) for d in docs]
        assert sum(max(d) >= 0x80 for d in docs) > 0.9 * len(docs)
    lengths = _census(oracle, docs, mode, k, _class_of(2 * k - 1))
    assert {L for L in LENGTHS if L >= 2 * k - 1} <= lengths
    _assert_exact(oracle, "minhash", docs, mode, k, want_status=0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. flushes under byte pressure, the carry copy
# ---------------------------------------------------------------------------------------------------------------------

def _dense_docs(k_max):
    """64 documents of 4-12 KiB, 0..63 leading spaces, single spaces between tokens, every window of k_max tokens within
    LIMIT.  k_max = 9: one token of 150-250 bytes in every 9, the others 60-140 (8 * 140 + 250 + 8 = 1378).
    k_max = 64: one token of 60-250 bytes in every 64, the others 4-17, mostly 14-17 (63 * 17 + 250 + 63 = 1384) -- 64 tokens and 63
    separators within 1405 bytes cannot average more than 20.9 bytes a token."""
    docs = []
    for lead in range(64):
        size = 4096 + (lead * 131) % 7900
        toks, used, i = [], lead, 0
        while used < size:
            r = int.from_bytes(_word(2, 1000 * lead + i), "little")
            if i % k_max == lead % k_max:
                n = (150 if k_max == 9 else 60) + r % (101 if k_max == 9 else 191)
            else:
                n = 60 + r % 81 if k_max == 9 else (4 + r % 14 if i % 7 == 3 else 17 - r % 4)
            toks.append(_word(n, 77 * lead + i))
            used += n + 1
            i += 1
        docs.append(b" " * lead + b" ".join(toks))
    return docs


def _mixed_docs():
    """64 documents of 4-12 KiB that alternate runs of one-letter tokens (up to 240: the token cap flushes) with pairs of
    300-600-byte tokens (the byte cap flushes).  Pairs are at least 64 tokens apart, so a window of up to 64 tokens
    holds at most two long tokens: 2 * 600 + 62 + 63 = 1325 <= LIMIT."""
    docs = []
    for lead in range(64):
        size = 4096 + (lead * 197) % 6400
        toks, used, seg = [], lead, 0
        while used < size:
            r = int.from_bytes(_word(2, 3000 * lead + seg), "little")
            run = (240, 64, 100, 230)[(seg + lead) % 4]
            toks += [_word(1, 50 * lead + seg + j) for j in range(run)]
            toks += [_word(300 + (r + 97 * j) % 301, 9 * lead + seg + j) for j in range(2)]
            used += 2 * run + sum(len(t) + 1 for t in toks[-2:])
            seg += 1
        docs.append(b" " * lead + b" ".join(toks))
    return docs


def _byte_pressure_census(oracle, docs, ks, min_mean, tok_range):
    for lead, d in enumerate(docs):
        assert 4096 <= len(d) <= 12 * 1024 and len(d) - len(d.lstrip(b" ")) == lead
        starts, lens, slen = _spans(oracle, d, RAW)
        for k in ks:
            assert _windows(starts, lens, k)[1].max() <= LIMIT, (lead, k)
        assert lens.mean() >= min_mean, (lead, lens.mean())
        assert tok_range[0] <= lens.min() and lens.max() <= tok_range[1]
        # the byte cap comes first: no 224 consecutive tokens fit the bytes of one batch
        assert _windows(starts, lens, min(TOK_FLUSH, lens.size))[1].min() > LIMIT + 1, lead


@pytest.fixture(scope="module")
def dense9():
    return _dense_docs(9)


@pytest.fixture(scope="module")
def dense64():
    return _dense_docs(64)


@pytest.fixture(scope="module")
def mixed():
    return _mixed_docs()


@pytest.mark.parametrize("kind,k", [("minhash", 1), ("minhash", 2), ("minhash", 5), ("minhash", 9), ("simhash", 1)])
def test_flush_under_byte_pressure(gpu_ctx, oracle, dense9, kind, k):
    """Tokens of 60-250 bytes, mean >= 48: every flush is a byte-cap flush and carries up to k - 1 long tokens."""
    _byte_pressure_census(oracle, dense9, [1, 2, 5, 9], 48, (60, 250))
    _assert_exact(oracle, kind, dense9, RAW, k, want_status=0)


@pytest.mark.parametrize("kind,k", [("minhash", 64), ("minhash", 9), ("simhash", 1)])
def test_flush_under_byte_pressure_k64(gpu_ctx, oracle, dense64, kind, k):
    """k = 64 cannot have both windows within the limit and a mean token length of 48 (64 tokens + 63 separators in 1405
    bytes average at most 20.9), so these documents are as dense as k = 64 allows: mean >= 10 bytes a token, which
    still reaches the byte cap long before 224 tokens.  Every flush carries 63 tokens, about 1.3 KiB: the carry copy
    runs some 20 passes of 64 bytes."""
    _byte_pressure_census(oracle, dense64, [1, 9, 64], 10, (4, 250))
    for d in dense64[:8]:
        starts, lens, _ = _spans(oracle, d, RAW)
        assert _windows(starts, lens, 63)[1].max() > 1100        # the carried range is most of the batch
    _assert_exact(oracle, kind, dense64, RAW, k, want_status=0)


@pytest.mark.parametrize("kind,k", [("minhash", 1), ("minhash", 2), ("minhash", 5), ("minhash", 9), ("minhash", 64),
                                    ("simhash", 1)])
def test_flush_caps_alternate(gpu_ctx, oracle, mixed, kind, k):
    """Runs of one-letter tokens fill a batch by tokens, pairs of 300-600-byte tokens fill it by bytes."""
    for lead, d in enumerate(mixed):
        assert 4096 <= len(d) <= 12 * 1024 and len(d) - len(d.lstrip(b" ")) == lead
        starts, lens, _ = _spans(oracle, d, RAW)
        for kk in (1, 2, 5, 9, 64):
            assert _windows(starts, lens, kk)[1].max() <= LIMIT
        assert set(np.unique(lens[lens < 300]).tolist()) == {1} and lens.max() <= 600 and (lens >= 300).sum() >= 4
        w224 = _windows(starts, lens, TOK_FLUSH)[1]
        assert w224.min() <= LIMIT and w224.max() > LIMIT + 1     # some batches fill by tokens, some by bytes
    _assert_exact(oracle, kind, mixed, RAW, k, want_status=0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the -2 contract, both sides
# ---------------------------------------------------------------------------------------------------------------------

_SHORT = [b"the quick brown fox jumps over the lazy dog", b"one two", b"x", b"Don't stop 3.14 me_now a:b"]


def _window_doc(W, phase, k, ntok, trailing):
    """`phase` spaces, then ntok tokens of joined length W in one of three shapes (short ones first, the long one first,
    near-equal), then optionally one more one-byte token, which makes no window longer than W."""
    shape = (W + phase) % 3
    if ntok == 1:
        lens = [W]
    elif shape == 2:
        body = W - (ntok - 1)
        lens = [body // ntok + (1 if j < body % ntok else 0) for j in range(ntok)]
    else:
        lens = _split(W, ntok, 2 * (W + phase) + shape)
    assert sum(lens) + ntok - 1 == W and min(lens) >= 1
    toks = [_word(n, 31 * W + 7 * phase + j) for j, n in enumerate(lens)]
    if trailing:
        toks.append(b"z")
    return b" " * phase + b" ".join(toks)


def _sweep(ws, k, ntok):
    """Sweep documents at every third place, short normal documents between them: the sweep documents visit all four
    wave positions of a block.  -> (docs, indices of the sweep documents)."""
    docs, at = [], []
    for W in ws:
        for phase in range(64):
            at.append(len(docs))
            docs.append(_window_doc(W, phase, k, ntok, trailing=ntok >= k and (W + phase) % 2 == 0))
            docs += [_SHORT[(W + phase) % 4], _SHORT[(W + phase + 1) % 4]]
    return docs, np.array(at)


def _check_contract(oracle, kind, k, docs, at, ws):
    # what the inputs are, from the canonical stream alone
    wmax = np.zeros(at.size, np.int64)
    for j, i in enumerate(at):
        starts, lens, _ = _spans(oracle, docs[i], RAW)
        assert starts.size and len(docs[i]) - len(docs[i].lstrip(b" ")) == j % 64
        wmax[j] = _windows(starts, lens, k)[1].max()
    assert np.array_equal(wmax, np.repeat(np.array(ws), 64))            # every W at every phase 0..63
    assert wmax.min() <= LIMIT - 40 and wmax.max() >= LIMIT + 140 and (wmax > CANON_CAP).any()
    g, gs = _gpu(kind, docs, RAW, k)
    o, os_ = _ref(oracle, kind, docs, RAW, k)
    assert not os_.any()
    same = (g == o).all(axis=1)
    zero = ~g.any(axis=1)
    sw_st, sw_same, sw_zero = gs[at], same[at], zero[at]
    # never a wrong record: status 0 with the oracle's bytes, or -2 with zeros
    assert np.isin(sw_st, (0, -2)).all(), np.unique(sw_st)
    wrong = np.flatnonzero(~np.where(sw_st == 0, sw_same, sw_zero))
    assert wrong.size == 0, f"wrong record at (W, phase) {[(int(wmax[j]), int(j % 64)) for j in wrong[:8]]}"
    refused_ok = np.flatnonzero((sw_st != 0) & (wmax <= LIMIT))
    assert refused_ok.size == 0, f"refused within the limit: (W, phase) {[(int(wmax[j]), int(j % 64)) for j in refused_ok[:8]]}"
    hashed_big = np.flatnonzero((sw_st == 0) & (wmax > CANON_CAP))
    assert hashed_big.size == 0, f"hashed beyond the batch: W {wmax[hashed_big[:8]].tolist()}"
    # neighbours of refused documents are untouched, and refused documents sat in every wave position of a block
    others = np.setdiff1d(np.arange(len(docs)), at)
    assert not gs[others].any() and same[others].all()
    assert set((at[sw_st == -2] % 4).tolist()) == {0, 1, 2, 3}
    return wmax, sw_st


@pytest.mark.parametrize("kind,k", [("minhash", 1), ("minhash", 5), ("minhash", 64), ("simhash", 1)])
def test_unsupported_contract_sweep(gpu_ctx, oracle, kind, k):
    """Window lengths LIMIT - 40 .. LIMIT + 140 at start phases 0..63: exact up to LIMIT, exact or refused above it,
    refused beyond the LDS batch."""
    ws = list(range(LIMIT - 40, LIMIT + 141))
    docs, at = _sweep(ws, k, k)
    wmax, st = _check_contract(oracle, kind, k, docs, at, ws)
    first = int(wmax[st == -2].min())
    always = int(wmax[st == 0].max()) + 1
    print(f"{kind} k={k}: first -2 at W={first}, -2 at every phase from W={always}")
    assert first > LIMIT


@pytest.mark.parametrize("k,ntok", [(5, 3), (64, 10), (64, 63)])
def test_fewer_than_k_tokens_at_the_limit(gpu_ctx, oracle, k, ntok):
    """A document of fewer than k tokens is one shingle: below the limit it is hashed from one batch, above it the
    first flush can consume nothing (`keep_from == 0`) and the document must be refused, not truncated."""
    ws = list(range(LIMIT - 40, LIMIT + 141))
    docs, at = _sweep(ws, k, ntok)
    for i in at[::97]:
        assert _spans(oracle, docs[i], RAW)[1].size == ntok < k
    _check_contract(oracle, "minhash", k, docs, at, ws)


# ---------------------------------------------------------------------------------------------------------------------
# 4. directed tokeniser edges
# ---------------------------------------------------------------------------------------------------------------------

PATTERNS = [b"a.b", b"a'b", b"a:b", b"1,2", b"1.2", b"1;2", b"a.1", b"1.a", b"a..b", b"a.", b".a", b"1,", b"A.B", b"a_b",
            b"a_.b"]
PUNCT_AT = [62, 63, 64, 65, 254, 255, 256, 257, 510, 511, 512, 513]


def _punct_index(pat):
    return min(i for i, c in enumerate(pat) if c in b".':,;_")


def _filler(n, kind):
    if kind == 0:
        return b" " * n                                   # no token open at the step boundary
    if kind == 1:
        return _word(n, n)                                # one token open across every boundary before the pattern
    return (b"ab " * (n // 3 + 1))[:n]                     # tokens ending at, before and after boundaries


def _edge_docs():
    docs, meta = [], []
    for pat in PATTERNS:
        pi = _punct_index(pat)
        for at in PUNCT_AT:
            for fk in range(3):
                head = _filler(at - pi, fk)
                ends = [head + pat[:pi + 1]] + [head + pat + b"e f1"[:t] for t in range(5)]
                for e in ends:
                    assert e[at] == pat[pi]
                    for follower in (b"b next doc", b"2 next doc"):
                        meta.append((pat, at, fk, len(e) - at - 1))
                        docs += [e, follower]
                        if len(docs) % 7 == 0:
                            docs.append(b"")
    return docs, meta


@pytest.mark.parametrize("kind,k", [("minhash", 1), ("minhash", 5), ("simhash", 1)])
def test_tokeniser_boundaries(gpu_ctx, oracle, kind, k):
    """Punctuation that joins or splits tokens depending on (prev, cur, next), placed on lanes 62..1 of a 64-byte step,
    on the 256-byte stage boundary and on the last byte of a document whose successor in the blob would join it."""
    docs, meta = _edge_docs()
    assert {(p, a, f) for p, a, f, _ in meta} == {(p, a, f) for p in PATTERNS for a in PUNCT_AT for f in range(3)}
    assert {m[3] for m in meta} >= {0, 1, 2, 3, 4, 5} and docs.count(b"") > 100
    # the property, from the canonical stream: a punctuation byte that ends its document never joins, and the same
    # pattern both joins (one token) and splits somewhere in the set
    joined = {True: 0, False: 0}
    for d, (pat, at, fk, after) in zip([x for x in docs if x and not x.endswith(b"next doc")], meta):
        cs, _ = oracle.text_canon(d, RAW)
        if after == 0 and pat[_punct_index(pat)] != ord("_"):
            assert not cs.endswith(pat[_punct_index(pat):_punct_index(pat) + 1])
        if fk == 0 and after >= len(pat) - _punct_index(pat) - 1:
            joined[pat[_punct_index(pat):_punct_index(pat) + 1] in cs or b"_" in pat] += 1
    assert joined[True] > 500 and joined[False] > 500
    g, gs = _gpu(kind, docs, RAW, k)
    o, os_ = _ref(oracle, kind, docs, RAW, k)
    assert set(np.unique(os_).tolist()) == {-1, 0}              # empty and punctuation-only documents are in the set
    assert np.array_equal(gs, os_)
    bad = np.flatnonzero((g != o).any(axis=1))
    assert bad.size == 0, f"{bad.size} records differ, first: {[docs[i][-12:] for i in bad[:6]]}"


def _raw_call(gpu_ctx, kind, blob, offs, n, mode, k):
    from ucfp_amd import _lib
    lib = _lib.load()
    rec = 8 if kind == "simhash" else 1032
    out = np.zeros((n, rec), np.uint8)
    st = np.full(n, 99, np.int32)
    if kind == "simhash":
        _lib.check(lib.ucfp_text_simhash_batch(gpu_ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode,
                                               out.ctypes.data, st.ctypes.data))
    else:
        _lib.check(lib.ucfp_text_minhash_batch(gpu_ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, k,
                                               out.ctypes.data, st.ctypes.data))
    return out, st


@pytest.mark.parametrize("kind", ["minhash", "simhash"])
def test_small_batches_and_offset_base(gpu_ctx, oracle, kind):
    """n = 1, 2, 3, 5 (partial blocks), empty documents between others, and a host call whose offsets[0] > 0: the
    bytes before offsets[0] and after offsets[n] belong to nobody."""
    docs = [b"a.", b"", b"b one two three four five six", b"", b"1,", b"2,000 x.y"]
    for n in (1, 2, 3, 5):
        _assert_exact(oracle, kind, docs[:n], RAW, 5)
        _assert_exact(oracle, kind, docs[6 - n:], RAW, 2)
    o, os_ = _ref(oracle, kind, docs, RAW, 5)
    for base in (1, 3, 64, 255):
        blob = np.frombuffer(b"z" * base + b"".join(docs) + b"z9" * 8, np.uint8).copy()
        offs = np.zeros(len(docs) + 1, np.uint64)
        offs[0] = base
        offs[1:] = base + np.cumsum([len(d) for d in docs])
        g, gs = _raw_call(gpu_ctx, kind, blob, offs, len(docs), RAW, 5)
        assert np.array_equal(gs, os_) and np.array_equal(g, o), base


# ---------------------------------------------------------------------------------------------------------------------
# 5. PRETOKENIZED: a NUL is a token byte
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,k", [("minhash", 1), ("minhash", 5), ("simhash", 1)])
def test_pretokenized_nul_is_a_token_byte(gpu_ctx, oracle, kind, k):
    """The spec (oracle): in PRETOKENIZED mode every byte other than ' ' belongs to a token, 0x00 included.  A kernel
    that takes NUL for a separator splits `ab\\0cd` in two and finds no token in a document of NULs."""
    docs = [b"ab\x00cd ef", b"\x00", b"\x00\x00 \x00", b"a \x00 b", b"one\x00 two \x00three four five six",
            b"x" * 63 + b"\x00" + b"y" * 64 + b" \x00z", b"\x00" * 300 + b" tail", b"plain tokens only"]
    for d in docs[:-1]:
        cs, nt = oracle.text_canon(d, PRETOK)
        assert b"\x00" in cs and nt == len(d.split(b" "))       # the NULs are inside the oracle's tokens
    _assert_exact(oracle, kind, docs, PRETOK, k, want_status=0)
