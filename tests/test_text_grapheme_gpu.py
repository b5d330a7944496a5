"""The grapheme tokeniser and caller-segmented tokens on the GPU: records and statuses bit-exact against
the plain-Python restatement (tests/text_grapheme_ref.py), through the C ABI (host and _dev entries) and through text.py.
Every case is a few documents of at most a few KiB; the restatement itself is checked against \\X without a GPU in
test_text_grapheme_spec.py."""
import random
import unicodedata

import numpy as np
import pytest

import text_canon_ref as canon_ref
import text_grapheme_ref as ref

pytestmark = pytest.mark.gpu

KINDS = ["minhash", "simhash"]
A, U = ref.RAW_ASCII, ref.RAW_UTF8


def _rec(kind):
    return ref.SIMHASH_BYTES if kind == "simhash" else ref.MINHASH_BYTES


def _pack(docs, lead=b""):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[0] = len(lead)
    offs[1:] = len(lead) + np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.frombuffer(lead + b"".join(docs) + b"\0" * 16, np.uint8).copy(), offs


def _gpu(ctx, kind, docs, mode, k=5, lead=b""):
    """ucfp_text_*_batch_ex(GRAPHEME) on the host entry -> (records, status)."""
    from ucfp_amd import _lib
    lib = _lib.load()
    blob, offs = _pack(docs, lead)
    n = len(docs)
    out, st = np.full((n, _rec(kind)), 0xAB, np.uint8), np.full(n, 77, np.int32)
    if kind == "simhash":
        _lib.check(lib.ucfp_text_simhash_batch_ex(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, ref.TOK_GRAPHEME,
                                                  out.ctypes.data, st.ctypes.data))
    else:
        _lib.check(lib.ucfp_text_minhash_batch_ex(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, mode, ref.TOK_GRAPHEME, k,
                                                  out.ctypes.data, st.ctypes.data))
    return out, st


def _gpu_tokens(ctx, kind, docs, k=5):
    """ucfp_text_*_tokens_batch on the host entry -> (records, status)."""
    from ucfp_amd import _lib
    lib = _lib.load()
    blob, to, dt = ref.pack_tokens(docs)
    n = len(docs)
    out, st = np.full((n, _rec(kind)), 0xAB, np.uint8), np.full(n, 77, np.int32)
    if kind == "simhash":
        _lib.check(lib.ucfp_text_simhash_tokens_batch(ctx.handle, blob.ctypes.data, to.ctypes.data, dt.ctypes.data, n,
                                                      out.ctypes.data, st.ctypes.data))
    else:
        _lib.check(lib.ucfp_text_minhash_tokens_batch(ctx.handle, blob.ctypes.data, to.ctypes.data, dt.ctypes.data, n, k,
                                                      out.ctypes.data, st.ctypes.data))
    return out, st


def _want(kind, docs, mode, k=5):
    r = [ref.grapheme_simhash(d, mode) if kind == "simhash" else ref.grapheme_minhash(d, mode, k) for d in docs]
    return np.array([np.frombuffer(b, np.uint8) for b, _ in r]).reshape(len(docs), _rec(kind)), np.array([s for _, s in r], np.int32)


def _want_tokens(kind, docs, k=5):
    r = [ref.simhash_tokens(d) if kind == "simhash" else ref.minhash_tokens(d, k) for d in docs]
    return np.array([np.frombuffer(b, np.uint8) for b, _ in r]).reshape(len(docs), _rec(kind)), np.array([s for _, s in r], np.int32)


def _check(ctx, kind, docs, mode, k=5, statuses=None):
    o, s = _gpu(ctx, kind, docs, mode, k)
    wo, ws = _want(kind, docs, mode, k)
    assert list(s) == list(ws), (kind, mode, k)
    assert np.array_equal(o, wo), (kind, mode, k, [i for i in range(len(docs)) if not np.array_equal(o[i], wo[i])])
    if statuses is not None:
        assert list(s) == list(statuses), (kind, mode, k)


def _ascii(rng, n):
    return bytes(rng.choice(b"abcdefgh ijkLMNOP.,;\t\x00'_0123456789\r\n") for _ in range(n))


def _utf8(rng, n_bytes):
    """Covered text of exactly n_bytes bytes: Latin with diacritics, Han, kana, full-width forms, ligatures, a 4-byte letter."""
    pool = "abc XYZ.\r\n\u00e9\u00df\u00c5\u0416\u03a3\u05d0\u65e5\u672c\u30ab\u304c\uff21\ufb03\u2163\u00ad\U00010400\U00010428"
    out = b""
    while len(out) < n_bytes:
        ch = rng.choice(pool).encode("utf-8")
        if len(out) + len(ch) <= n_bytes:
            out += ch
    return out


@pytest.mark.parametrize("kind,k", [("minhash", 1), ("minhash", 2), ("minhash", 5), ("minhash", 64), ("simhash", 5)])
def test_cluster_counts_around_k(gpu_ctx, kind, k):
    """Documents of 0, 1, k - 1, k and k + 1 clusters (SimHash has no k: one series)."""
    rng = random.Random(k)
    counts = sorted({0, 1, max(k - 1, 0), k, k + 1})
    docs_a = [_ascii(rng, c).replace(b"\r", b"x").replace(b"\n", b"y") for c in counts]
    assert [len(ref.device_clusters(d, A)) for d in docs_a] == counts
    _check(gpu_ctx, kind, docs_a, A, k, [-1] + [0] * (len(counts) - 1))
    docs_u = ["".join(rng.choice("\u00e9\u65e5\u30ab\u0416a\U00010428") for _ in range(c)).encode("utf-8") for c in counts]
    assert [len(ref.device_clusters(d, U)) for d in docs_u] == counts
    _check(gpu_ctx, kind, docs_u, U, k, [-1] + [0] * (len(counts) - 1))


@pytest.mark.parametrize("kind", KINDS)
def test_lengths_around_the_step_the_chunk_and_the_batch(gpu_ctx, kind):
    rng = random.Random(11)
    lens = [63, 64, 65, 255, 256, 257, 600]          # 600 crosses the 256-token batch and its flush
    for k in (1, 5, 64):
        _check(gpu_ctx, kind, [_ascii(rng, n) for n in lens], A, k, [0] * len(lens))
        _check(gpu_ctx, kind, [_utf8(rng, n) for n in lens], U, k, [0] * len(lens))
        if kind == "simhash":
            break


@pytest.mark.parametrize("kind", KINDS)
def test_cr_lf_across_a_step_and_a_chunk(gpu_ctx, kind):
    docs = []
    for at in (63, 255):
        docs.append(b"a" * at + b"\r\n" + b"b" * 10)             # CR at `at`, LF at `at` + 1: one cluster across the step
        docs.append(b"a" * (at - 1) + b"\r\n" + b"b" * 10)       # the pair inside the step
        docs.append(b"a" * at + b"\r" + b"b" * 10)
        docs.append(b"a" * (at + 1) + b"\n" + b"b" * 10)
        docs.append(b"a" * at + b"\n\r" + b"b" * 10)             # LF CR: two clusters
        docs.append(b"a" * at + b"\r\r\n\n")
    docs += [b"\r", b"\n", b"\n\r", b"\r\n", b"\r\n\r\n", b"\r\r", b"x\ry", b"x\ny"]
    n_pairs = [len(d) - len(ref.device_clusters(d, A)) for d in docs]
    assert n_pairs[:6] == [1, 1, 0, 0, 0, 1] and n_pairs[-8:] == [0, 0, 0, 1, 2, 0, 0, 0]
    for mode in (A, U):
        for k in (1, 2):
            _check(gpu_ctx, kind, docs, mode, k, [0] * len(docs))


@pytest.mark.parametrize("kind", KINDS)
def test_multibyte_sequences_across_a_step_and_a_chunk(gpu_ctx, kind):
    docs = []
    for ch in ("\u00e9", "\u65e5", "\U00010428", "\uff21"):       # 2, 3, 4 bytes; full-width A: 3 bytes -> 1
        b = ch.encode("utf-8")
        for edge in (64, 256):
            for cut in range(1, len(b)):                          # `cut` bytes of the sequence before the edge
                docs.append(b"a" * (edge - cut) + b + b"\r\nz" * 3)
    _check(gpu_ctx, kind, docs, U, 2, [0] * len(docs))
    _check(gpu_ctx, kind, docs, U, 5, [0] * len(docs))


@pytest.mark.parametrize("kind", KINDS)
def test_expansions_deletions_and_mode_equality(gpu_ctx, kind):
    six = next(cp for cp in range(0x20000) if ref.covered(cp) and len(canon_ref.lookup(cp)[0]) == 6)     # a 1 -> 6 expansion
    docs = [chr(six).encode(), ("x" * 62 + chr(six) * 3 + "y").encode(), (chr(six) * 40).encode(),
            "\ufb03\u2163\u00bd".encode(), ("a\u00adb\u200bc" * 30).encode()]
    assert len(ref.device_clusters(docs[0], U)) == 6
    _check(gpu_ctx, kind, docs, U, 5, [0] * len(docs))
    _check(gpu_ctx, kind, docs, U, 1, [0] * len(docs))
    # only Cf: nothing is left, no token
    _check(gpu_ctx, kind, ["\u00ad\u200b\u200d\u2060".encode(), b"", "\u00ad".encode() * 100], U, 5, [-1, -1, -1])
    # an ASCII document gives the same record in both modes
    rng = random.Random(3)
    asc = [_ascii(rng, n) for n in (1, 7, 64, 300, 1000)] + [b"Hello, World!\r\n_'s"]
    oa, sa = _gpu(gpu_ctx, kind, asc, A)
    ou, su = _gpu(gpu_ctx, kind, asc, U)
    assert np.array_equal(oa, ou) and list(sa) == list(su) == [0] * len(asc)
    _check(gpu_ctx, kind, asc, A)


@pytest.mark.parametrize("kind", KINDS)
def test_every_hand_back(gpu_ctx, kind):
    bad = ["e\u0301", "\u1100", "\u1176", "\u11c3", "\u0d4e", "\U0001F1E6\U0001F1E7"]
    docs = [("ok " * 30 + b + " ok").encode("utf-8") for b in bad]
    docs += [b"ok \xc0\xaf ok", b"ok \xe0\x80\xaf", b"x" * 70 + b"\xe6\x97", b"\xf0\x9f\x87", b"a\xbfb"]
    docs += [b"fine", "\ud55c\uae00 fine".encode("utf-8")]         # Hangul syllables (LV, LVT) are covered
    o, s = _gpu(gpu_ctx, kind, docs, U)
    assert list(s) == [1] * (len(docs) - 2) + [0, 0]
    assert not o[:-2].any()
    _check(gpu_ctx, kind, docs, U)
    # RAW_ASCII: a byte >= 0x80 anywhere
    docs = [b"a" * 300 + b"\x80", b"\xc3\xa9", b"plain", b"a" * 63 + b"\xff" + b"a" * 10]
    _check(gpu_ctx, kind, docs, A, 5, [1, 1, 0, 1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 4, 5, 300])
def test_ragged_batches(gpu_ctx, kind, n):
    rng = random.Random(n)
    docs = [_ascii(rng, rng.choice([0, 1, 5, 40, 64, 130, 257])) for _ in range(n)]
    o, s = _gpu(gpu_ctx, kind, docs, A, 5, lead=b"xyz")           # offsets that do not start at 0
    wo, ws = _want(kind, docs, A, 5)
    assert list(s) == list(ws) and np.array_equal(o, wo)
    docs = [_utf8(rng, rng.choice([0, 2, 9, 64, 130, 257])) for _ in range(n)]
    if n > 4:
        docs[3] = b"\xffbad"
    o, s = _gpu(gpu_ctx, kind, docs, U, 5, lead=b"\xe6")
    wo, ws = _want(kind, docs, U, 5)
    assert list(s) == list(ws) and np.array_equal(o, wo)


@pytest.mark.parametrize("kind", KINDS)
def test_token_form(gpu_ctx, kind):
    rng = random.Random(5)
    word = lambda: bytes(rng.choice(b"abcdefg\xc3\xa9\x00") for _ in range(rng.randint(1, 12)))   # noqa: E731
    docs = [
        [b"a b", b"c", b" ", b"\x00", b"\x00 \x00", b"  "],                       # spaces and NULs inside tokens
        [b"", b"", b"x", b"", b"yy", b"", b""],                                   # empty tokens: start, middle, end
        [],                                                                       # zero tokens
        [b"", b""],                                                               # only empty ones
        [word() for _ in range(400)],                                             # crosses the batch
        [bytes([65 + i % 26]) for i in range(700)],                               # one byte per token
        [b"q" * 70, b"r" * 200, b"s" * 64, b"t" * 63, b"u"],                      # tokens longer than a step
    ]
    for k in (1, 2, 5, 64):
        o, s = _gpu_tokens(gpu_ctx, kind, docs, k)
        wo, ws = _want_tokens(kind, docs, k)
        assert list(s) == list(ws) == [0, 0, -1, -1, 0, 0, 0], k
        assert np.array_equal(o, wo), k
        if kind == "simhash":
            break


@pytest.mark.parametrize("kind", KINDS)
def test_token_form_equals_pretokenized_and_grapheme_entries(gpu_ctx, kind):
    from ucfp_amd import text
    rng = random.Random(9)
    docs = [[bytes(rng.choice(b"abcxyz.\x00\t") for _ in range(rng.randint(1, 9))) for _ in range(n)] for n in (0, 1, 4, 5, 6, 333)]
    o, s = _gpu_tokens(gpu_ctx, kind, docs, 5)
    po, ps = text._run(kind, [b" ".join(d) for d in docs], text.PRETOKENIZED, 5, gpu_ctx)
    assert np.array_equal(o, po) and list(s) == list(ps)
    # the clusters the host cuts, handed in as tokens, give the record of the grapheme entry
    texts = ["Stra\u00dfe caf\u00e9\r\n\uff21\ufb03 \u65e5\u672c\u8a9e" * 9, "a\r\n\r\nb", "", "\u00ad"]
    go, gs = _gpu(gpu_ctx, kind, [t.encode() for t in texts], U, 5)
    to, ts = _gpu_tokens(gpu_ctx, kind, [ref.host_clusters(t) for t in texts], 5)
    assert np.array_equal(go, to) and list(gs) == list(ts) == [0, 0, -1, -1]


@pytest.mark.parametrize("kind", KINDS)
def test_window_limit(gpu_ctx, kind):
    """G8: a k-token window of 1405 canonical bytes is hashed, one of 1537 is refused (-2, zero record)."""
    k = 1 if kind == "simhash" else 5
    sizes = [281, 281, 281, 281, 281 - (k - 1)] if k == 5 else [1405]
    assert sum(sizes) + k - 1 == 1405
    fits = [bytes([97 + i]) * n for i, n in enumerate(sizes)]
    docs = [[b"lead", b"in"] + fits + [b"tail"], fits, [b"x" * 1537], [b"a", b"b" * 1533, b"c", b"d"] if k == 5 else [b"y" * 1600],
            [b"ok"] * 20]
    o, s = _gpu_tokens(gpu_ctx, kind, docs, k)
    wo, ws = _want_tokens(kind, docs, k)
    if k == 5:
        assert len(b" ".join(docs[3])) == 1539 and len(docs[3]) < k      # fewer than k tokens: the whole document is the window
    assert list(s) == [0, 0, -2, -2, 0]
    assert np.array_equal(o[[0, 1, 4]], wo[[0, 1, 4]]) and not o[[2, 3]].any()
    # the grapheme entries keep the guarantee trivially (a window of k <= 64 clusters is short); a long document still hashes
    _check(gpu_ctx, kind, [b"ab\r\n" * 1000], A, 64, [0])


def test_offset_tables_are_checked(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    blob = np.frombuffer(b"0123456789abcdefghijklmnopqrstuvwxyz" + b"\0" * 16, np.uint8).copy()
    to = np.array([0, 4, 9, 14, 12, 20, 26, 30], np.uint64)          # token 3 -> 4 decreases, inside document 1
    dt = np.array([0, 2, 5, 7], np.uint64)
    out, st = np.zeros((3, 1032), np.uint8), np.zeros(3, np.int32)
    rc = lib.ucfp_text_minhash_tokens_batch(gpu_ctx.handle, blob.ctypes.data, to.ctypes.data, dt.ctypes.data, 3, 2,
                                            out.ctypes.data, st.ctypes.data)
    assert rc == ref.E_INVALID and not out.any()
    assert lib.ucfp_text_simhash_tokens_batch(gpu_ctx.handle, blob.ctypes.data, to.ctypes.data, dt.ctypes.data, 3,
                                              out.ctypes.data, st.ctypes.data) == ref.E_INVALID
    bad_dt = np.array([0, 5, 3, 7], np.uint64)
    good_to = np.array([0, 4, 9, 12, 14, 20, 26, 30], np.uint64)
    assert lib.ucfp_text_minhash_tokens_batch(gpu_ctx.handle, blob.ctypes.data, good_to.ctypes.data, bad_dt.ctypes.data, 3, 2,
                                              out.ctypes.data, st.ctypes.data) == ref.E_INVALID

    def dev(kind, to_, dt_, k):
        d_blob = torch.from_numpy(blob).cuda()
        d_to, d_dt = torch.from_numpy(to_.view(np.int64)).cuda(), torch.from_numpy(dt_.view(np.int64)).cuda()
        d_out = torch.full((3, _rec(kind)), 0xAB, dtype=torch.uint8, device="cuda")
        d_st = torch.full((3,), 77, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream or None
        if kind == "simhash":
            _lib.check(lib.ucfp_text_simhash_tokens_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_to.data_ptr(), d_dt.data_ptr(), 3,
                                                              d_out.data_ptr(), d_st.data_ptr(), stream))
        else:
            _lib.check(lib.ucfp_text_minhash_tokens_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_to.data_ptr(), d_dt.data_ptr(), 3,
                                                              k, d_out.data_ptr(), d_st.data_ptr(), stream))
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_st.cpu().numpy()

    raw = blob.tobytes()
    for kind in KINDS:
        # a decreasing pair inside document 1: that document alone is refused
        o, s = dev(kind, to, dt, 2)
        wo, ws = _want_tokens(kind, [[raw[0:4], raw[4:9]], [], [raw[20:26], raw[26:30]]], 2)
        assert list(s) == [0, ref.E_INVALID, 0]
        assert np.array_equal(o[[0, 2]], wo[[0, 2]]) and not o[1].any()
        # a decreasing pair of document bounds: document 1 is refused, 0 and 2 own tokens 0..4 and 3..6
        o, s = dev(kind, good_to, bad_dt, 2)
        toks = [raw[good_to[i]:good_to[i + 1]] for i in range(7)]
        wo, ws = _want_tokens(kind, [toks[0:5], [], toks[3:7]], 2)
        assert list(s) == [0, ref.E_INVALID, 0]
        assert np.array_equal(o[[0, 2]], wo[[0, 2]]) and not o[1].any()


@pytest.mark.parametrize("kind", KINDS)
def test_dev_entries_on_a_side_stream_with_an_unaligned_base(gpu_ctx, torch_cuda, kind):
    from ucfp_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    rng = random.Random(21)
    side = torch.cuda.Stream()
    for mode, lead in ((A, b"x"), (U, b"\xe6\x97\xa5")):
        docs = [(_ascii if mode == A else _utf8)(rng, rng.choice([0, 3, 64, 65, 200, 257, 600])) for _ in range(37)]
        docs.append(b"bad \xff")
        n = len(docs)
        blob, offs = _pack(docs, lead)
        with torch.cuda.stream(side):
            d_blob, d_offs = torch.from_numpy(blob).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
            d_out = torch.full((n, _rec(kind)), 0xAB, dtype=torch.uint8, device="cuda")
            d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            if kind == "simhash":
                _lib.check(lib.ucfp_text_simhash_batch_ex_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode,
                                                              ref.TOK_GRAPHEME, d_out.data_ptr(), d_st.data_ptr(), side.cuda_stream))
            else:
                _lib.check(lib.ucfp_text_minhash_batch_ex_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, mode,
                                                              ref.TOK_GRAPHEME, 5, d_out.data_ptr(), d_st.data_ptr(), side.cuda_stream))
        side.synchronize()
        wo, ws = _want(kind, docs, mode, 5)
        assert list(d_st.cpu().numpy()) == list(ws) and ws[-1] == 1
        assert np.array_equal(d_out.cpu().numpy(), wo)
    # the token entries: a table that starts at token 2 and byte 5 of the blob, nothing read back
    toks = [bytes(rng.choice(b"ab \x00c") for _ in range(rng.randint(0, 9))) for _ in range(150)]
    docs = [toks[0:40], toks[40:40], toks[40:149], toks[149:150]]
    blob, to, dt = ref.pack_tokens(docs)
    blob = np.concatenate([np.frombuffer(b"JUNK!", np.uint8), blob])
    to = np.concatenate([np.array([0, 2], np.uint64), to + np.uint64(5)])
    dt = dt + np.uint64(2)
    with torch.cuda.stream(side):
        d_blob = torch.from_numpy(blob).cuda()
        d_to, d_dt = torch.from_numpy(to.view(np.int64)).cuda(), torch.from_numpy(dt.view(np.int64)).cuda()
        d_out = torch.full((4, _rec(kind)), 0xAB, dtype=torch.uint8, device="cuda")
        d_st = torch.full((4,), 77, dtype=torch.int32, device="cuda")
        if kind == "simhash":
            _lib.check(lib.ucfp_text_simhash_tokens_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_to.data_ptr(), d_dt.data_ptr(), 4,
                                                              d_out.data_ptr(), d_st.data_ptr(), side.cuda_stream))
        else:
            _lib.check(lib.ucfp_text_minhash_tokens_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_to.data_ptr(), d_dt.data_ptr(), 4,
                                                              5, d_out.data_ptr(), d_st.data_ptr(), side.cuda_stream))
    side.synchronize()
    wo, ws = _want_tokens(kind, docs, 5)
    assert list(d_st.cpu().numpy()) == list(ws) and np.array_equal(d_out.cpu().numpy(), wo)


def test_abi_edges(gpu_ctx):
    from ucfp_amd import _lib
    lib = _lib.load()
    h = gpu_ctx.handle
    doc = np.frombuffer(b"abc" + b"\0" * 16, np.uint8).copy()
    offs = np.array([0, 3], np.uint64)
    out, st = np.zeros(1032, np.uint8), np.zeros(1, np.int32)
    args = (doc.ctypes.data, offs.ctypes.data, 1)
    assert lib.ucfp_text_minhash_batch_ex(h, *args, ref.PRETOKENIZED, ref.TOK_GRAPHEME, 5, out.ctypes.data, st.ctypes.data) == -4
    assert lib.ucfp_text_simhash_batch_ex(h, *args, ref.PRETOKENIZED, ref.TOK_GRAPHEME, out.ctypes.data, st.ctypes.data) == -4
    assert lib.ucfp_text_minhash_batch_ex(h, *args, 3, ref.TOK_GRAPHEME, 5, out.ctypes.data, st.ctypes.data) == -4
    assert lib.ucfp_text_minhash_batch_ex(h, *args, 0, 2, 5, out.ctypes.data, st.ctypes.data) == -4          # no such tokeniser
    assert lib.ucfp_text_simhash_batch_ex(h, *args, 0, -1, out.ctypes.data, st.ctypes.data) == -4
    for k in (0, 65):
        assert lib.ucfp_text_minhash_batch_ex(h, *args, 0, ref.TOK_GRAPHEME, k, out.ctypes.data, st.ctypes.data) == -1
        assert lib.ucfp_text_minhash_tokens_batch(h, doc.ctypes.data, offs.ctypes.data, offs.ctypes.data, 1, k, out.ctypes.data,
                                                  st.ctypes.data) == -1
    assert lib.ucfp_text_minhash_batch_ex(h, None, None, 0, 0, ref.TOK_GRAPHEME, 5, None, None) == 0
    assert lib.ucfp_text_minhash_batch_ex_dev(h, None, None, 0, 2, ref.TOK_GRAPHEME, 5, None, None, None) == 0
    assert lib.ucfp_text_minhash_tokens_batch(h, None, None, None, 0, 5, None, None) == 0
    assert lib.ucfp_text_simhash_tokens_batch_dev(h, None, None, None, 0, None, None, None) == 0
    assert lib.ucfp_text_minhash_batch_ex(h, *args, 0, ref.TOK_GRAPHEME, 5, None, st.ctypes.data) == -4      # out is NULL
    # tokenizer = WORD is the existing entry
    from ucfp_amd import text
    for mode, d in ((0, b"The quick brown fox"), (1, b"the quick brown fox"), (2, "Stra\u00dfe caf\u00e9 na\u00efve".encode())):
        blob, o2 = _pack([d])
        assert lib.ucfp_text_minhash_batch_ex(h, blob.ctypes.data, o2.ctypes.data, 1, mode, ref.TOK_WORD, 2, out.ctypes.data,
                                              st.ctypes.data) == 0
        wo, ws = text._run("minhash", [d], mode, 2, gpu_ctx)
        assert np.array_equal(out, wo[0]) and st[0] == ws[0] == 0


def test_text_py_routes(gpu_ctx):
    from ucfp_amd import text
    from ucfp_amd.errors import UnsupportedError
    texts = ["Hello, World!\r\nSecond line.", "Stra\u00dfe caf\u00e9 \u00c5ngstr\u00f6m", "\u65e5\u672c\u8a9e\u306e\u30c6\u30ad\u30b9\u30c8",
             "\u0e01\u0e34\u0e19\u0e02\u0e49\u0e32\u0e27\u0e41\u0e25\u0e49\u0e27", "e\u0301 \u1100\u1161 \U0001F1E6\U0001F1E7", "", "\u00ad"]
    assert any(unicodedata.combining(ch) for ch in texts[3])          # Thai with combining vowels: the host route
    for k in (1, 5):
        opts = text.TextOpts(tokenizer="grapheme", k=k)
        o, s = text.minhash_batch(texts, opts, gpu_ctx)
        wo, ws = _want_tokens("minhash", [ref.host_clusters(t) for t in texts], k)
        assert list(s) == list(ws) == [0, 0, 0, 0, 0, -1, -1] and np.array_equal(o, wo)
    o, s = text.simhash_batch(texts, text.TextOpts(tokenizer="grapheme"), gpu_ctx)
    wo, ws = _want_tokens("simhash", [ref.host_clusters(t) for t in texts])
    assert list(s) == list(ws) and np.array_equal(o, wo)
    # another canonicaliser: the host canonicalises and cuts, the token entries hash
    canon = text.Canonicalizer(normalization="nfc", case_fold=False)
    o, s = text.minhash_batch(texts[:5], text.TextOpts(canonicalizer=canon, tokenizer="grapheme"), gpu_ctx)
    wo, ws = _want_tokens("minhash", [ref.host_clusters(t, canon) for t in texts[:5]])
    assert list(s) == [0] * 5 and np.array_equal(o, wo)
    assert not np.array_equal(o[0], text.minhash_batch(texts[:1], text.TextOpts(tokenizer="grapheme"), gpu_ctx)[0][0])   # no case fold
    # the public token entries, and the records around them
    o, s = text.minhash_tokens([[b"a b", b"", b"c"], []], 2, gpu_ctx)
    wo, ws = _want_tokens("minhash", [[b"a b", b"c"], []], 2)
    assert list(s) == [0, -1] and np.array_equal(o, wo)
    o, s = text.simhash_tokens([[b"a b", b"", b"c"], []], gpu_ctx)
    assert list(s) == [0, -1] and o[0].tobytes() == ref.simhash_tokens([b"a b", b"c"])[0]
    opts = text.TextOpts(tokenizer="grapheme")
    r = text.fingerprint_minhash_with(texts[1], opts, 1, 2)
    assert r.fingerprint == ref.minhash_tokens(ref.host_clusters(texts[1]), 5)[0] and r.config_hash == text.CONFIG_HASH_UNKNOWN
    assert text.fingerprint_lsh(texts[1], opts, 1, 2).fingerprint == r.fingerprint
    assert text.fingerprint_minhash_with(texts[1], opts, 1, 2, config_hash_value=42).config_hash == 42
    want_sim = ref.simhash_tokens(ref.host_clusters(texts[2]))[0]
    assert text.fingerprint_simhash_tf(texts[2], opts, 1, 2).fingerprint == want_sim
    assert text.fingerprint_simhash_idf(texts[2], opts, None, 1, 2).fingerprint == want_sim
    for tok in ("cjk-jp", "cjk-ko"):
        with pytest.raises(UnsupportedError, match="minhash_tokens"):
            text.minhash_batch(["abc"], text.TextOpts(tokenizer=tok), gpu_ctx)
    batcher = text.TextBatcher("minhash", opts, ctx=gpu_ctx)        # the micro-batcher is not built for graphemes
    try:
        with pytest.raises(UnsupportedError):
            batcher.submit("abc")
    finally:
        batcher.close()


def test_dedup_corpus_finds_a_one_character_edit(gpu_ctx):
    from ucfp_amd import text
    rng = random.Random(77)
    texts = ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz      ") for _ in range(220)) for _ in range(40)]
    edited = texts[7][:100] + "#" + texts[7][101:]
    texts.append(edited)
    keep, labels, status = text.dedup_corpus(texts, 0.8, text.TextOpts(tokenizer="grapheme"), ctx=gpu_ctx)
    assert not status.any()
    assert labels[40] == 7 and not keep[40] and keep[:40].all() and list(labels[:40]) == list(range(40))


@pytest.mark.parametrize("kind", KINDS)
def test_dense_steps(gpu_ctx, kind):
    """Steps of more than 64 and more than 128 canonical code points (canon_whole's second and third round), at the leads
    that put a sequence across the step edge: the dense documents of text_canon_ref."""
    docs = []
    for cp in canon_ref.expanders():
        docs += [d for i, d in enumerate(canon_ref.dense_copies(cp)) if i % 64 in (0, 1, 2, 3, 61, 62, 63) and len(d) < 600]
    docs += canon_ref.dense_mixed(16) + canon_ref.dense_dots()[::12] + canon_ref.dense_open_segments(1)[::401]
    assert any(len(ref.device_clusters(d, U)) >= 129 and len(d) <= 66 for d in docs)
    _check(gpu_ctx, kind, docs, U, 5, [0] * len(docs))
    _check(gpu_ctx, kind, docs, U, 1, [0] * len(docs))
