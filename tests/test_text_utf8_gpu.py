"""GPU: text mode RAW_UTF8 (canonicalise + tokenise on the device) against the table-driven restatement
tests/text_canon_ref.py -- token blobs byte for byte, statuses equal (the kernel hands back exactly what the spec
does), records equal to the PRETOKENIZED hash of the restatement's tokens."""
import ctypes as C
import random

import numpy as np
import pytest

import text_canon_ref as ref

pytestmark = pytest.mark.gpu

KINDS = [("minhash", 1), ("minhash", 5), ("simhash", 1)]


def _expect(kind, docs, k):
    """Restatement tokens -> the library's own PRETOKENIZED hash; NEEDS_HOST wins with a zero record."""
    from ucfp_amd import text
    toks, st = zip(*[ref.canon_bytes(d) for d in docs])
    st = np.array(st, np.int32)
    rec, hs = text._run(kind, list(toks), text.PRETOKENIZED, k)
    rec[st == ref.NEEDS_HOST] = 0
    return rec, np.where(st == ref.NEEDS_HOST, ref.NEEDS_HOST, hs).astype(np.int32)


def _check(docs, kinds=KINDS):
    from ucfp_amd import text
    want = [ref.canon_bytes(d) for d in docs]
    toks, st = text.canon_batch(docs)
    assert list(st) == [s for _, s in want]
    bad = [i for i in range(len(docs)) if toks[i] != want[i][0]]
    assert not bad, (bad[:5], docs[bad[0]], toks[bad[0]], want[bad[0]][0])
    for kind, k in kinds:
        g, gs = text._run(kind, docs, text.RAW_UTF8, k)
        o, os_ = _expect(kind, docs, k)
        assert np.array_equal(gs, os_), (kind, k, np.flatnonzero(gs != os_)[:5])
        diff = [i for i in range(len(docs)) if not np.array_equal(g[i], o[i])]
        assert not diff, (kind, k, diff[:5])
    return st


def test_random_documents():
    rng = random.Random(2)
    docs = [ref.random_string(rng, 1, 400).encode("utf-8") for _ in range(512)]
    st = _check(docs)
    assert not st.any()          # the generator draws covered code points only


def test_phase_sweep_over_step_and_chunk_edges():
    """Every split of sequence and context across the 64-byte step and the 256-byte chunk of the hash pass."""
    six = next(chr(cp) for cp in range(0x3300, 0x3400) if ref.lookup(cp) and len(ref.lookup(cp)[0]) == 6)
    seqs = ["\u00e9", "\u65e5", "\U0001d400", six, "a\u200d:\u200db", "a\u2019e", "'e", "a.b", "\u05d0\"\u05d1"]
    assert len(seqs[2].encode()) == 4 and ref.lookup(0x1D400) == ((0x61,), 1 | 16 | 32)
    docs = []
    for off in list(range(58, 67)) + list(range(250, 259)):
        for s in seqs:
            docs.append(b"x" * off + s.encode("utf-8") + b" tail")
            docs.append((b"ab " * 100)[:off] + s.encode("utf-8"))
    assert len(docs) <= 512
    st = _check(docs)
    assert not st.any()


def test_adjacent_tokens():
    docs = ["\u65e5\u672c\u8a9e\u30ab\u30bf\u30ab\u30caabc".encode(), ("\u6f22" * 300).encode(),
            ("\u6f22\u5b57" * 150 + "x").encode()]
    assert ref.canon_bytes(docs[0])[0].decode() == "\u65e5 \u672c \u8a9e \u30ab\u30bf\u30ab\u30ca abc"
    assert ref.canon_bytes(docs[1])[0].count(b" ") == 299      # 300 tokens, more than one 256-token batch of the hash pass
    _check(docs)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_late_tokens(n):
    from ucfp_amd import text
    docs = [b"_" * n + b"a", b"_" * n + b" ", b"x " + b"_" * n + b" y", b"x " + b"_" * n + b"\xc3\xa9 y"]
    assert ref.canon_bytes(docs[0]) == (docs[0], 0) and ref.canon_bytes(docs[1]) == (b"", 0)
    _check(docs)
    _, st = text._run("minhash", docs, text.RAW_UTF8, 5)
    assert list(st) == [0, -1, 0, 0]


def test_hand_backs_leave_their_neighbours_alone():
    rng = random.Random(3)
    poison = ["\u0301", "\u1161", "\U0001f1e6", "\u0130", "\ufdfa", "\U000e0001", "\U00020000"]
    broken = [b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"\xe6\x97", b"\xff"]
    docs, handed = [], []
    for i in range(192):
        s = ref.random_string(rng, 20, 300)
        d = s.encode("utf-8")
        if i % 3 == 1:
            at = rng.randint(0, len(s))
            p = rng.choice(poison + broken)
            d = s[:at].encode("utf-8") + (p.encode("utf-8") if isinstance(p, str) else p) + s[at:].encode("utf-8")
            handed.append(i)
        docs.append(d)
    docs.append(b"cut at the end \xe6\x97")
    handed.append(192)
    st = _check(docs)
    assert list(np.flatnonzero(st == ref.NEEDS_HOST)) == handed


def test_ascii_without_underscore_and_apostrophe_equals_mode_0():
    from ucfp_amd import text
    rng = random.Random(4)
    alphabet = [chr(c) for c in list(range(32, 127)) + [9, 10, 13] if chr(c) not in "_'"] + list("   eeaatt..,,::")
    docs = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 700))).encode() for _ in range(128)]
    for kind, k in KINDS:
        a, as_ = text._run(kind, docs, text.RAW_ASCII, k)
        b, bs = text._run(kind, docs, text.RAW_UTF8, k)
        assert np.array_equal(as_, bs) and np.array_equal(a, b), (kind, k)
    _check(docs, kinds=[])
    # and the documented difference (U6)
    a, _ = text._run("minhash", [b"x 'e", b"a_b c"], text.RAW_ASCII, 5)
    b, _ = text._run("minhash", [b"x 'e", b"a_b c"], text.RAW_UTF8, 5)
    assert not np.array_equal(a[0], b[0])
    assert text.canon_batch([b"x 'e", b"__ a_b _c"])[0] == [b"x 'e", b"a_b _c"]


def test_limits():
    from ucfp_amd import text
    w = text.MAX_WINDOW_BYTES
    docs = [("\u00c9" * (w // 2) + "a").encode(),        # one token of exactly MAX_WINDOW_BYTES canonical bytes
            ("\u00e9" * 800).encode(),                   # 1600 bytes: more than an LDS batch holds
            b"", "\u200b\u200d\u00ad".encode(), b" \n "]
    assert len(ref.canon_bytes(docs[0])[0]) == w and len(ref.canon_bytes(docs[1])[0]) == 1600
    _check(docs)
    for kind in ("minhash", "simhash"):
        _, st = text._run(kind, docs, text.RAW_UTF8, 5)
        assert list(st) == [0, -2, -1, -1, -1], kind


def test_device_entry_points_with_an_offset_base(gpu_ctx, torch_cuda):
    """The _dev calls: offsets that do not start at 0, results left on the device, one stream."""
    from ucfp_amd import _lib, text
    torch = torch_cuda
    lib = _lib.load()
    rng = random.Random(6)
    docs = [ref.random_string(rng, 1, 200).encode("utf-8") for _ in range(37)] + [b"bad \xff"]
    n = len(docs)
    lead = b"\xe6\x97\xa5junk"
    blob = np.frombuffer(lead + b"".join(docs) + b"\0" * 16, np.uint8)
    offs = np.zeros(n + 1, np.int64)
    offs[0] = len(lead)
    offs[1:] = len(lead) + np.cumsum([len(d) for d in docs])
    d_blob, d_offs = torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(offs).cuda()
    total = int(offs[n] - offs[0])
    d_tok = torch.zeros(lib.ucfp_text_canon_bound(total) + 64, dtype=torch.uint8, device="cuda")
    d_toff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream or None
    _lib.check(lib.ucfp_text_canon_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, d_tok.data_ptr(),
                                             d_toff.data_ptr(), d_st.data_ptr(), stream))
    d_rec = torch.zeros((n, text.MINHASH_BYTES), dtype=torch.uint8, device="cuda")
    d_hst = torch.zeros(n, dtype=torch.int32, device="cuda")
    _lib.check(lib.ucfp_text_minhash_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, text.RAW_UTF8, 5,
                                               d_rec.data_ptr(), d_hst.data_ptr(), stream))
    torch.cuda.synchronize()
    toff, tok = d_toff.cpu().numpy(), d_tok.cpu().numpy()
    want = [ref.canon_bytes(d) for d in docs]
    assert toff[0] == 0 and list(d_st.cpu().numpy()) == [s for _, s in want] and want[-1][1] == ref.NEEDS_HOST
    assert [tok[toff[i]:toff[i + 1]].tobytes() for i in range(n)] == [t for t, _ in want]
    o, os_ = _expect("minhash", docs, 5)
    assert np.array_equal(d_hst.cpu().numpy(), os_) and np.array_equal(d_rec.cpu().numpy(), o)


def test_abi_edges(gpu_ctx):
    from ucfp_amd import _lib, text
    lib = _lib.load()
    assert lib.ucfp_text_canon_bound(0) == 0 and lib.ucfp_text_canon_bound(10) == 40
    assert lib.ucfp_text_canon_bound(2**64 - 1) == 2**64 - 1
    toff = (C.c_uint64 * 1)(7)
    assert lib.ucfp_text_canon_batch(gpu_ctx.handle, None, None, 0, None, 0, toff, None) == 0 and toff[0] == 0
    assert lib.ucfp_text_canon_batch_dev(gpu_ctx.handle, None, None, 0, None, None, None, None) == 0
    assert lib.ucfp_text_minhash_batch(gpu_ctx.handle, None, None, 0, text.RAW_UTF8, 5, None, None) == 0
    assert lib.ucfp_text_simhash_batch(gpu_ctx.handle, None, None, 0, text.RAW_UTF8, None, None) == 0
    assert lib.ucfp_text_minhash_batch_dev(gpu_ctx.handle, None, None, 0, text.RAW_UTF8, 5, None, None, None) == 0
    assert lib.ucfp_text_canon_batch(None, None, None, 0, None, 0, None, None) == -4
    assert lib.ucfp_text_minhash_batch(gpu_ctx.handle, None, None, 0, 3, 5, None, None) == -4        # no such mode
    h = C.c_void_p()
    assert lib.ucfp_text_batcher_create(gpu_ctx.handle, text.ALGO_MINHASH, 3, 5, 16, 1 << 16, 100, C.byref(h)) == -4
    # a token buffer smaller than the blob is refused, nothing is cut
    doc = "\u65e5\u672c\u8a9e".encode()
    offs = (C.c_uint64 * 2)(0, len(doc))
    toff2, st, small = (C.c_uint64 * 2)(), (C.c_int32 * 1)(), (C.c_uint8 * 4)()
    assert lib.ucfp_text_canon_batch(gpu_ctx.handle, doc, offs, 1, small, 4, toff2, st) == -4
    assert text.canon_batch([doc])[0] == ["\u65e5 \u672c \u8a9e".encode()]
    assert text.canon_batch([])[0] == []


def _mixed():
    return ["plain ascii goes raw, with don't and foo_bar", "Caf\u00e9 au lait, na\u00efve fa\u00e7ade \u2014 STRASSE stra\u00dfe \ufb01ne",
            "\u4f60\u597d \u4e16\u754c hello world 123", "l\u2019\u00e9t\u00e9 \u00e0 l'or\u00e9e \u05d0\"\u05d1 \uff21\uff22\uff23 \u30ab\u30bf\u30ab\u30ca",
            "cafe\u0301 noir with a combining accent", "\U0001f1eb\U0001f1f7 france", "\u1112\u1161\u11ab jamo", "", "\u200b",
            "\u0130stanbul"] + ["\u65e5\u672c\u8a9e word %d \u00e9" % i for i in range(6)]


@pytest.mark.parametrize("kind", ["minhash", "simhash"])
def test_routing_gives_the_host_path_records(gpu_ctx, oracle, kind):
    from ucfp_amd import text
    fo = oracle.text_minhash_batch if kind == "minhash" else oracle.text_simhash_batch
    for opts in (text.TextOpts(), text.TextOpts(canonicalizer=text.Canonicalizer(normalization="nfc"))):
        docs = _mixed()
        fn = text.minhash_batch if kind == "minhash" else text.simhash_batch
        recs, st = fn(docs, opts)
        for i, d in enumerate(docs):
            b, mode = text._prepare(d, opts)
            o, os_ = fo([b], mode=mode)
            assert st[i] == os_[0], (i, d)
            assert np.array_equal(recs[i], o[0]) if st[i] == 0 else not recs[i].any(), (i, d)
    assert [text._device_utf8(d, text.TextOpts()) for d in _mixed()[:5]] == [False, True, True, True, True]
    assert ref.canon_bytes(_mixed()[4].encode())[1] == ref.NEEDS_HOST and ref.canon_bytes(_mixed()[3].encode())[1] == 0


def test_batcher_routes_like_the_batch_call(gpu_ctx, oracle):
    from concurrent.futures import ThreadPoolExecutor
    from ucfp_amd import text
    docs = _mixed() * 8
    want = []
    for d in docs:
        b, mode = text._prepare(d, text.TextOpts())
        o, s = oracle.text_minhash_batch([b], mode=mode)
        want.append((o[0].tobytes(), int(s[0])))
    b = text.TextBatcher("minhash", max_batch=64, max_bytes=64 << 10, max_delay_us=1000, ctx=gpu_ctx)
    try:
        with ThreadPoolExecutor(16) as pool:
            got = list(pool.map(b.submit, docs))
        assert [s for _, s in got] == [s for _, s in want]
        assert all(g[0] == w[0] for g, w in zip(got, want) if w[1] == 0)
        assert b.stats()[1] == len(docs)
    finally:
        b.close()
