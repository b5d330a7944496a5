"""BM25 terms on the device: every key, count, offset and status of ucfp_bm25_terms_batch(_dev) equals the
plain-Python restatement (tests/bm25_terms_ref.py), tuple for tuple, in both forms and through both entries: at the seams
of the 64-byte step and of the LDS batch, for long tokens, the rule's edges, handed-back and refused documents."""
import ctypes as C

import numpy as np
import pytest

import bm25_terms_ref as ref
from ucfp_amd import _lib

pytestmark = pytest.mark.gpu

E_INVALID = -4
VOCAB = [b"a", b"B", b"it", b"The", b"quick", b"brown", b"fox", b"x9", b"2024", b"Zebra", b"lazy", b"dogs", b"over", b"JUMPS"]
SEPS = [b" ", b"  ", b", ", b"_", b"'", b".", b":", b";", b"\n", b"-", b"\x00", b"(", b"\x7f"]


def _text(rng, nbytes, end_in_token=None):
    """nbytes of words and separators; end_in_token: True the last byte is a word byte, False a separator, None either."""
    out = bytearray()
    while len(out) < nbytes + 8:
        out += VOCAB[int(rng.integers(len(VOCAB)))] + SEPS[int(rng.integers(len(SEPS)))]
    out = out[:nbytes]
    if nbytes and end_in_token is not None:
        out[-1] = ord("k") if end_in_token else ord(" ")
    return bytes(out)


def _blob(docs):
    offs = np.zeros(len(docs) + 1, np.uint64)
    np.cumsum([len(d) for d in docs], out=offs[1:])
    return b"".join(docs), offs


def _host(ctx, blob, offs, form, tfs_null=False):
    lib = _lib.load()
    n = offs.size - 1
    cap = int(lib.ucfp_bm25_terms_max_pairs(int(offs[n]), n))
    keys, tfs = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32)
    po, st = np.full(n + 1, 99, np.uint64), np.full(max(n, 1), 99, np.int32)
    buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
    _lib.check(lib.ucfp_bm25_terms_batch(ctx.handle, C.addressof(buf), offs.ctypes.data, n, form, keys.ctypes.data,
                                         None if tfs_null else tfs.ctypes.data, cap, po.ctypes.data, st.ctypes.data))
    total = int(po[n])
    return keys[:total], (tfs[:total] if form == ref.COUNTS else tfs[:0]), po, st[:n]


def _dev(torch, ctx, blob, offs, n_bytes, form, tfs_null=False, slack=64):
    """The device entry on torch buffers; the blob tensor is `slack` bytes longer than n_bytes says."""
    lib = _lib.load()
    n = offs.size - 1
    cap = int(lib.ucfp_bm25_terms_max_pairs(n_bytes, n))
    d_blob = torch.from_numpy(np.frombuffer(blob + b"\xc3" * slack, np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    d_keys = torch.zeros(max(cap, 1), dtype=torch.int64, device="cuda")
    d_tfs = torch.zeros(max(cap, 1), dtype=torch.int32, device="cuda")
    d_po = torch.full((n + 1,), 99, dtype=torch.int64, device="cuda")
    d_st = torch.full((max(n, 1),), 99, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.ucfp_bm25_terms_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, n_bytes, form, d_keys.data_ptr(),
                                             None if tfs_null else d_tfs.data_ptr(), cap, d_po.data_ptr(), d_st.data_ptr(), None))
    torch.cuda.synchronize()
    po = d_po.cpu().numpy().view(np.uint64)
    total = int(po[n])
    keys = d_keys.cpu().numpy().view(np.uint64)[:total]
    tfs = d_tfs.cpu().numpy().view(np.uint32)
    return keys, (tfs[:total] if form == ref.COUNTS else tfs[:0]), po, d_st.cpu().numpy()[:n]


def _same(got, want, what):
    for g, w, name in zip(got, want, ("keys", "tfs", "pair_offsets", "status")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g[:8], w[:8])


def _check(torch, ctx, docs, long_ok=()):
    """Both forms through both entries against the restatement; documents listed in long_ok may be 0 or -2 (A23.4)."""
    blob, offs = _blob(docs)
    statuses = None
    for form in (ref.COUNTS, ref.SEQUENCE):
        host = _host(ctx, blob, offs, form, tfs_null=form == ref.SEQUENCE)
        if long_ok:
            assert all(int(host[3][i]) in (0, ref.E_UNSUPPORTED) for i in long_ok), host[3][list(long_ok)]
            want = ref._pack([ref.doc_terms(d, form, int(host[3][i]) if i in long_ok else ref.E_UNSUPPORTED) for i, d in enumerate(docs)], form)
        else:
            want = ref.batch(docs, form)
        _same(host, want, ("host", form))
        _same(_dev(torch, ctx, blob, offs, len(blob), form, tfs_null=form == ref.SEQUENCE), host, ("dev", form))
        if form == ref.COUNTS:                        # what upsert_dev demands: a key once per document, tf > 0
            k, t, po, _ = host
            assert (t > 0).all()
            for i in range(len(docs)):
                seg = k[int(po[i]):int(po[i + 1])]
                assert (seg[1:] > seg[:-1]).all(), i
        statuses = host[3]
    return statuses


def _seam_docs():
    rng = np.random.default_rng(64)
    docs = []
    for end in (61, 62, 63, 64, 65, 66, 127, 128, 129):          # the token's last byte stands at end - 1
        for start in (0, 1, end - 1, end - 40):
            docs.append(b"." * start + b"T" * (end - start) + b" z9 t")
            docs.append(b"." * start + b"T" * (end - start))     # ... and the document ends with it
    docs += [b"." * 10 + b"w" * 90 + b" w", b"_" * 50 + b"Q" * 150 + b"_q", b"m" * 200, b"7" * 63 + b"." + b"7" * 64]   # two, three steps
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000):
        docs += [_text(rng, n, True), _text(rng, n, False), _text(rng, n)]
    docs += [b"", b"k", b" ", b"k" * 64, b" " * 64, b"k " * 32, b" k" * 32, b"k " * 33]
    # every seam document begins at an odd byte offset
    out, at = [], 0
    for d in docs:
        if at % 2 == 0:
            out.append(b";")
            at += 1
        out.append(d)
        at += len(d)
    return out


def test_step_and_batch_seams(gpu_ctx, torch_cuda):
    docs = _seam_docs()
    _, offs = _blob(docs)
    assert all(int(offs[i]) % 2 == 1 for i, d in enumerate(docs) if d != b";")
    st = _check(torch_cuda, gpu_ctx, docs)
    assert not st.any()


def test_lds_flush_seams(gpu_ctx, torch_cuda):
    letters = [bytes([97 + i % 26]) for i in range(300)]
    many = b" ".join(letters)                                        # 300 one-letter tokens: past the 256-token batch
    big = b"w" * 200
    wide = b",".join([big, b"X" * 300, big, b"y" * 400, big.upper(), b"z" * 500, b"w" * 199, big])   # past 1536 bytes, 8 tokens
    distinct = b" ".join(b"t%d" % i for i in range(5000))            # ~5 000 distinct terms
    docs = [b"pre fix", many, b"a", wide, distinct, many + b" " + many, b"post"]
    st = _check(torch_cuda, gpu_ctx, docs)
    assert not st.any()
    k, t, po, _ = _host(gpu_ctx, *_blob(docs), ref.COUNTS)
    assert int(po[2] - po[1]) == 26 and int(t[int(po[1]):int(po[2])].sum()) == 300     # a term across a flush is one pair
    seg = slice(int(po[3]), int(po[4]))
    assert int(t[seg][list(k[seg]).index(ref.key(big))]) == 4
    assert int(po[5] - po[4]) == 5000


def test_long_tokens(gpu_ctx, torch_cuda):
    limit = ref.MAX_WINDOW_BYTES
    docs = [b"left neighbour", b"a " + b"L" * limit + b" b", b"x" * limit, b"mid", b"q " + b"r" * 2000 + b" s a", b"r" * 2000,
            b"right neighbour", b"e" * (limit + 1) + b"\xc3\xa9"]
    st = _check(torch_cuda, gpu_ctx, docs, long_ok=(4, 5))
    assert list(st[:4]) == [0, 0, 0, 0] and st[6] == 0 and st[7] == ref.NEEDS_HOST
    k, _, po, _ = _host(gpu_ctx, *_blob(docs), ref.SEQUENCE)
    assert int(k[int(po[2])]) == ref.key(b"x" * limit)


def test_rule_edges(gpu_ctx, torch_cuda):
    docs = [b"a_b", b"it's", b"3.14", b"A1b2", b" \t\n_'.:,;-", b"Fox fox FOX fOx", b"", b"_", b"9", b"a:b,c;d", b"\x00a\x00"]
    _check(torch_cuda, gpu_ctx, docs)
    k, t, po, st = _host(gpu_ctx, *_blob(docs), ref.COUNTS)
    assert not st.any()
    doc = lambda i: dict(zip(k[int(po[i]):int(po[i + 1])].tolist(), t[int(po[i]):int(po[i + 1])].tolist()))
    assert doc(0) == {ref.key(b"a"): 1, ref.key(b"b"): 1}
    assert doc(1) == {ref.key(b"it"): 1, ref.key(b"s"): 1}
    assert doc(2) == {ref.key(b"3"): 1, ref.key(b"14"): 1}
    assert doc(3) == {ref.key(b"a1b2"): 1}
    assert doc(4) == {} and doc(6) == {} and doc(7) == {}
    assert doc(5) == {ref.key(b"fox"): 4}


def test_hand_back(gpu_ctx, torch_cuda):
    rng = np.random.default_rng(80)
    hi = b"\xe9"
    docs = [_text(rng, 100), hi + _text(rng, 99), _text(rng, 70), _text(rng, 99) + hi, _text(rng, 63) + hi + _text(rng, 40),
            _text(rng, 64) + hi + _text(rng, 40), _text(rng, 255) + hi, _text(rng, 256) + hi + b"a", hi, _text(rng, 300),
            "naïve Σίσυφος 漢字".encode("utf-8")]
    st = _check(torch_cuda, gpu_ctx, docs)
    assert list(st) == [0, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1]


def test_invalid_offsets(gpu_ctx, torch_cuda):
    rng = np.random.default_rng(81)
    blob = _text(rng, 400)
    cases = [([0, 50, 40, 120, 130, 400], 400),       # a decreasing offset: documents 1 and 2 (it would share bytes with 0)
             ([0, 50, 120, 130, 405], 400),           # the last offset passes n_bytes
             ([0, 50, 120, 130, 400], 399),           # ... by one byte
             ([7, 7, 3, 3, 200, 100, 250, 400], 400),
             ([0, 1 << 40, 100, 400], 400)]
    for offs, n_bytes in cases:
        offs = np.array(offs, np.uint64)
        for form in (ref.COUNTS, ref.SEQUENCE):
            want = ref.batch_offsets(blob, offs, n_bytes, form)
            _same(_dev(torch_cuda, gpu_ctx, blob[:n_bytes], offs, n_bytes, form), want, (offs, form))
    st = ref.batch_offsets(blob, np.array(cases[0][0], np.uint64), 400, 0)[3]
    assert list(st) == [0, E_INVALID, E_INVALID, 0, 0]
    assert list(ref.batch_offsets(blob, np.array(cases[1][0], np.uint64), 400, 0)[3]) == [0, 0, 0, E_INVALID]
    # the host form takes n_bytes = offsets[n]
    offs = np.array([0, 50, 40, 120, 400], np.uint64)
    _same(_host(gpu_ctx, blob, offs, ref.COUNTS), ref.batch_offsets(blob, offs, 400, ref.COUNTS), "host")


def test_size_limits(gpu_ctx, torch_cuda):
    lib = _lib.load()
    for form in (ref.COUNTS, ref.SEQUENCE):
        for docs in ([], [b"one Two two"], [b""]):
            _same(_host(gpu_ctx, *_blob(docs), form), ref.batch(docs, form), (docs, form))
            blob, offs = _blob(docs)
            _same(_dev(torch_cuda, gpu_ctx, blob, offs, len(blob), form), ref.batch(docs, form), (docs, form))
    blob, offs = _blob([b"a b c", b"d e"])
    cap = int(lib.ucfp_bm25_terms_max_pairs(len(blob), 2))
    assert cap == 5
    keys, tfs, po, st = np.full(cap, 7, np.uint64), np.full(cap, 7, np.uint32), np.full(3, 7, np.uint64), np.full(2, 7, np.int32)
    buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
    rc = lib.ucfp_bm25_terms_batch(gpu_ctx.handle, C.addressof(buf), offs.ctypes.data, 2, 0, keys.ctypes.data, tfs.ctypes.data, cap - 1,
                                   po.ctypes.data, st.ctypes.data)
    assert rc == E_INVALID
    assert (keys == 7).all() and (tfs == 7).all() and (po == 7).all() and (st == 7).all()
    rc = lib.ucfp_bm25_terms_batch(gpu_ctx.handle, C.addressof(buf), offs.ctypes.data, 2, 0, keys.ctypes.data, tfs.ctypes.data, cap,
                                   po.ctypes.data, st.ctypes.data)
    assert rc == 0 and int(po[2]) == 5                # the bound is met exactly


def test_many_documents_and_scratch_reuse(gpu_ctx, torch_cuda):
    """More than one block and one compaction tile; then a small batch after a large one in the same scratch."""
    rng = np.random.default_rng(82)
    docs = [_text(rng, int(rng.integers(0, 200))) for _ in range(1500)]
    _check(torch_cuda, gpu_ctx, docs)
    _check(torch_cuda, gpu_ctx, docs[:3])


def test_terms_batch_fills_the_host_route(gpu_ctx):
    from ucfp_amd import terms
    texts = ["The quick brown fox", "naïve Σίσυφος ΣΊΣΥΦΟΣ 漢字 x", "", "fox FOX " + "r" * 2000 + " tail", "İstanbul a_b it's", "plain again"]
    for form, f in (("counts", ref.COUNTS), ("sequence", ref.SEQUENCE)):
        keys, tfs, po, st = terms.terms_batch(texts, form, gpu_ctx)
        assert list(st[:3]) == [0, 1, 0] and st[3] in (0, -2) and list(st[4:]) == [1, 0]
        for i, t in enumerate(texts):
            toks = [ref.key(w.encode("utf-8")) for w in terms.tokenize(t)]
            got = keys[int(po[i]):int(po[i + 1])].tolist()
            if f == ref.SEQUENCE:
                assert got == toks, i
            else:
                want = sorted(set(toks))
                assert got == want and tfs[int(po[i]):int(po[i + 1])].tolist() == [toks.count(k) for k in want], i
        assert int(po[0]) == 0 and int(po[-1]) == keys.size and (tfs.size == keys.size) == (f == ref.COUNTS)
