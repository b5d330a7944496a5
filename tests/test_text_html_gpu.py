"""HTML pages -> text on the GPU: ucfp_text_html_batch and ucfp_text_html_batch_dev byte for byte -- text
bytes, offsets and flags -- against the plain-Python restatement (tests/text_html_ref.py), then the stage in front of the
hash kernels on one stream, and `TextOpts(preprocess="html")` through every batch entry of ucfp_amd.text.  The shapes
are the smallest that can break the kernel: every construct across every step seam and look-ahead seam, the lengths
around one and two steps, batches around a workgroup's four waves, one long page and one long unterminated comment."""
import random

import numpy as np
import pytest

import text_html_ref as ref

pytestmark = pytest.mark.gpu


def _pack(docs, lead=b""):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    offs += np.uint64(len(lead))
    return np.frombuffer(lead + b"".join(docs) + b"\0" * 16, np.uint8).copy(), offs


def _host(ctx, docs, lead=b""):
    """ucfp_text_html_batch -> (texts, offsets, flags)"""
    from ucfp_amd import _lib
    lib = _lib.load()
    blob, offs = _pack(docs, lead)
    n = len(docs)
    cap = int(lib.ucfp_text_html_bound(int(offs[n] - offs[0])))
    text = np.full(cap + 8, 0xAB, np.uint8)
    toff = np.full(n + 1, 77, np.uint64)
    flags = np.full(max(n, 1), 77, np.uint32)
    _lib.check(lib.ucfp_text_html_batch(ctx.handle, blob.ctypes.data, offs.ctypes.data, n, text.ctypes.data, cap, toff.ctypes.data,
                                        flags.ctypes.data))
    assert (text[cap:] == 0xAB).all()
    return [text[int(toff[i]):int(toff[i + 1])].tobytes() for i in range(n)], toff.tolist(), flags[:n].tolist()


def _dev(torch, ctx, docs, lead=b""):
    """ucfp_text_html_batch_dev -> (texts, offsets, flags); the bytes behind the text must stay untouched"""
    from ucfp_amd import _lib
    lib = _lib.load()
    blob, offs = _pack(docs, lead)
    n = len(docs)
    cap = int(offs[n] - offs[0])
    d_blob = torch.from_numpy(blob).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    d_text = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    d_toff = torch.full((n + 1,), 77, dtype=torch.int64, device="cuda")
    d_flags = torch.full((max(n, 1),), 77, dtype=torch.int32, device="cuda")
    _lib.check(lib.ucfp_text_html_batch_dev(ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, d_text.data_ptr(), d_toff.data_ptr(),
                                            d_flags.data_ptr(), torch.cuda.current_stream().cuda_stream or None))
    torch.cuda.synchronize()
    text, toff, flags = d_text.cpu().numpy(), d_toff.cpu().numpy().view(np.uint64), d_flags.cpu().numpy().view(np.uint32)
    assert (text[int(toff[n]):] == 0xAB).all(), "a store past the text the count pass sized"
    return [text[int(toff[i]):int(toff[i + 1])].tobytes() for i in range(n)], toff.tolist(), flags[:n].tolist()


def _check(got, docs, what=""):
    texts, offs, flags = ref.html_to_text_batch(docs)
    g_texts, g_offs, g_flags = got
    assert g_offs == offs, what
    bad = [i for i in range(len(docs)) if g_texts[i] != texts[i] or g_flags[i] != flags[i]]
    assert not bad, (what, len(bad), [(docs[i], g_texts[i], texts[i], g_flags[i], flags[i]) for i in bad[:3]])


def test_vector_table_through_both_entries(gpu_ctx, torch_cuda):
    docs = [v[0] for v in ref.VECTORS]
    for got in (_host(gpu_ctx, docs), _dev(torch_cuda, gpu_ctx, docs)):
        _check(got, docs)
        assert got[0] == [v[1] for v in ref.VECTORS] and got[2] == [v[2] for v in ref.VECTORS]


SEAM_CONSTRUCTS = [
    b"&thetasym;", b"&lt;", b"&#x10FFFF;", b"&#9999999;", b"&nbsp;", b"&amp", b"&bogus;",
    b"<!--x-->", b"<!---->", b"<!-->x-->", b"<!DOCTYPE html>", b"<?x?>",
    b"<script>q</script >", b"<style>q</STYLE>", b"<script>a<b</scripty></script>",
    b'<p class="a>b">', b"<a href='x'>", b"<p title=it's>", b"<br/>", b"</strong>", b"<strongx>", b"<1",
    b" \t\n\r\f", "漢".encode(), "😀".encode(),
    b"<b\0>", b"<style>q</style\0>r</style>", b"&lt\0;", b"&thetasy\0;", b"\0",
]


def test_every_construct_across_every_step_seam(gpu_ctx):
    """`a` * s + construct + ` z` for s = 0 .. 75: every byte of every construct meets the end of a 64-byte step and the
    end of the 9-byte look-ahead behind it.  One batch."""
    docs = [b"a" * s + c + b" z" for c in SEAM_CONSTRUCTS for s in range(76)]
    assert len(SEAM_CONSTRUCTS) >= 20 and len(docs) >= 1500
    _check(_host(gpu_ctx, docs), docs)


def test_document_lengths_around_the_step(gpu_ctx):
    rng = random.Random(5)
    for fill in (b"a", b"<", b" ", b"&"):
        docs = [fill * n for n in (0, 1, 63, 64, 65, 127, 128, 129)]
        _check(_host(gpu_ctx, docs), docs, fill)
    page = ref.gen_page(rng, blocks=3).encode()
    docs = [page[:n] for n in (0, 1, 63, 64, 65, 127, 128, 129)]
    _check(_host(gpu_ctx, docs), docs)


@pytest.mark.parametrize("n", [0, 1, 4, 5])
def test_batch_sizes_around_a_workgroup(gpu_ctx, torch_cuda, n):
    rng = random.Random(n)
    docs = [ref.gen_page(rng, blocks=2).encode() for _ in range(n)]
    _check(_host(gpu_ctx, docs), docs)
    _check(_dev(torch_cuda, gpu_ctx, docs), docs)      # n = 0 still writes text_offsets[0] = 0


def test_nonzero_first_offset(gpu_ctx, torch_cuda):
    rng = random.Random(9)
    docs = [ref.gen_page(rng, blocks=2).encode() for _ in range(3)] + [b"<b>x</b> y"]
    lead = b"<p>not a document <!--"
    _check(_host(gpu_ctx, docs, lead), docs)
    _check(_dev(torch_cuda, gpu_ctx, docs, lead), docs)


def test_random_documents(gpu_ctx):
    rng = random.Random(13)
    docs = [ref.fuzz_doc(rng, 220)[:300] for _ in range(4096)]
    assert min(map(len, docs)) == 0 and max(map(len, docs)) == 300
    _check(_host(gpu_ctx, docs), docs)


def test_long_page_and_long_unterminated_comment(gpu_ctx, torch_cuda):
    rng = random.Random(17)
    page = ref.gen_page(rng, blocks=1350).encode()
    assert 150_000 < len(page) < 300_000
    comment = b"<!--" + b"a-- >b->c" * 11_400
    assert len(comment) > 100_000 and b"-->" not in comment
    docs = [page, comment, b"after"]
    got = _dev(torch_cuda, gpu_ctx, docs)
    _check(got, docs)
    assert got[0][1] == b"" and got[2][1] == ref.FLAG_OPEN_MARKUP
    assert len(got[0][0]) > 50_000


def test_bytes_that_are_not_utf8_pass_through(gpu_ctx):
    docs = [b"\xff\xfe\x80", b"<p>\xff</p>\xfe \x80", b"\xc3<b>\xa9</b>"]
    got = _host(gpu_ctx, docs)
    _check(got, docs)
    assert got[0] == [b"\xff\xfe\x80", b"\xff \xfe \x80", b"\xc3\xa9"] and got[2] == [1, 1, 1]


def test_null_flags_and_small_buffer(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib
    lib = _lib.load()
    docs = [b"<p>a</p> b", b"c"]
    blob, offs = _pack(docs)
    text, toff = np.zeros(16, np.uint8), np.zeros(3, np.uint64)
    _lib.check(lib.ucfp_text_html_batch(gpu_ctx.handle, blob.ctypes.data, offs.ctypes.data, 2, text.ctypes.data, 16, toff.ctypes.data, None))
    assert toff.tolist() == [0, 3, 4] and text[:4].tobytes() == b"a bc"
    assert lib.ucfp_text_html_batch(gpu_ctx.handle, blob.ctypes.data, offs.ctypes.data, 2, text.ctypes.data, 3, toff.ctypes.data, None) == -4
    assert lib.ucfp_text_html_batch_dev(None, None, None, 0, None, None, None, None) == -4


# ---- the stage in front of the hash kernels ----

_PROSE = ("The quick brown fox jumps over the lazy dog while seven wizards quietly mix potions near a frozen lake and nobody "
          "expects any answer before dawn breaks again over the silent northern hills").split()


def _ascii_pages(n, seed):
    rng = random.Random(seed)
    return [ref.gen_page(rng, blocks=8, words=12, utf8=False, refs=False) for _ in range(n)]


def test_device_chain_into_the_hash_kernels(gpu_ctx, torch_cuda):
    """ucfp_text_html_batch_dev, then MinHash and SimHash (RAW_ASCII) over its output on the same stream, nothing between."""
    torch = torch_cuda
    from ucfp_amd import _lib, text
    lib = _lib.load()
    pages = [p.encode() for p in _ascii_pages(9, 21)]
    texts = ref.html_to_text_batch(pages)[0]
    assert all(t.isascii() and len(t) > 100 for t in texts)
    blob, offs = _pack(pages)
    n = len(pages)
    d_blob, d_offs = torch.from_numpy(blob).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    d_text = torch.zeros(int(offs[n]) + 64, dtype=torch.uint8, device="cuda")
    d_toff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_min = torch.zeros((n, text.MINHASH_BYTES), dtype=torch.uint8, device="cuda")
    d_sim = torch.zeros((n, text.SIMHASH_BYTES), dtype=torch.uint8, device="cuda")
    d_st = torch.full((2, n), 77, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream or None
    _lib.check(lib.ucfp_text_html_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, d_text.data_ptr(), d_toff.data_ptr(),
                                            None, st))
    _lib.check(lib.ucfp_text_minhash_batch_dev(gpu_ctx.handle, d_text.data_ptr(), d_toff.data_ptr(), n, text.RAW_ASCII, text.DEFAULT_K,
                                               d_min.data_ptr(), d_st[0].data_ptr(), st))
    _lib.check(lib.ucfp_text_simhash_batch_dev(gpu_ctx.handle, d_text.data_ptr(), d_toff.data_ptr(), n, text.RAW_ASCII,
                                               d_sim.data_ptr(), d_st[1].data_ptr(), st))
    torch.cuda.synchronize()
    strs = [t.decode() for t in texts]
    want_min, st_min = text.minhash_batch(strs, ctx=gpu_ctx)
    want_sim, st_sim = text.simhash_batch(strs, ctx=gpu_ctx)
    assert not st_min.any() and not st_sim.any() and not d_st.cpu().numpy().any()
    assert np.array_equal(d_min.cpu().numpy(), want_min) and np.array_equal(d_sim.cpu().numpy(), want_sim)


def _route_pages():
    """Pages whose text is ASCII, Latin through `&eacute;`-style references (the page itself is ASCII), and Han from `&#x..;`
    references and literal UTF-8."""
    body = " ".join(_PROSE)
    ascii_page = ("<!DOCTYPE html><html><head><title>Fox</title><style>p > a { color: red }</style></head><body><h1>Fox &amp; dog</h1>"
                  "<p class=\"a>b\">%s <b>bo</b>ld 1 &lt; 2</p><script>if (a < b) x = '</p>';</script><!-- c > d --></body></html>" % body)
    latin = ("<div><p>Le caf&eacute; na&iuml;f du r&eacute;sum&eacute; &agrave; Z&uuml;rich: <em>%s</em></p><br/>"
             "<p>Stra&szlig;e &Eacute;cole &#233;t&#xE9; d&eacute;j&agrave; vu</p></div>" % body)
    han = ("<p>&#x6F22;&#x5B57; 漢字 <span>日本語</span>のテキスト %s</p><ul><li>中文 &#20013;&#25991;</li><li>文字 列</li></ul>" % body)
    return [ascii_page, latin, han, _ascii_pages(1, 33)[0]]


@pytest.fixture(scope="module")
def routes():
    pages = _route_pages()
    want = [t.decode("utf-8") for t in ref.html_to_text_batch([p.encode("utf-8") for p in pages])[0]]
    assert want[0].isascii() and pages[1].isascii() and not want[1].isascii() and "漢字 漢字" in want[2]
    return pages, want


@pytest.mark.parametrize("tokenizer,h", [("word", 128), ("grapheme", 128), ("word", 64), ("grapheme", 64)])
def test_routes_minhash(gpu_ctx, routes, tokenizer, h):
    from ucfp_amd import text
    pages, want = routes
    got = text.minhash_batch(pages, text.TextOpts(tokenizer=tokenizer, h=h, preprocess="html"), ctx=gpu_ctx)
    exp = text.minhash_batch(want, text.TextOpts(tokenizer=tokenizer, h=h), ctx=gpu_ctx)
    assert not exp[1].any() and np.array_equal(got[1], exp[1]) and np.array_equal(got[0], exp[0])
    raw = text.minhash_batch(pages, text.TextOpts(tokenizer=tokenizer, h=h), ctx=gpu_ctx)
    assert not np.array_equal(raw[0], exp[0])               # the markup was being hashed


@pytest.mark.parametrize("tokenizer", ["word", "grapheme"])
def test_routes_simhash_tf_and_idf(gpu_ctx, routes, tokenizer):
    from ucfp_amd import text
    pages, want = routes
    html, plain = text.TextOpts(tokenizer=tokenizer, preprocess="html"), text.TextOpts(tokenizer=tokenizer)
    got, exp = text.simhash_batch(pages, html, ctx=gpu_ctx), text.simhash_batch(want, plain, ctx=gpu_ctx)
    assert not exp[1].any() and np.array_equal(got[1], exp[1]) and np.array_equal(got[0], exp[0])
    table = text.IdfTable(plain, ctx=gpu_ctx).fit(want + ["the fox and the dog", "漢字 の テキスト"])
    try:
        got, exp = text.simhash_batch(pages, html, ctx=gpu_ctx, idf=table), text.simhash_batch(want, plain, ctx=gpu_ctx, idf=table)
        assert not exp[1].any() and np.array_equal(got[1], exp[1]) and np.array_equal(got[0], exp[0])
        rec = text.fingerprint_simhash_idf(pages[1], html, table, 1, 2)
        assert rec.text == want[1] and rec.fingerprint == exp[0][1].tobytes()
    finally:
        table.close()
    rec = text.fingerprint_simhash_tf(pages[2], html, 1, 2)
    assert rec.text == want[2] and rec.fingerprint == text.fingerprint_simhash_tf(want[2], plain, 1, 2).fingerprint


def test_routes_tlsh(gpu_ctx, routes):
    from ucfp_amd import text
    pages, want = routes
    html = text.TextOpts(preprocess="html")
    got, exp = text.tlsh_batch(pages, html, ctx=gpu_ctx), text.tlsh_batch(want, ctx=gpu_ctx)
    assert not exp[1][:3].any() and np.array_equal(got[1], exp[1]) and np.array_equal(got[0], exp[0])
    # a `bytes` page is stripped and hashed as the bytes it leaves
    got_b = text.tlsh_batch([p.encode("utf-8") for p in pages], html, ctx=gpu_ctx)
    exp_b = text.tlsh_batch([w.encode("utf-8") for w in want], ctx=gpu_ctx)
    assert np.array_equal(got_b[0], exp_b[0]) and np.array_equal(got_b[1], exp_b[1])
    rec = text.fingerprint_tlsh(pages[0], html, 1, 2)
    assert rec.text == want[0] and rec.fingerprint == text.fingerprint_tlsh(want[0], text.TextOpts(), 1, 2).fingerprint


def test_routes_records(gpu_ctx, routes):
    from ucfp_amd import text
    pages, want = routes
    for tokenizer, h in (("word", 128), ("grapheme", 64)):
        html, plain = text.TextOpts(tokenizer=tokenizer, h=h, preprocess="html"), text.TextOpts(tokenizer=tokenizer, h=h)
        for page, w in zip(pages, want):
            for fn in (text.fingerprint_minhash_with, text.fingerprint_lsh):
                got, exp = fn(page, html, 7, 9), fn(w, plain, 7, 9)
                assert got.text == w and got == exp


def test_html_to_text_batch_takes_str_and_bytes(gpu_ctx, routes):
    from ucfp_amd import text
    pages, want = routes
    got, flags = text.html_to_text_batch(pages + [pages[2].encode("utf-8"), b"<p"], ctx=gpu_ctx)
    assert got == [w.encode("utf-8") for w in want] + [want[2].encode("utf-8"), b""]
    assert flags.dtype == np.uint32 and flags.tolist() == [0, 1, 1, 0, 1, 2]
    assert text.html_to_text_batch([], ctx=gpu_ctx)[0] == []
    # markup between the bytes of one character: the strip takes any bytes, the entries that hash text want UTF-8
    from ucfp_amd.errors import InvalidArgument
    assert text.html_to_text_batch([b"\xc3<p>\xa9"], ctx=gpu_ctx)[0] == [b"\xc3 \xa9"]
    for entry in (text.minhash_batch, text.simhash_batch):
        with pytest.raises(InvalidArgument):
            entry([b"\xc3<p>\xa9"], text.TextOpts(preprocess="html"), ctx=gpu_ctx)


def test_dedup_corpus_sees_through_markup(gpu_ctx):
    from ucfp_amd import text
    prose = " ".join(_PROSE)
    a = "<html><body><p>%s</p></body></html>" % prose
    b = ("<div class='x'><script>var prose = '<p>';</script><!-- %s -->%s</div>"
         % ("tracking > pixel", " ".join("<span>%s</span>" % w if i % 3 else "<b>%s</b>\n" % w for i, w in enumerate(_PROSE))))
    c = "<p>%s</p>" % " ".join(reversed(_PROSE))
    assert ref.html_to_text(a.encode())[0] == ref.html_to_text(b.encode())[0] == prose.encode()
    keep, labels, status = text.dedup_corpus([a, b, c], 0.8, text.TextOpts(preprocess="html"), ctx=gpu_ctx)
    assert not status.any() and keep.tolist() == [True, False, True] and labels.tolist() == [0, 0, 2]


def test_other_preprocess_values_are_refused(gpu_ctx):
    from ucfp_amd import index, terms, text
    from ucfp_amd.errors import UnsupportedError
    page = "<p>%s</p>" % " ".join(_PROSE)
    table = text.IdfTable(ctx=gpu_ctx).fit([page])
    bm25 = index.Bm25Index(ctx=gpu_ctx, keys="hashed")
    try:
        for value in ("markdown", "pdf", "HTML"):
            o = text.TextOpts(preprocess=value)
            calls = [lambda: text.minhash_batch([page], o, ctx=gpu_ctx), lambda: text.simhash_batch([page], o, ctx=gpu_ctx),
                     lambda: text.simhash_batch([page], o, ctx=gpu_ctx, idf=table), lambda: text.tlsh_batch([page], o, ctx=gpu_ctx),
                     lambda: text.tlsh_batch([page.encode()], o, ctx=gpu_ctx),
                     lambda: text.fingerprint_minhash_with(page, o, 1, 2), lambda: text.fingerprint_simhash_tf(page, o, 1, 2),
                     lambda: text.fingerprint_simhash_idf(page, o, None, 1, 2), lambda: text.fingerprint_simhash_idf(page, o, table, 1, 2),
                     lambda: text.fingerprint_lsh(page, o, 1, 2), lambda: text.fingerprint_tlsh(page, o, 1, 2),
                     lambda: text.dedup_corpus([page], 0.8, o, ctx=gpu_ctx), lambda: text.dedup_corpus([], 0.8, o, ctx=gpu_ctx)]
            for i, call in enumerate(calls):
                with pytest.raises(UnsupportedError):
                    call()
        # the entries that take no preprocess yet refuse "html" as well
        for value in ("markdown", "html"):
            o = text.TextOpts(preprocess=value)
            calls = [lambda: text.StreamingMinHashSession(o, 1, 2), lambda: text.StreamingSimHashSession(o, 1, 2),
                     lambda: text.ingest_stream_ndjson(b'"a b c d e f"\n', o, 1, 2), lambda: text.TextBatcher("minhash", o, ctx=gpu_ctx),
                     lambda: text.TextBatcher("simhash", o, ctx=gpu_ctx), lambda: terms.terms_batch([page], ctx=gpu_ctx, preprocess=value),
                     lambda: bm25.upsert(0, [1], [page], preprocess=value), lambda: text.IdfTable(o, ctx=gpu_ctx).add([page])]
            for call in calls:
                with pytest.raises(UnsupportedError):
                    call()
    finally:
        table.close()
        bm25.close()
