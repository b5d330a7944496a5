"""TF.IDF SimHash on the GPU: the weighted fold, the table, the fit and the interface, every record and
count compared bit for bit with the plain-Python restatement (tests/simhash_idf_ref.py)."""
import numpy as np
import pytest

from ucfp_amd import _lib, text
from ucfp_amd.errors import InvalidArgument, UnsupportedError

import simhash_idf_ref as ref
import text_canon_ref as canon_ref

pytestmark = pytest.mark.gpu

A, P, U = text.RAW_ASCII, text.PRETOKENIZED, text.RAW_UTF8
WORD, GRAPHEME = text.TOK_WORD, text.TOK_GRAPHEME
ONE = 0x10000
VOCAB = [f"w{i}".encode() for i in range(40)] + [b"the", b"of", b"and", b"zebra", b"quartz", b"x" * 70, b"y" * 300]


def _table(gpu_ctx, weights, default, **kw):
    """A supplied table from {key int: q16}."""
    t = text.IdfTable(ctx=gpu_ctx, **kw)
    keys = np.array(list(weights), np.uint64)
    wts = np.array([weights[k] for k in weights], np.uint32)
    return t._set_q16(keys, wts, default)


def _expect(docs_tokens, weights, default):
    recs, sts = zip(*[ref.simhash_weighted(d, weights, default) if d is not None else (bytes(8), None) for d in docs_tokens])
    return np.frombuffer(b"".join(recs), np.uint8).reshape(-1, 8), list(sts)


def _check_tokens(gpu_ctx, docs, weights, default):
    t = _table(gpu_ctx, weights, default)
    got, st = text.simhash_tokens(docs, ctx=gpu_ctx, idf=t)
    exp, est = _expect(docs, weights, default)
    assert list(st) == est
    assert np.array_equal(got, exp)
    t.close()
    return got


def _weights_for(rng, tokens, frac=0.7):
    return {ref.key(t): int(rng.integers(0, 1 << 32)) for t in tokens if rng.random() < frac}


# ---------------------------------------------------------------- the fold

def test_fold_over_several_lds_batches(gpu_ctx):
    rng = np.random.default_rng(1)
    doc = [VOCAB[int(i)] for i in rng.integers(0, 45, 600)]          # 600 tokens: more than two batches of 256
    w = _weights_for(rng, VOCAB)
    docs = [doc, doc[:256], doc[:257], doc[:512], doc[:1]]
    _check_tokens(gpu_ctx, docs, w, 12345)
    t = _table(gpu_ctx, w, 12345)
    got, st = text.simhash_batch([b" ".join(d).decode() for d in docs], ctx=gpu_ctx, idf=t)
    exp, _ = _expect(docs, w, 12345)
    assert not st.any() and np.array_equal(got, exp)
    t.close()


def test_ties_carries_zero_weights_and_defaults(gpu_ctx):
    a, b, c, d = b"alpha", b"beta", b"gamma", b"delta"
    ka, kb, kc = ref.key(a), ref.key(b), ref.key(c)
    # two tokens of equal weight: every differing bit ties and is clear
    got = _check_tokens(gpu_ctx, [[a, b]], {ka: 777, kb: 777}, ONE)
    assert int.from_bytes(got[0].tobytes(), "little") == ka & kb
    # three tokens of weight 0xFFFF0000: the sums pass 2^32
    got = _check_tokens(gpu_ctx, [[a, b, c], [a, a, a, b, b, c] * 50], {ka: 0xFFFF0000, kb: 0xFFFF0000, kc: 0xFFFF0000}, 1)
    assert int.from_bytes(got[0].tobytes(), "little") == (ka & kb) | (ka & kc) | (kb & kc)
    # a weight-0 token among others; only weight-0 tokens: -1 and a zero record
    t = _table(gpu_ctx, {kb: 0}, 5)
    got, st = text.simhash_tokens([[a, b, b, b], [b, b], [b], [d]], ctx=gpu_ctx, idf=t)
    exp, est = _expect([[a, b, b, b], [b, b], [b], [d]], {kb: 0}, 5)
    assert list(st) == est == [0, -1, -1, 0] and np.array_equal(got, exp) and not got[1].any()
    assert got[0].tobytes() == ka.to_bytes(8, "little")
    t.close()
    # unknown tokens take the default, 0 included
    _check_tokens(gpu_ctx, [[a, d, d], [d]], {ka: 3 * ONE}, 2 * ONE)
    _check_tokens(gpu_ctx, [[a, d, d], [d]], {ka: 3 * ONE}, 0)


def test_every_route_gives_one_record(gpu_ctx):
    rng = np.random.default_rng(2)
    words = [b"alpha", b"beta", b"gamma9", b"x1y2", b"delta", b"the", b"of"]
    docs = [[words[int(i)] for i in rng.integers(0, len(words), n)] for n in (1, 7, 64, 300, 520)]
    w = _weights_for(rng, words, 0.6)
    t = _table(gpu_ctx, w, 9 * ONE)
    exp, _ = _expect(docs, w, 9 * ONE)
    raw = [b", ".join(d).upper() + b"." for d in docs]            # mode 0 and mode 2 lower-case and cut at the punctuation
    for mode, blob in ((A, raw), (U, raw), (P, [b" ".join(d) for d in docs])):
        got, st = t._simhash_docs(gpu_ctx, blob, mode, WORD)
        assert not st.any() and np.array_equal(got, exp), mode
    got, st = t._simhash_tokens(docs, gpu_ctx)
    assert not st.any() and np.array_equal(got, exp)
    t.close()


def test_grapheme_routes(gpu_ctx):
    rng = np.random.default_rng(3)
    asc = [b"Hello, World!\r\nHello", b"a", b"aAbB\r\n\r\n" * 70, bytes(rng.integers(1, 128, 700, dtype=np.uint8))]
    utf = ["héllo wörld ñandú\r\n".encode(), "Éé".encode() * 200, b"plain ascii too"]
    for docs, mode in ((asc, A), (utf, U)):
        toks = [ref.graphemes(d, mode) for d in docs]
        assert all(x is not None for x in toks)
        w = _weights_for(rng, {g for x in toks for g in x}, 0.5)
        t = _table(gpu_ctx, w, 40000)
        got, st = t._simhash_docs(gpu_ctx, docs, mode, GRAPHEME)
        exp, est = _expect(toks, w, 40000)
        assert list(st) == est and np.array_equal(got, exp), mode
        t.close()
    # statuses are those of the TF entries: a byte >= 0x80 in mode 0, a document the device hands back in mode 2
    t = _table(gpu_ctx, {}, ONE)
    assert list(t._simhash_docs(gpu_ctx, [b"caf\xc3\xa9", b""], A, GRAPHEME)[1]) == [1, -1]
    assert list(t._simhash_docs(gpu_ctx, [b"caf\xc3\xa9", b"\xff"], A, WORD)[1]) == [1, 1]
    o, s = t._simhash_docs(gpu_ctx, ["é".encode(), b"ok"], U, WORD)
    assert list(s) == [1, 0] and not o[0].any()
    t.close()


def test_equal_weights_are_tf(gpu_ctx):
    import random
    rng, prng = np.random.default_rng(4), random.Random(4)
    texts = []
    for i in range(300):
        if i % 2:
            texts.append(canon_ref.random_string(prng, 0, 200))
        else:
            texts.append(" ".join(VOCAB[int(j)].decode() for j in rng.integers(0, 45, int(rng.integers(0, 60)))))
    tf, tf_st = text.simhash_batch(texts, ctx=gpu_ctx)
    flat = text.IdfTable.from_weights({}, default=1.0, ctx=gpu_ctx)
    empty = text.IdfTable(ctx=gpu_ctx).finalize()
    assert not flat and not empty and empty.is_final and len(empty) == 0
    for t in (flat, empty):
        got, st = text.simhash_batch(texts, ctx=gpu_ctx, idf=t)
        assert np.array_equal(st, tf_st) and np.array_equal(got, tf)
        t.close()


# ---------------------------------------------------------------- the table

def _roundtrip(gpu_ctx, weights, default, **kw):
    t = _table(gpu_ctx, weights, default, **kw)
    e = t.export()
    ks = sorted(weights)
    assert len(t) == len(weights) and t.is_final and t.n_docs == 0
    assert e["keys"].tolist() == ks and e["weights"].tolist() == [weights[k] for k in ks] and e["default"] == default
    assert not e["dfs"].any()
    return t


def test_table_holds_every_key(gpu_ctx):
    rng = np.random.default_rng(5)
    toks = VOCAB[:20]
    docs = [[toks[int(i)] for i in rng.integers(0, 20, 50)], toks[:10], toks[10:]]
    real = {ref.key(t): int(rng.integers(0, 1 << 32)) for t in toks[:10]}            # the documents hit these and miss the rest
    low = {(i << 20) | 0xABCDE: 1000 + i for i in range(64)}                         # share their low 20 bits
    high = {(0xABCDE << 44) | (i * 0x10001): 2000 + i for i in range(64)}            # share their high 20 bits
    many = {int(k): int(v) for k, v in zip(rng.integers(0, 1 << 64, 5000, dtype=np.uint64), rng.integers(0, 1 << 32, 5000))}
    for raw, kw in (({0: 11, (1 << 64) - 1: 22}, {}), (low, {}), (high, {}), (many, {"capacity_hint": 16})):
        weights = dict(raw)
        weights.update(real)
        t = _roundtrip(gpu_ctx, weights, 4242, **kw)
        got, st = text.simhash_tokens(docs, ctx=gpu_ctx, idf=t)
        exp, _ = _expect(docs, weights, 4242)
        assert not st.any() and np.array_equal(got, exp)
        t.close()
    # key 0 absent: it takes the default like any other
    t = _roundtrip(gpu_ctx, {5: 1}, 99)
    assert t.weight(0) == 99 / 65536 and t.weight(5) == 1 / 65536 and t.weight((1 << 64) - 1) == 99 / 65536
    t.close()


def test_duplicate_key_is_refused_without_change(gpu_ctx):
    t = _roundtrip(gpu_ctx, {1: 10, 2: 20, 0: 30}, 7)
    before = t.export()
    for keys in ([9, 9], [0, 4, 0], [3, 2 ** 64 - 1, 2 ** 64 - 1]):
        with pytest.raises(InvalidArgument):
            t._set_q16(np.array(keys, np.uint64), np.ones(len(keys), np.uint32), 1)
    after = t.export()
    assert all(np.array_equal(before[k], after[k]) for k in ("keys", "dfs", "weights")) and after["default"] == 7 and t.is_final
    t.close()


def test_from_weights_keys_and_quantisation(gpu_ctx):
    t = text.IdfTable.from_weights({"Straße": 2.5, b"raw bytes": 0.0, 17: 1.0 / 3}, default=0.25, ctx=gpu_ctx)
    e = t.export()
    want = {ref.key("strasse".encode()): int(2.5 * 65536), ref.key(b"raw bytes"): 0, 17: int(np.floor(65536 / 3 + 0.5))}
    assert dict(zip(e["keys"].tolist(), e["weights"].tolist())) == want and e["default"] == 16384
    assert t.weight("STRASSE") == 2.5 and t.weight("unseen") == 0.25
    d = t.digest
    t2 = text.IdfTable.load(e, ctx=gpu_ctx)
    assert t2.digest == d and text.IdfTable.from_weights({17: 0.5}, ctx=gpu_ctx).digest != d
    for bad in (-0.1, float("nan"), 65536.0):
        with pytest.raises(InvalidArgument):
            text.IdfTable.from_weights({1: bad}, ctx=gpu_ctx)
    t.close(), t2.close()


# ---------------------------------------------------------------- the fit

@pytest.fixture(scope="module")
def corpus():
    """300 ASCII documents, tokens repeated within and across them; 12 of them get a status != 0 in mode 0."""
    rng = np.random.default_rng(6)
    docs = []
    for i in range(300):
        n = int(rng.integers(1, 80))
        docs.append(b" ".join(VOCAB[int(j)] for j in rng.integers(0, 47, n)))
    docs[7] = b" ".join(VOCAB[int(j)] for j in rng.integers(0, 40, 1500))          # > 4096 bytes: a piece of its own
    for i in (20, 120, 220, 299):
        docs[i] = b""                                                               # -1
    for i in (21, 121, 221, 0):
        docs[i] = docs[i] + b" caf\xc3\xa9 " + docs[i]                              # a byte >= 0x80 in mode 0: 1
    for i in (22, 122, 222, 298):
        docs[i] = b"early tokens of the long one " + b"z" * 1600 + b" late"         # -2, after tokens were emitted
    toks = [None if i in (20, 120, 220, 299, 21, 121, 221, 0, 22, 122, 222, 298) else ref.words(d, A) for i, d in enumerate(docs)]
    return docs, toks


def _check_fit(t, toks):
    n, df = ref.fit(toks)
    e = t.export()
    assert t.n_docs == n == e["n_docs"] and len(t) == len(df)
    assert dict(zip(e["keys"].tolist(), e["dfs"].tolist())) == df
    return n, df, e


def test_fit_counts_and_weights(gpu_ctx, corpus):
    docs, toks = corpus
    t = text.IdfTable(ctx=gpu_ctx, capacity_hint=16, piece_tokens=4096)             # grows several times, several pieces
    _, st = t._add_docs(docs, A, WORD)
    assert [int(s) for s in st] == [0 if x is not None else {b"": -1}.get(docs[i], 1 if b"\xc3" in docs[i] else -2)
                                    for i, x in enumerate(toks)]
    assert not t.is_final
    with pytest.raises(InvalidArgument):
        text.simhash_batch(["a b"], ctx=gpu_ctx, idf=t)                             # not final
    n, df, _ = _check_fit(t, toks)
    assert ref.key(b"early") not in df and ref.key(b"caf") not in df               # nothing of a refused document
    t.finalize()
    e = t.export()
    assert t.is_final and e["default"] == ref.weight_q16(n, 0)
    assert e["weights"].tolist() == [ref.weight_q16(n, int(d)) for d in e["dfs"]]
    weights, default = ref.weights_of(n, df)
    texts = [d.decode() for d, x in zip(docs, toks) if x is not None][:60] + ["unseen words only", "the zebra of quartz"]
    got, st = text.simhash_batch(texts, ctx=gpu_ctx, idf=t)
    exp, est = _expect([ref.words(x.encode(), A) for x in texts], weights, default)
    assert list(st) == est and np.array_equal(got, exp)
    # load(export()) reproduces the records
    t2 = text.IdfTable.load(e, ctx=gpu_ctx)
    got2, _ = text.simhash_batch(texts, ctx=gpu_ctx, idf=t2)
    assert np.array_equal(got2, got) and t2.digest == t.digest
    # add after finalize: not final any more; the counts go on
    t.add(["the zebra the zebra"])
    assert not t.is_final and t.n_docs == n + 1
    with pytest.raises(InvalidArgument):
        text.simhash_tokens([[b"a"]], ctx=gpu_ctx, idf=t)
    t.finalize()
    assert dict(zip(*(t.export()[k].tolist() for k in ("keys", "dfs"))))[ref.key(b"zebra")] == df.get(ref.key(b"zebra"), 0) + 1
    t.close(), t2.close()


def test_fit_in_two_calls_every_route(gpu_ctx, corpus):
    docs, toks = corpus
    good = [d.decode() for d, x in zip(docs, toks) if x is not None]
    utf = ["café au lait 中文 café", "Über straße über", "é handed back to the host"]
    texts = good[:80] + utf + good[80:160]
    want = [ref.words(x.encode(), A) if x.isascii() else [t.encode() for t in text._host_tokens(text.Canonicalizer().apply(x))]
            for x in texts]
    one, two = text.IdfTable(ctx=gpu_ctx), text.IdfTable(ctx=gpu_ctx, capacity_hint=16, piece_tokens=4096)
    assert not one.add(texts).any()
    assert not two.add(texts[:50]).any() and not two.add(texts[50:]).any()
    _, _, e1 = _check_fit(one, want)
    _, _, e2 = _check_fit(two, want)
    assert all(np.array_equal(e1[k], e2[k]) for k in ("keys", "dfs"))
    # the token form and the grapheme tokeniser count the same way
    tk = text.IdfTable(ctx=gpu_ctx, piece_tokens=64)
    st = tk.add_tokens(want + [[], [b"", b""]])
    assert list(st) == [0] * len(want) + [-1, -1]
    _check_fit(tk, want)
    g = text.IdfTable(text.TextOpts(tokenizer="grapheme"), ctx=gpu_ctx, piece_tokens=512)
    gtexts = ["Hello, World!\r\n", "héllo héllo", "aaa", ""]
    assert list(g.fit(gtexts).add(gtexts[:1])) == [0]
    _check_fit(g, [ref.graphemes(x.encode(), A if x.isascii() else U) for x in gtexts] + [ref.graphemes(gtexts[0].encode(), A)])
    for t in (one, two, tk, g):
        t.close()


# ---------------------------------------------------------------- interface

def test_fingerprint_simhash_idf(gpu_ctx):
    """Three boilerplate tokens, two rare ones, a table fitted on 50 boilerplate-heavy documents.

    With EACH boilerplate token 20 times the weighted record cannot differ from the TF record under T9.4, whatever the
    keys: a boilerplate weight is wb >= 1.0, a rare one wr <= weight(0) = 1 + log2(51) = 6.67 at N = 50.  A bit held by two
    boilerplate tokens has 2 pos >= 80 wb > 60 wb + 2 wr = tot and is set in both records; a bit held by one has
    2 pos <= 40 wb + 4 wr < 60 wb + 2 wr (as wr < 10 wb) and is clear in both.  That document is therefore checked for its
    tag and against the restatement only.  The difference is shown on the document with 20 boilerplate occurrences in all
    (7 + 7 + 6): there a bit held by both rare tokens and one boilerplate token is set by IDF (2 (6 + 13.3) > 33.3) and
    clear in TF (2 (6 + 2) < 22); the rare pair is searched for with the restatement, so the assertion cannot miss."""
    boiler = ["lorem", "ipsum", "dolor"]
    corpus = [" ".join(boiler * (3 + i % 4) + [f"rare{i}"]) for i in range(50)]
    opts = text.TextOpts()
    t = text.IdfTable(opts, ctx=gpu_ctx).fit(corpus)
    n, df = ref.fit([ref.words(c.encode(), A) for c in corpus])
    weights, default = ref.weights_of(n, df)
    assert t.n_docs == 50 and bool(t)
    assert all(weights[ref.key(b.encode())] == ONE for b in boiler) and default == ref.weight_q16(50, 0)

    def check(doc):
        rec = text.fingerprint_simhash_idf(doc, opts, t, 1, 2)
        assert rec.algorithm == "simhash-b64-idf" and len(rec.fingerprint) == 8
        assert rec.fingerprint == ref.simhash_weighted(ref.words(doc.encode(), A), weights, default)[0]
        tf = text.fingerprint_simhash_tf(doc, opts, 1, 2)
        assert text.fingerprint_simhash_idf(doc, opts, None, 1, 2).fingerprint == tf.fingerprint      # unchanged
        return rec.fingerprint, tf.fingerprint

    check(" ".join(boiler * 20 + ["aardvark", "zeppelin"]))
    few = ["lorem"] * 7 + ["ipsum"] * 7 + ["dolor"] * 6
    for i in range(100):                                     # construct the pair: rare tokens whose keys make a bit differ
        rare = [f"aardvark{i}", f"zeppelin{i}"]
        toks = [x.encode() for x in few + rare]
        if ref.simhash_weighted(toks, weights, default) != ref.simhash_weighted(toks, {}, ONE):
            break
    else:
        raise AssertionError("no rare pair found")
    idf_rec, tf_rec = check(" ".join(few + rare))
    assert idf_rec != tf_rec
    with pytest.raises(UnsupportedError):
        text.fingerprint_simhash_idf(" ".join(few), opts, {"lorem": 1.0}, 1, 2)
    t.close()


def test_dev_entries_on_a_stream(gpu_ctx, torch_cuda, corpus):
    torch = torch_cuda
    lib = _lib.load()
    docs, toks = corpus
    docs, toks = docs[:64], toks[:64]
    host = text.IdfTable(ctx=gpu_ctx, piece_tokens=4096)
    _, h_st = host._add_docs(docs, A, WORD)
    host.finalize()
    blob, offs = text._pack(docs)
    n = len(docs)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_blob, d_offs = torch.from_numpy(blob.copy()).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
        d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
        dev = text.IdfTable(ctx=gpu_ctx, piece_tokens=4096)
        _lib.check(lib.ucfp_idf_table_add_batch_dev(dev.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, A, WORD, d_st.data_ptr(),
                                                    s.cuda_stream))
        _lib.check(lib.ucfp_idf_table_finalize(dev.handle, s.cuda_stream))
        s.synchronize()
        assert np.array_equal(d_st.cpu().numpy(), h_st)
        eh, ed = host.export(), dev.export()
        assert all(np.array_equal(eh[k], ed[k]) for k in ("keys", "dfs", "weights")) and eh["default"] == ed["default"]
        _lib.check(lib.ucfp_text_simhash_idf_batch_dev(gpu_ctx.handle, dev.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, A, WORD,
                                                       d_out.data_ptr(), d_st.data_ptr(), s.cuda_stream))
        s.synchronize()
        h_out, h_st2 = host._simhash_docs(gpu_ctx, docs, A, WORD)
        assert np.array_equal(d_out.cpu().numpy(), h_out) and np.array_equal(d_st.cpu().numpy(), h_st2)
        # the token form, fit and record
        tdocs = [x or [] for x in toks]
        tb, to, dt = text._pack_tokens(tdocs)
        d_tb, d_to, d_dt = (torch.from_numpy(a.copy().view(np.int64) if a.dtype == np.uint64 else a.copy()).cuda() for a in (tb, to, dt))
        dev2 = text.IdfTable(ctx=gpu_ctx, piece_tokens=100)
        _lib.check(lib.ucfp_idf_table_add_tokens_batch_dev(dev2.handle, d_tb.data_ptr(), d_to.data_ptr(), d_dt.data_ptr(), n,
                                                           d_st.data_ptr(), s.cuda_stream))
        s.synchronize()
        e2 = dev2.export()
        assert all(np.array_equal(eh[k], e2[k]) for k in ("keys", "dfs")) and dev2.n_docs == host.n_docs
        _lib.check(lib.ucfp_text_simhash_idf_tokens_batch_dev(gpu_ctx.handle, dev.handle, d_tb.data_ptr(), d_to.data_ptr(),
                                                              d_dt.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), s.cuda_stream))
        s.synchronize()
        t_out, t_st = host._simhash_tokens(tdocs, gpu_ctx)
        assert np.array_equal(d_out.cpu().numpy(), t_out) and np.array_equal(d_st.cpu().numpy(), t_st)
        # a non-final table is refused by the _dev entries too
        assert lib.ucfp_text_simhash_idf_batch_dev(gpu_ctx.handle, dev2.handle, d_blob.data_ptr(), d_offs.data_ptr(), n, A, WORD,
                                                   d_out.data_ptr(), d_st.data_ptr(), s.cuda_stream) == -4
    for t in (host, dev, dev2):
        t.close()
