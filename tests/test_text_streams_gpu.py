"""Streaming MinHash (ucfp_amd/csrc/text_streams.hip) on the GPU.  A stream's final record and status
must be those of the whole document, however it is cut: the expected value is always the CPU oracle's
text_minhash_batch on the concatenation, and the offline GPU entry is asserted equal to it too."""
import numpy as np
import pytest

from ucfp_amd import text as T
from ucfp_amd.errors import InvalidArgument, ModalityError, UnsupportedError

pytestmark = pytest.mark.gpu

RAW, PRETOK, UTF8 = 0, 1, 2
NEEDS_HOST, E_MODALITY, E_UNSUPPORTED = 1, -1, -2

_WORDS = ("the quick brown fox jumps over lazy dog it's 3.14 a:b x.y. 1,000;2 _a Upper CASE end. stream minhash wave "
          "token shingle batch flush carry lane k9 0x1f q").split()


def _prose(rng, n_bytes, seps=(" ", " ", " ", ", ", ". ", "\n", "  ", "; ")):
    out, size = [], 0
    while size < n_bytes:
        w = _WORDS[int(rng.integers(len(_WORDS)))] + seps[int(rng.integers(len(seps)))]
        out.append(w)
        size += len(w)
    return "".join(out)[:n_bytes].encode("ascii")


def _cut(doc, sizes):
    """doc -> chunks of the given sizes in turn (the sizes repeat); never empty for an empty doc."""
    chunks, at, i = [], 0, 0
    while at < len(doc):
        chunks.append(doc[at:at + sizes[i % len(sizes)]])
        at += sizes[i % len(sizes)]
        i += 1
    return chunks or [b""]


def _expected(oracle, gpu_ctx, docs, mode, k):
    """The oracle's records and statuses of the whole documents; the offline GPU entry agrees."""
    rec, st = oracle.text_minhash_batch(docs, mode, k)
    grec, gst = T._run("minhash", docs, mode, k, gpu_ctx)
    assert np.array_equal(gst, st) and np.array_equal(grec, rec)
    return rec, st


def _advance(streams, chunked, mode, history=None):
    """Opens one stream per chunk list and advances them together, one chunk each per push, the last chunk final.
    -> (records [n, 1032] uint8, status [n]).  `history[i]` collects stream i's status after every push."""
    slots = [streams.open(mode) for _ in chunked]
    assert len(set(slots)) == len(slots)
    rec = np.zeros((len(chunked), 1032), np.uint8)
    st = np.full(len(chunked), 99, np.int32)
    for r in range(max(len(c) for c in chunked)):
        live = [i for i, c in enumerate(chunked) if r < len(c)]
        fin = [slots[i] for i in live if r == len(chunked[i]) - 1]
        got = streams.push({slots[i]: chunked[i][r] for i in live}, final=fin)
        for i in live:
            record, status = got[slots[i]]
            if history is not None:
                history[i].append(status)
            assert (record is not None) == (slots[i] in fin)
            if record is not None:
                rec[i] = np.frombuffer(record, np.uint8)
                st[i] = status
    return rec, st


def _check(oracle, gpu_ctx, streams, docs, chunked, mode, k, history=None):
    for d, c in zip(docs, chunked):
        assert b"".join(c) == d
    want, want_st = _expected(oracle, gpu_ctx, docs, mode, k)
    rec, st = _advance(streams, chunked, mode, history)
    bad = [i for i in range(len(docs)) if st[i] != want_st[i] or not np.array_equal(rec[i], want[i])]
    assert not bad, (bad[:8], st[bad[:8]], want_st[bad[:8]])
    return want, want_st


EDGE_DOC = (b"It's 3.14 here: a:b and x.y. then 1,000;2 _a b_ UPPER Case mixed; don't 'quote' 1.2.3 a..b 4,5, x:y:z "
            b"The Quick brown Fox, jumps over the lazy dog's back 42 times; o'clock 7:30 pm e.g. i.e. U.S.A. end.")


@pytest.mark.parametrize("k", [1, 5, 64])
def test_every_two_chunk_cut(oracle, gpu_ctx, k):
    """One stream per cut position, all advanced together: two pushes, the second final."""
    doc = EDGE_DOC
    assert 180 <= len(doc) <= 220 and doc.endswith(b".")
    for piece in (b"It's", b"3.14", b"a:b", b"x.y.", b"1,000;2", b"_a"):
        assert piece in doc
    cuts = list(range(len(doc) + 1))
    s = T.MinHashStreams(len(cuts), k, gpu_ctx)
    try:
        _check(oracle, gpu_ctx, s, [doc] * len(cuts), [[doc[:c], doc[c:]] for c in cuts], RAW, k)
    finally:
        s.destroy()


def test_one_byte_chunks(oracle, gpu_ctx):
    rng = np.random.default_rng(1)
    docs = [_prose(rng, 280 + int(rng.integers(0, 40))) for _ in range(64)]
    assert len(set(docs)) == 64
    s = T.MinHashStreams(64, 5, gpu_ctx)
    try:
        _check(oracle, gpu_ctx, s, docs, [[d[i:i + 1] for i in range(len(d))] for d in docs], RAW, 5)
    finally:
        s.destroy()


def test_state_carried_across_lds_flushes(oracle, gpu_ctx):
    """8 KiB documents (several LDS batches each) at chunk sizes around the 64-byte step, the 256-byte stage and the
    1536-byte batch, with empty pushes in between; one 1000-byte token that spans four pushes."""
    rng = np.random.default_rng(2)
    docs, chunked = [], []
    for sizes in ([63], [64], [65], [255], [256], [257], [1535], [int(v) for v in rng.integers(1, 701, 64)]):
        d = _prose(rng, 8192)
        assert len(oracle.text_canon(d, RAW)[0].split(b" ")) > 256
        c = _cut(d, sizes)
        if len(c) > 4:
            c.insert(3, b"")            # empty non-final pushes, one right after the other too
            c.insert(3, b"")
            c.insert(len(c) - 1, b"")
        docs.append(d)
        chunked.append(c)
    long_tok = bytes(rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8), 1000))
    d = b"one two three " + long_tok + b" four five six seven eight"
    c = _cut(d, [300])
    assert sum(1 for x in range(0, len(d), 300) if x < 14 + 1000 and x + 300 > 14) == 4     # the token's bytes lie in 4 chunks
    docs.append(d)
    chunked.append(c)
    s = T.MinHashStreams(len(docs), 5, gpu_ctx)
    try:
        want, want_st = _check(oracle, gpu_ctx, s, docs, chunked, RAW, 5)
        assert (want_st == 0).all()
    finally:
        s.destroy()


def test_short_and_empty_streams(oracle, gpu_ctx):
    docs = [b"a b c", b" .,; -- ", b"", b"", b"word", b"a b c d e"]
    chunked = [[b"a b", b" c"], [b" .,", b"; -- "], [b""], [b"", b"", b""], [b"wo", b"rd"], [b"a b c d", b" e"]]
    s = T.MinHashStreams(len(docs), 5, gpu_ctx)
    try:
        want, want_st = _check(oracle, gpu_ctx, s, docs, chunked, RAW, 5)
        assert list(want_st) == [0, E_MODALITY, E_MODALITY, E_MODALITY, 0, 0]
        assert want[0].any() and not want[1].any() and not want[2].any()
        one, _ = oracle.text_minhash_batch([b"a b c"], PRETOK, 3)        # fewer than k tokens: ONE shingle of all of them
        assert np.array_equal(want[0], one[0])
    finally:
        s.destroy()


def test_pretokenized(oracle, gpu_ctx):
    docs = [b"ab\x00cd e\x00 \x00 f g h i", b"a  b   c    d e  f", b"tok1 tok2 tok3 tok4 tok5 tok6", b"\xc3\xa9t\xc3\xa9 \xe4\xb8\xad \xe6\x96\x87 a b c"]
    chunked = [[b"ab\x00", b"cd e\x00 \x00", b" f g h i"], [b"a  b ", b"  c ", b"   d e", b"  f"],
               [b"tok1 tok2 ", b"tok3 tok4", b" tok5 tok6"], [b"\xc3", b"\xa9t\xc3\xa9 \xe4\xb8", b"\xad \xe6\x96\x87 a b c"]]
    assert chunked[2][0].endswith(b" ") and chunked[2][2].startswith(b" ")
    s = T.MinHashStreams(len(docs), 3, gpu_ctx)
    try:
        _, want_st = _check(oracle, gpu_ctx, s, docs, chunked, PRETOK, 3)
        assert (want_st == 0).all()
    finally:
        s.destroy()


def test_needs_host_is_sticky(oracle, gpu_ctx):
    docs = [b"plain ascii words caf\xc3\xa9 and more words after it to the very end",
            b"the high byte is the last of its chunk\xe9 and the text goes on and on"]
    chunked = [[docs[0][:12], docs[0][12:30], docs[0][30:45], docs[0][45:]],
               [docs[1][:20], docs[1][20:39], docs[1][39:50], docs[1][50:]]]
    for d, c in zip(docs, chunked):
        assert max(c[0]) < 0x80 and max(c[1]) >= 0x80
    assert chunked[1][1][-1] == 0xe9        # held back by push 2, yet seen by it
    hist = [[], []]
    s = T.MinHashStreams(2, 5, gpu_ctx)
    try:
        want, want_st = _check(oracle, gpu_ctx, s, docs, chunked, RAW, 5, hist)
        assert list(want_st) == [NEEDS_HOST, NEEDS_HOST] and not want.any()
        assert hist == [[0, NEEDS_HOST, NEEDS_HOST, NEEDS_HOST]] * 2
    finally:
        s.destroy()


def test_window_limit(oracle, gpu_ctx):
    rng = np.random.default_rng(3)
    pool = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8)
    toks = [bytes(rng.choice(pool, n)) for n in (280, 280, 280, 280, 281)]
    window = b" ".join(toks)
    assert len(window) == T.MAX_WINDOW_BYTES == 1405
    doc = b"a few short words first " + window + b" and some more after it x y z"
    cuts = list(range(700, 764))
    s = T.MinHashStreams(64, 5, gpu_ctx)
    try:
        _, want_st = _check(oracle, gpu_ctx, s, [doc] * 64, [[doc[:c], doc[c:]] for c in cuts], RAW, 5)
        assert (want_st == 0).all()
    finally:
        s.destroy()
    # a 1537-byte window is longer than the LDS batch: refused offline and by a stream, sticky
    big = b"some words " + bytes(rng.choice(pool, 1537)) + b" and the rest of the text " + _prose(rng, 800)
    _, off_st = T._run("minhash", [big], RAW, 5, gpu_ctx)
    assert off_st[0] == E_UNSUPPORTED
    hist = [[]]
    s = T.MinHashStreams(1, 5, gpu_ctx)
    try:
        rec, st = _advance(s, [_cut(big, [400])], RAW, hist)
        assert st[0] == E_UNSUPPORTED and not rec.any()
        first = hist[0].index(E_UNSUPPORTED)
        assert 0 < first < len(hist[0]) - 1 and set(hist[0][:first]) == {0} and set(hist[0][first:]) == {E_UNSUPPORTED}
    finally:
        s.destroy()


def test_many_streams(oracle, gpu_ctx):
    """1024 slots; pushes of 1, 4, 5 and 1023 entries in shuffled slot order; opens, closes and finals interleaved."""
    rng = np.random.default_rng(4)
    N = 1024
    docs = [_prose(rng, 40 + int(rng.integers(0, 120))) for _ in range(N + 3)]
    want, want_st = _expected(oracle, gpu_ctx, docs, RAW, 5)
    s = T.MinHashStreams(N, 5, gpu_ctx)
    try:
        slots = [s.open(RAW) for _ in range(N)]
        assert sorted(slots) == list(range(N))
        with pytest.raises(InvalidArgument, match="slots are open"):
            s.open(RAW)
        doc_of = {sl: i for i, sl in enumerate(slots)}       # slot -> document
        at = {sl: 0 for sl in slots}                          # bytes pushed
        done = {}                                             # document -> (record, status)

        def push(sls, finish=()):
            finish = set(finish)
            chunks = {}
            for sl in sls:
                d = docs[doc_of[sl]]
                left = len(d) - at[sl]
                n = left if sl in finish else int(rng.integers(0, min(50, left) + 1))
                chunks[sl] = d[at[sl]:at[sl] + n]
                at[sl] += n
            got = s.push(chunks, final=finish)
            for sl in finish:
                done[doc_of[sl]] = got[sl]

        order = [int(v) for v in rng.permutation(N)]
        push(order[:1])
        push(order[1:5])
        push(order[:5], finish=order[2:4])                   # two of the five end here
        s.close(order[4])                                     # one is discarded
        dropped = doc_of[order[4]]
        reopened = [s.open(RAW) for _ in range(3)]            # the three free slots come back and start clean
        assert reopened == sorted(order[2:5])
        for j, sl in enumerate(reopened):
            doc_of[sl], at[sl] = N + j, 0
        live = [int(v) for v in rng.permutation(N)]
        push(live[:1023], finish=live[:300])
        push(live[300:], finish=live[300:])                  # 723 second pushes and one first push, all final
        assert sorted(done) == [i for i in range(N + 3) if i != dropped]
        for i, (record, status) in done.items():
            assert status == want_st[i] and np.array_equal(np.frombuffer(record, np.uint8), want[i]), i
        assert s.open(RAW) == 0                               # every final freed its slot
    finally:
        s.destroy()


def test_errors(oracle, gpu_ctx, torch_cuda):
    for k in (0, 65):
        with pytest.raises(ModalityError, match=r"shingle k must be in \[1, 64\]"):
            T.MinHashStreams(4, k, gpu_ctx)
    docs = [b"alpha beta gamma delta epsilon zeta eta theta", b"one two three four five six seven eight nine"]
    want, want_st = _expected(oracle, gpu_ctx, docs, RAW, 5)
    d_bytes = torch_cuda.zeros(16, dtype=torch_cuda.uint8, device="cuda")
    d_st = torch_cuda.zeros(4, dtype=torch_cuda.int32, device="cuda")
    s = T.MinHashStreams(4, 5, gpu_ctx)
    try:
        with pytest.raises(UnsupportedError, match="RAW_UTF8"):
            s.open(UTF8)
        with pytest.raises(InvalidArgument, match="unknown text mode"):
            s.open(7)
        a, b = s.open(RAW), s.open(RAW)
        s.push({a: docs[0][:10], b: docs[1][:13]})
        for bad, why in (([a, 4], "out of range"), ([a, 3], "not open"), ([b, a, b], "twice")):
            with pytest.raises(InvalidArgument, match=why):
                s.push_dev(bad, [1] * len(bad), d_bytes, None, d_st)
        with pytest.raises(InvalidArgument, match="2\\^63"):
            s.push_dev([b, a], [1, (1 << 63) - 5], d_bytes, None, d_st)
        with pytest.raises(InvalidArgument, match="not open"):
            s.close(3)
        # the refused pushes changed nothing: both streams finish with the whole document's record
        got = s.push({a: docs[0][10:], b: docs[1][13:]}, final=[a, b])
        for i, sl in enumerate((a, b)):
            assert got[sl][1] == want_st[i] == 0 and np.array_equal(np.frombuffer(got[sl][0], np.uint8), want[i])
        with pytest.raises(InvalidArgument, match="not open"):           # a final push freed the slot
            s.push({a: b"x"})
    finally:
        s.destroy()


def test_push_dev_odd_addresses_on_a_side_stream(oracle, gpu_ctx, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(5)
    docs = [_prose(rng, 1500 + 2 * i + 1) for i in range(6)]
    want, want_st = _expected(oracle, gpu_ctx, docs, RAW, 5)
    halves = [len(d) // 2 | 1 for d in docs]                 # odd lengths: every chunk but the first starts odd
    s = T.MinHashStreams(8, 5, gpu_ctx)
    side = torch.cuda.Stream()
    try:
        slots = [s.open(RAW) for _ in docs]
        with torch.cuda.stream(side):
            for r in range(2):
                parts = [d[:h] if r == 0 else d[h:] for d, h in zip(docs, halves)]
                buf = torch.from_numpy(np.frombuffer(b"\0" * (1 + r) + b"".join(parts), np.uint8).copy()).cuda()
                d_bytes = buf[1 + r:]
                assert r == 1 or d_bytes.data_ptr() % 2 == 1
                d_out = torch.zeros((len(docs), 1032), dtype=torch.uint8, device="cuda")
                d_st = torch.full((len(docs),), 99, dtype=torch.int32, device="cuda")
                s.push_dev(slots, [len(p) for p in parts], d_bytes, d_out if r else None, d_st,
                           final=slots if r else (), stream=side.cuda_stream)
            side.synchronize()
        assert np.array_equal(d_st.cpu().numpy(), want_st) and np.array_equal(d_out.cpu().numpy(), want)
    finally:
        s.destroy()


SESSION_TEXTS = [
    "The quick brown fox's 3.14 jumps; over_the lazy dog. " * 12,
    "Ünïcode straße İstanbul ΣΊΣΥΦΟΣ ﬁne — Привет, мир! Это тест. 中文文本 和 日本語 テキスト, naïve café. " * 6,
    "plain ascii first: it's a_b and x_y don't 'stop' here 1,5 " * 5 + "then é arrives, Grüße, and ascii again it's a_b " * 5,
]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_session_equals_the_whole_text(gpu_ctx, which):
    text = SESSION_TEXTS[which]
    opts = T.TextOpts()
    want, want_st = T.minhash_batch([text], opts, gpu_ctx)
    assert want_st[0] == 0
    raw = text.encode("utf-8")
    rng = np.random.default_rng(10 + which)
    if which:                       # cuts inside a multi-byte sequence do occur
        assert any(b & 0xC0 == 0x80 for b in raw)
    for trial in range(4):
        sizes = [1, 2, 3] if trial == 0 else [int(v) for v in rng.integers(1, 90, 32)]
        chunks = _cut(raw, sizes)
        if which:
            assert trial or any(c[0] & 0xC0 == 0x80 for c in chunks)
        sess = T.StreamingMinHashSession(opts, 7, 9)
        for c in chunks:
            assert sess.push(c) == []
        (rec,) = sess.finalize()
        assert rec.fingerprint == want[0].tobytes(), (which, trial)
        assert (rec.tenant_id, rec.record_id, rec.algorithm, rec.format_version, rec.text) == \
            (7, 9, T.ALGORITHM_MINHASH_128, T.FORMAT_VERSION_MINHASH_HIP, None)
        for again in (sess.finalize, lambda: sess.push(b"x")):
            with pytest.raises(ModalityError, match="already finalized"):
                again()


def test_session_options_and_bad_input(gpu_ctx):
    text = "No Case Folding Here: Straße stays, ASCII Too. " * 8
    opts = T.TextOpts(canonicalizer=T.Canonicalizer(normalization="nfc", case_fold=False), k=3)
    want, _ = T.minhash_batch([text, "Only ASCII Without Folding, routed by the host. " * 6], opts, gpu_ctx)
    for i, t in enumerate((text, "Only ASCII Without Folding, routed by the host. " * 6)):
        sess = T.StreamingMinHashSession(opts, 1, 2)
        for c in _cut(t.encode(), [7, 31, 2]):
            sess.push(c)
        assert sess.finalize()[0].fingerprint == want[i].tobytes()
    with pytest.raises(UnsupportedError):
        T.StreamingMinHashSession(T.TextOpts(tokenizer="grapheme"), 1, 2)
    for chunks in ([b"abc \xc3"], [b"ok words \xff\xfe more", b" and more"]):       # truncated; invalid
        sess = T.StreamingMinHashSession(T.TextOpts(), 1, 2)
        for c in chunks:
            sess.push(c)
        with pytest.raises(ModalityError, match="UTF-8"):
            sess.finalize()
    with pytest.raises(ModalityError, match="no tokens"):
        T.StreamingMinHashSession(T.TextOpts(), 1, 2).finalize()


def test_ingest_stream_ndjson(gpu_ctx):
    parts = ["The first line of the body, ", "its second line — with an é —", " and the third one it's done."]
    body = "\r\n".join(__import__("json").dumps(p) for p in parts).encode() + b"\n\n"
    rec = T.ingest_stream_ndjson(body, T.TextOpts(), 3, 4)
    ref = T.fingerprint_minhash_with("".join(parts), T.TextOpts(), 3, 4)
    assert (rec.fingerprint, rec.algorithm, rec.config_hash, rec.format_version, rec.tenant_id, rec.record_id) == \
        (ref.fingerprint, ref.algorithm, ref.config_hash, ref.format_version, 3, 4)
