"""UTF-8 MinHash streams (DESIGN.md T7 "UTF-8 streams"; text_stream_kernel<true> in ucfp_amd/csrc/text_streams.hip) on the
GPU.  A RAW_UTF8 stream's final record and status must be those of ucfp_text_minhash_batch(RAW_UTF8) on the whole
document however it is cut -- inside a UTF-8 sequence, between a letter and its MidLetter, inside a Cf run -- so the
expected value is always T._run("minhash", [doc], 2, k) on the concatenation."""
import json

import numpy as np
import pytest

import text_canon_ref as ref
from ucfp_amd import text as T
from ucfp_amd.errors import InvalidArgument, ModalityError, UnsupportedError

pytestmark = pytest.mark.gpu

RAW, PRETOK, UTF8 = 0, 1, 2
NEEDS_HOST, E_MODALITY, E_UNSUPPORTED = 1, -1, -2

# Latin with diacritics, Greek, Cyrillic, Hebrew with ' and " between letters, Arabic, Hiragana, Katakana, Han, Hangul
# syllables, full-width forms, a ligature that expands, soft hyphen and ZERO WIDTH SPACE, and the tokeniser's edge cases
MIXED = ("Ünï Straße l'été x ’e 1,000;2 a:b _a __ Σίσυφος "
         "Привет ש'ל צה\"ל مرحبا "
         "ひらがな カタカナ 漢字中文 한국어 ＡＢ１２ "
         "ﬁne so\u00adft ze\u200bro Ελληνικά Українська 東京タワー d’un œuvre end.")
MIXED2 = ("café א\"ב naïve ｶﾀ 日本語 d'âme ﬃ 3,5 Жук "
          "\u200bx\u00ad y_z \U0001d400b 가나 o’a __")


def _expected(ctx, docs, mode, k):
    """The offline records and statuses of the whole documents, computed once per test."""
    return T._run("minhash", docs, mode, k, ctx)


def _cut(doc, sizes):
    chunks, at, i = [], 0, 0
    while at < len(doc):
        chunks.append(doc[at:at + sizes[i % len(sizes)]])
        at += sizes[i % len(sizes)]
        i += 1
    return chunks or [b""]


def _advance(streams, chunked, modes, history=None):
    """One stream per chunk list, advanced together, one chunk each per push, the last chunk final.
    -> (records [n, 1032], status [n]); history[i] collects stream i's status after every push."""
    if isinstance(modes, int):
        modes = [modes] * len(chunked)
    slots = [streams.open(m) for m in modes]
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


def _check_cuts(ctx, doc, cut_lists, k=5, history=None, want=None):
    """`doc` cut at every list of positions of `cut_lists`, each in its own slot of one set: records and statuses
    equal the offline ones of the whole document."""
    want_rec, want_st = want if want is not None else _expected(ctx, [doc], UTF8, k)
    chunked = [[doc[a:b] for a, b in zip([0] + list(c), list(c) + [len(doc)])] for c in cut_lists]
    s = T.MinHashStreams(len(chunked), k, ctx, utf8=True, max_push_bytes=max(1, len(doc)) * len(chunked))
    try:
        rec, st = _advance(s, chunked, UTF8, history)
    finally:
        s.destroy()
    bad = [i for i in range(len(chunked)) if st[i] != want_st[0] or not np.array_equal(rec[i], want_rec[0])]
    assert not bad, (bad[:8], [cut_lists[i] for i in bad[:8]], st[bad[:8]], want_st[0])
    return want_rec, want_st


@pytest.mark.parametrize("k", [5, 1])
def test_every_two_chunk_cut(gpu_ctx, k):
    """One stream per cut position, all advanced together: two batched pushes in all."""
    doc = MIXED.encode("utf-8")
    assert 230 <= len(doc) <= 270 and ref.canon_bytes(doc)[1] == 0
    for piece in ("l'été", "x ’e", "1,000;2", "a:b", "_a", "__ ", "\u00ad", "\u200b", "ﬁ"):
        assert piece in MIXED
    _, want_st = _check_cuts(gpu_ctx, doc, [[c] for c in range(len(doc) + 1)], k)
    assert want_st[0] == 0


def test_one_byte_chunks(gpu_ctx):
    docs = [MIXED2.encode("utf-8"), MIXED.encode("utf-8")[:150].decode("utf-8", "ignore").encode("utf-8"),
            MIXED.encode("utf-8")[110:].decode("utf-8", "ignore").encode("utf-8"), ("カ" * 24 + "\u200bé:é א'").encode()]
    for d in docs:
        assert 80 <= len(d) <= 150 and ref.canon_bytes(d)[1] == 0
    want, want_st = _expected(gpu_ctx, docs, UTF8, 5)
    s = T.MinHashStreams(len(docs), 5, gpu_ctx, utf8=True, max_push_bytes=64)
    try:
        rec, st = _advance(s, [[d[i:i + 1] for i in range(len(d))] for d in docs], UTF8)
    finally:
        s.destroy()
    assert np.array_equal(st, want_st) and (st == 0).all() and np.array_equal(rec, want)


def test_step_and_batch_edges(gpu_ctx):
    """Chunk sizes around the canon stage's 64-byte step, the hash stage's 256-byte stage and its 1536-byte batch; the
    text puts 2-, 3- and 4-byte sequences across the 64-byte step edges of the chunks."""
    unit = "éa 日\U0001d400 жカ\U0001d7ce büＡ "      # 2-, 3- and 4-byte sequences at a period of 29 bytes
    doc = (unit * 140).encode("utf-8")
    assert len(unit.encode()) == 29 and ref.canon_bytes(doc)[1] == 0
    sizes = list(range(61, 69)) + [127, 128, 129, 130, 191, 192, 193, 1535, 1536, 1537]
    for width in (2, 3, 4):        # a sequence of each width straddles a step edge of the 64-byte chunks
        assert any(doc[e - 1] >= 0xC0 and (4 if doc[e - 1] >= 0xF0 else 3 if doc[e - 1] >= 0xE0 else 2) == width
                   for e in range(64, len(doc), 64))
    _check_cuts(gpu_ctx, doc, [list(range(sz, len(doc), sz)) for sz in sizes])


def test_cf_run_across_a_cut(gpu_ctx):
    """A run of Cf code points longer than a step makes nothing: whatever is cut inside it, `a` still meets `b`, and the
    MidLetter between two runs still joins them."""
    for text in ("a" + "\u200b" * 100 + "b", "a" + "\u200b" * 100 + ":" + "\u200b" * 70 + "b"):
        doc = text.encode("utf-8")
        assert ref.canon_bytes(doc) == (text.replace("\u200b", "").encode(), 0)
        _, want_st = _check_cuts(gpu_ctx, doc, [[c] for c in range(len(doc) + 1)], 1)
        assert want_st[0] == 0


def test_open_segment(gpu_ctx):
    """A segment without an alphanumeric yet waits in the slot's state, up to STREAM_OPEN_SEGMENT_BYTES at a push boundary."""
    assert T.STREAM_OPEN_SEGMENT_BYTES == 256
    for tail in ("a", " x"):
        doc = ("_" * 200 + tail).encode()
        _, want_st = _check_cuts(gpu_ctx, doc, [[c] for c in range(len(doc) + 1)], 1)
        assert want_st[0] == 0
    doc = b"_" * 300 + b"a"
    want = _expected(gpu_ctx, [doc], UTF8, 1)
    assert want[1][0] == 0
    hist = [[], []]
    _check_cuts(gpu_ctx, doc, [[], [250]], 1, hist, want)             # one chunk: any length; 250 bytes pending: under the cap
    assert hist == [[0], [0, 0]]
    s = T.MinHashStreams(1, 1, gpu_ctx, utf8=True, max_push_bytes=512)
    try:
        hist = [[]]
        rec, st = _advance(s, [[doc[:100], doc[100:280], doc[280:290], doc[290:]]], UTF8, hist)
        assert hist == [[0, NEEDS_HOST, NEEDS_HOST, NEEDS_HOST]] and st[0] == NEEDS_HOST and not rec.any()
    finally:
        s.destroy()


HAND_BACKS = [("combining mark", "\u0301".encode()), ("regional indicator", "\U0001F1E6".encode()), ("plane 2", "\U00020000".encode()),
              ("overlong", b"\xe0\x80\xaf"), ("surrogate", b"\xed\xa0\x80"), ("stray continuation", b"\xa9"), ("0xFF", b"\xff")]


@pytest.mark.parametrize("name,bad", HAND_BACKS, ids=[n for n, _ in HAND_BACKS])
def test_hand_backs(gpu_ctx, name, bad):
    """0, then sticky NEEDS_HOST -- never before the offending byte has been pushed; the final status is offline's."""
    head = "ok wörds ".encode()
    doc = head + bad + " more é text".encode()
    want = _expected(gpu_ctx, [doc], UTF8, 5)
    assert want[1][0] == NEEDS_HOST and not want[0].any()
    cuts = [[c] for c in range(len(doc) + 1)]
    hist = [[] for _ in cuts]
    _check_cuts(gpu_ctx, doc, cuts, 5, hist, want)
    for (c,), h in zip(cuts, hist):
        assert h[1] == NEEDS_HOST and h[0] in (0, NEEDS_HOST) and (h[0] == 0 or c > len(head)), (c, h)
    hist = [[]]
    _check_cuts(gpu_ctx, doc, [[4, len(head) + len(bad) + 2, len(doc) - 3]], 5, hist, want)     # sticky over later pushes
    assert hist[0][0] == 0 and hist[0][1:] == [NEEDS_HOST] * 3


def test_truncated_and_completed_sequences(gpu_ctx):
    for doc in ("abc déf 日".encode()[:-1], "abc \U0001d400".encode()[:-2], b"abc \xc3"):
        want = _expected(gpu_ctx, [doc], UTF8, 5)
        assert want[1][0] == NEEDS_HOST
        cuts = [[c] for c in range(len(doc) + 1)]
        hist = [[] for _ in cuts]
        _check_cuts(gpu_ctx, doc, cuts, 5, hist, want)
        assert all(h == [0, NEEDS_HOST] for h in hist[:-1]), hist          # malformed only once the stream ends there
    doc = "café 日本 \U0001d400x".encode()                   # incomplete at a non-final push, then continued: no error
    hist = [[] for _ in range(len(doc) + 1)]
    _, want_st = _check_cuts(gpu_ctx, doc, [[c] for c in range(len(doc) + 1)], 2, hist)
    assert want_st[0] == 0 and all(h == [0, 0] for h in hist)


def test_window_limit_counts_canonical_bytes(gpu_ctx):
    kat = ["カ" * n for n in (93, 93, 93, 94, 94)]                   # 3 canonical bytes each, one token per run
    window = " ".join(kat)
    assert len(window.encode()) == T.MAX_WINDOW_BYTES == 1405
    doc = ("quelques mots d'abord " + window + " et d'autres après x y z").encode()
    _, want_st = _check_cuts(gpu_ctx, doc, [[c] for c in range(700, 764, 3)] + [list(range(400, len(doc), 400))])
    assert want_st[0] == 0
    wide = ("début " + "Ａ" * 1390 + " fin").encode()           # 4170 source bytes for 1390 canonical ones: a 1400-byte window
    assert ref.canon_bytes(wide)[0] == ("début " + "a" * 1390 + " fin").encode()
    _, want_st = _check_cuts(gpu_ctx, wide, [[2000], list(range(500, len(wide), 500)), list(range(1537, len(wide), 1537))])
    assert want_st[0] == 0
    big = ("des mots " + "カ" * 513 + " et le reste du texte " + "mot " * 200).encode()     # a 1539-byte token: over the batch
    want = _expected(gpu_ctx, [big], UTF8, 5)
    assert want[1][0] == E_UNSUPPORTED
    hist = [[]]
    _check_cuts(gpu_ctx, big, [list(range(400, len(big), 400))], 5, hist, want)
    first = hist[0].index(E_UNSUPPORTED)
    assert 0 < first < len(hist[0]) - 1 and set(hist[0][:first]) == {0} and set(hist[0][first:]) == {E_UNSUPPORTED}


def test_mixed_set(gpu_ctx):
    """1024 slots, the three modes mixed in every push, ragged chunks with empty ones; every record is the offline one of
    its own mode; a slot closed and opened again starts clean, whatever mode it had."""
    rng = np.random.default_rng(8)
    N = 1024
    ascii_words = "the quick brown fox it's 3.14 a:b 1,000;2 _a Upper end. stream k9".split()
    utf8_words = MIXED.split() + MIXED2.split()
    pretok_words = [w for w in ref.canon_bytes(MIXED.encode())[0].decode().split()]

    def doc(i):
        words = (ascii_words, pretok_words, utf8_words)[i % 3]
        sep = " " if i % 3 == 1 else ("  " if i % 7 == 0 else " ")
        return sep.join(words[int(v)] for v in rng.integers(0, len(words), 4 + int(rng.integers(0, 24)))).encode("utf-8")

    docs = [doc(i) for i in range(N + 6)]
    modes = [i % 3 for i in range(N + 6)]
    want = np.zeros((N + 6, 1032), np.uint8)
    want_st = np.zeros(N + 6, np.int32)
    for m in (RAW, PRETOK, UTF8):
        idx = [i for i in range(N + 6) if modes[i] == m]
        want[idx], want_st[idx] = _expected(gpu_ctx, [docs[i] for i in idx], m, 5)
    assert (want_st == 0).all()
    s = T.MinHashStreams(N, 5, gpu_ctx, utf8=True, max_push_bytes=1 << 18)
    try:
        slots = [s.open(modes[i]) for i in range(N)]
        doc_of = {sl: i for i, sl in enumerate(slots)}
        at = {sl: 0 for sl in slots}
        done = {}

        def push(sls, finish=()):
            finish = set(finish)
            chunks = {}
            for sl in sls:
                d = docs[doc_of[sl]]
                left = len(d) - at[sl]
                n = left if sl in finish else int(rng.integers(0, min(40, left) + 1)) * int(rng.integers(0, 4) > 0)
                chunks[sl] = d[at[sl]:at[sl] + n]
                at[sl] += n
            got = s.push(chunks, final=finish)
            for sl in finish:
                done[doc_of[sl]] = got[sl]

        order = [int(v) for v in rng.permutation(N)]
        push(order)
        push(order[:700], finish=order[:6])
        for sl in order[6:12]:                                # six are discarded mid-stream, two of each mode
            s.close(sl)
        dropped = {doc_of[sl] for sl in order[6:12]}
        reopened = [s.open(modes[N + j]) for j in range(6)]   # six free slots come back, whatever mode they had before
        assert reopened == sorted(order[:12])[:6]
        for j, sl in enumerate(reopened):
            doc_of[sl], at[sl] = N + j, 0
        live = [sl for sl in order if sl not in set(order[:12])] + reopened
        push(live)
        push(live, finish=live)
        assert sorted(done) == sorted(set(range(N + 6)) - dropped)
        bad = [i for i, (record, status) in done.items()
               if status != want_st[i] or not np.array_equal(np.frombuffer(record, np.uint8), want[i])]
        assert not bad, (bad[:8], [modes[i] for i in bad[:8]])
    finally:
        s.destroy()


def test_creation_and_limits(gpu_ctx, torch_cuda):
    torch = torch_cuda
    lib = T._lib.load()
    assert lib.ucfp_text_streams_state_bytes_ex(0) == lib.ucfp_text_streams_state_bytes() < \
        lib.ucfp_text_streams_state_bytes_ex(T.STREAMS_UTF8)
    with pytest.raises(ModalityError, match=r"shingle k must be in \[1, 64\]"):
        T.MinHashStreams(4, 65, gpu_ctx, utf8=True)
    for mpb in (0, (1 << 28) + 1):
        with pytest.raises(InvalidArgument, match="max_push_bytes"):
            T.MinHashStreams(4, 5, gpu_ctx, utf8=True, max_push_bytes=mpb)
    import ctypes as C
    h = C.c_void_p()
    assert lib.ucfp_text_streams_create_ex(gpu_ctx.handle, 5, 4, 6, 4096, C.byref(h)) == -4 and b"flags" in lib.ucfp_last_error()
    assert lib.ucfp_text_streams_create_ex(gpu_ctx.handle, 5, 4, 0, 0, C.byref(h)) == 0        # no flag: as ucfp_text_streams_create
    plain = T.MinHashStreams.__new__(T.MinHashStreams)
    plain._lib, plain.ctx, plain.handle = lib, gpu_ctx, h
    try:
        with pytest.raises(UnsupportedError, match="RAW_UTF8"):
            plain.open(UTF8)
        assert plain.open(RAW) == 0
    finally:
        plain.destroy()
    docs = ["première chaîne de caractères assez longue pour cinq mots".encode(), "zweite Zeichenkette mit über fünf Wörtern drin".encode(),
            b"plain ascii words that do not count against the limit at all"]
    want, want_st = _expected(gpu_ctx, docs[:2], UTF8, 5)
    want_a, _ = _expected(gpu_ctx, docs[2:], RAW, 5)
    s = T.MinHashStreams(4, 5, gpu_ctx, utf8=True, max_push_bytes=40)
    try:
        a, b, c = s.open(UTF8), s.open(UTF8), s.open(RAW)
        s.push({a: docs[0][:20], b: docs[1][:20], c: docs[2][:30]})            # 40 RAW_UTF8 bytes: the ASCII stream's do not count
        with pytest.raises(InvalidArgument, match="max_push_bytes"):
            s.push({a: docs[0][20:41], b: docs[1][20:40]})
        d_bytes = torch.zeros(64, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(4, dtype=torch.int32, device="cuda")
        with pytest.raises(InvalidArgument, match="max_push_bytes"):
            s.push_dev([a], [1 << 40], d_bytes, None, d_st)
        with pytest.raises(InvalidArgument, match="twice"):
            s.push_dev([a, a], [1, 1], d_bytes, None, d_st)
        with pytest.raises(InvalidArgument, match="unknown text mode"):
            s.open(3)
        # the refused pushes changed nothing
        s.push({a: docs[0][20:60], c: docs[2][30:]})
        s.push({b: docs[1][20:60]})
        got = s.push({a: docs[0][60:], b: docs[1][60:], c: b""}, final=[a, b, c])
        for i, sl in enumerate((a, b)):
            assert got[sl][1] == want_st[i] == 0 and np.array_equal(np.frombuffer(got[sl][0], np.uint8), want[i])
        assert got[c][1] == 0 and np.array_equal(np.frombuffer(got[c][0], np.uint8), want_a[0])
    finally:
        s.destroy()


def test_session_routes(gpu_ctx):
    kana = "あいうえおカタカナ漢字、日本語の文章です。ＡＢ"
    text = (kana * 40)[:683]                                    # 3 bytes each: 2 KiB, no ASCII whitespace anywhere
    raw = text.encode("utf-8")
    assert 2000 <= len(raw) <= 2100 and not any(ch in text for ch in " \n\t\r")
    want, want_st = T.minhash_batch([text], T.TextOpts(), gpu_ctx)
    assert want_st[0] == 0
    sess = T.StreamingMinHashSession(T.TextOpts(), 7, 9)
    assert sess.route == "ascii"
    for c in _cut(raw, [7, 31, 2]):
        assert sess.push(c) == []
        assert sess.route == "utf8" and sess._tail == ""        # nothing waits on the host for whitespace
    (rec,) = sess.finalize()
    assert sess.route == "utf8" and rec.fingerprint == want[0].tobytes()
    marked = "ascii first, then cafe\u0301 with a combining mark, " * 6 + "and the end"
    want, want_st = T.minhash_batch([marked], T.TextOpts(), gpu_ctx)
    sess = T.StreamingMinHashSession(T.TextOpts(), 7, 9)
    for c in _cut(marked.encode("utf-8"), [7, 31, 2]):
        sess.push(c)
    (rec,) = sess.finalize()
    assert sess.route == "host" and want_st[0] == 0 and rec.fingerprint == want[0].tobytes()
    sess = T.StreamingMinHashSession(T.TextOpts(canonicalizer=T.Canonicalizer(normalization="nfc")), 7, 9)
    sess.push("café ".encode())
    assert sess.route == "host"                                 # another canonicaliser: never the device's
    sess.finalize()
    with pytest.raises(ModalityError, match="UTF-8"):
        bad = T.StreamingMinHashSession(T.TextOpts(), 7, 9)
        bad.push("début 日".encode()[:-1])
        assert bad.route == "utf8"
        bad.finalize()
    parts = ["最初の行、", "二行目は café を含み", "、三行目で終わり it's done."]
    body = "\r\n".join(json.dumps(p, ensure_ascii=(i == 1)) for i, p in enumerate(parts)).encode("utf-8") + b"\n\n"
    got = T.ingest_stream_ndjson(body, T.TextOpts(), 3, 4)
    assert got.fingerprint == T.fingerprint_minhash_with("".join(parts), T.TextOpts(), 3, 4).fingerprint


def test_dense_steps(gpu_ctx):
    """Steps that make more than 64 and more than 128 canonical code points (text_canon_ref.dense_*: canon_decide's second
    and third round, with the segment state of a slot carried into them), cut at every position and around the step.
    The expected records are the PRETOKENIZED hash of the restatement's tokens, not the offline kernel's, which runs the
    same rounds."""
    def want(doc, k):
        toks, st = ref.canon_bytes(doc)
        assert st == 0
        return T._run("minhash", [toks], PRETOK, k, gpu_ctx)

    dense, quiet = chr(ref.expanders()[0]).encode(), chr(ref.quiet_expander()).encode()
    every = [dense * 44, quiet * 22 + b"_" * 70 + b"a"]        # three rounds in a step; a segment kept across two steps
    assert [max(i for _, i, *_ in ref.decide_map(d)) >= n for d, n in zip(every, (128, 64))] == [True, True]
    for doc in every:
        _, want_st = _check_cuts(gpu_ctx, doc, [[c] for c in range(len(doc) + 1)], 2, want=want(doc, 2))
        assert want_st[0] == 0
    docs = [chr(cp).encode() * 100 for cp in ref.expanders()] + ref.dense_mixed(12) + ref.dense_dots()[-4:]
    docs += [d for d in ref.dense_open_segments(1) if len(d) == 3 * 22 + 1 + 70 + 1][:2]
    docs += [d for d in ref.dense_open_segments(2) if d.startswith(dense * 10 + b"_" * 70)]      # a token's `_` tail fills a round
    assert len(docs) == 6 + 12 + 4 + 2 + 3
    for doc in docs:
        _check_cuts(gpu_ctx, doc, [list(range(sz, len(doc), sz)) for sz in range(61, 69)], want=want(doc, 5))
