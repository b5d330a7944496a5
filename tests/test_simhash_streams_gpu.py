"""Streaming SimHash, TF and TF.IDF (text_stream_kernel<.., T_SIM / T_IDF> in
ucfp_amd/csrc/text_streams.hip) on the GPU.  A stream's final record and status must be those of the whole document,
however it is cut.  Expected values never come from the code under test: TF records are the CPU oracle's
text_simhash_batch, weighted records and every RAW_UTF8 record are simhash_idf_ref's (tests/simhash_streams_fixtures.py),
and the offline GPU entry is asserted equal to them too."""
import ctypes as C
import json

import numpy as np
import pytest

import simhash_idf_ref as iref
import simhash_streams_fixtures as F
from simhash_streams_fixtures import E_MODALITY, E_UNSUPPORTED, NEEDS_HOST, PRETOK, RAW, UTF8
from ucfp_amd import text as T
from ucfp_amd.errors import InvalidArgument, UnsupportedError

pytestmark = pytest.mark.gpu

KINDS = ["tf", "idf"]


def _table(ctx, weights, default):
    keys = np.array(list(weights), np.uint64)
    wts = np.array([weights[int(k)] for k in keys], np.uint32)
    return T.IdfTable(ctx=ctx, capacity_hint=max(16, len(weights)))._set_q16(keys, wts, default)


class Case:
    """TF (weights None) or weighted: the expected records of whole documents and the stream sets that must give them."""

    def __init__(self, oracle, ctx, weights=None, default=F.Q16_ONE):
        self.oracle, self.ctx, self.weights, self.default = oracle, ctx, weights, default
        self.table = _table(ctx, weights, default) if weights is not None else None

    @classmethod
    def of(cls, kind, oracle, ctx, docs, mode=RAW, **kw):
        """kind "tf", or "idf" with a table that weights about 70 % of the documents' tokens."""
        if kind == "tf":
            return cls(oracle, ctx)
        toks = [iref.words(d, mode) for d in docs]
        weights, default = F.weights_for(toks, **kw)
        return cls(oracle, ctx, weights, default)

    def expected(self, docs, mode):
        """The reference's records and statuses of the whole documents; the offline GPU entry agrees."""
        if self.weights is None:
            rec, st = F.expected_tf(self.oracle, docs, mode)
            grec, gst = T._run("simhash", docs, mode, 5, self.ctx)
        else:
            rec, st = F.expected_ref(docs, mode, self.weights, self.default)
            grec, gst = self.table._simhash_docs(self.ctx, docs, mode, T.TOK_WORD)
        assert np.array_equal(gst, st) and np.array_equal(grec, rec)
        return rec, st

    def streams(self, n, **kw):
        s = T.SimHashStreams(n, self.ctx, idf=self.table, **kw)
        assert s.record_bytes == 8 and (s.idf is self.table)
        return s

    def close(self):
        if self.table is not None:
            self.table.close()


def _advance(streams, chunked, modes, history=None):
    """One stream per chunk list, advanced together, one chunk each per push, the last chunk final.
    -> (records [n, 8] uint8, status [n]).  `history[i]` collects stream i's status after every push."""
    if isinstance(modes, int):
        modes = [modes] * len(chunked)
    slots = [streams.open(m) for m in modes]
    assert len(set(slots)) == len(slots)
    rec = np.zeros((len(chunked), 8), np.uint8)
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
                assert len(record) == 8
                rec[i] = np.frombuffer(record, np.uint8)
                st[i] = status
    return rec, st


def _check(case, streams, docs, chunked, modes, history=None):
    for d, c in zip(docs, chunked):
        assert b"".join(c) == d
    if isinstance(modes, int):
        want, want_st = case.expected(docs, modes)
    else:
        want, want_st = np.zeros((len(docs), 8), np.uint8), np.zeros(len(docs), np.int32)
        for m in sorted(set(modes)):
            idx = [i for i in range(len(docs)) if modes[i] == m]
            want[idx], want_st[idx] = case.expected([docs[i] for i in idx], m)
    rec, st = _advance(streams, chunked, modes, history)
    bad = [i for i in range(len(docs)) if st[i] != want_st[i] or not np.array_equal(rec[i], want[i])]
    assert not bad, (bad[:8], st[bad[:8]], want_st[bad[:8]])
    return want, want_st


@pytest.mark.parametrize("kind", KINDS)
def test_every_two_chunk_cut(oracle, gpu_ctx, kind):
    """One stream per cut position, all advanced together: a token ends exactly at a push boundary and the held-back byte
    decides."""
    doc = F.EDGE_DOC
    cuts = list(range(len(doc) + 1))
    case = Case.of(kind, oracle, gpu_ctx, [doc])
    s = case.streams(len(cuts))
    try:
        _, want_st = _check(case, s, [doc] * len(cuts), [[doc[:c], doc[c:]] for c in cuts], RAW)
        assert (want_st == 0).all()
    finally:
        s.destroy()
        case.close()


@pytest.mark.parametrize("kind", KINDS)
def test_one_byte_chunks(oracle, gpu_ctx, kind):
    """Every token is carried unfinished through many pushes."""
    rng = np.random.default_rng(1)
    docs = [F.prose(rng, 280 + int(rng.integers(0, 40))) for _ in range(64)]
    assert len(set(docs)) == 64
    case = Case.of(kind, oracle, gpu_ctx, docs)
    s = case.streams(64)
    try:
        _check(case, s, docs, [[d[i:i + 1] for i in range(len(d))] for d in docs], RAW)
    finally:
        s.destroy()
        case.close()


@pytest.mark.parametrize("kind", KINDS)
def test_state_carried_across_lds_flushes(oracle, gpu_ctx, kind):
    """8 KiB documents of more than 256 tokens (several LDS batches each; tests/test_simhash_streams_spec.py) at chunk sizes
    around the 64-byte step, the 256-byte stage and the 1536-byte batch, with empty pushes in between; one 1000-byte
    token that spans four pushes."""
    docs, chunked = F.flush_docs()
    case = Case.of(kind, oracle, gpu_ctx, docs)
    s = case.streams(len(docs))
    try:
        _, want_st = _check(case, s, docs, chunked, RAW)
        assert (want_st == 0).all()
    finally:
        s.destroy()
        case.close()


def test_ties_zero_weights_and_wide_sums(oracle, gpu_ctx):
    # two distinct tokens, each once: every bit where the keys differ is a tie and clears (the spec test: they do differ)
    tf = Case(oracle, gpu_ctx)
    s = tf.streams(2)
    try:
        want, _ = _check(tf, s, [F.TIE_DOC, F.TIE_DOC], [[b"alp", b"ha be", b"ta"], [b"alpha", b" ", b"beta"]], RAW)
        a, b = (iref.key(t) for t in iref.words(F.TIE_DOC, RAW))
        assert int.from_bytes(want[0].tobytes(), "little") == a & b and a != b
    finally:
        s.destroy()
    # every token weighs 0: UCFP_E_MODALITY, on the final entry only
    zero = Case(oracle, gpu_ctx, *F.ZERO_WEIGHTS)
    s = zero.streams(1)
    try:
        hist = [[]]
        want, want_st = _check(zero, s, [F.ZERO_DOC], [[F.ZERO_DOC[:7], F.ZERO_DOC[7:20], F.ZERO_DOC[20:]]], RAW, hist)
        assert hist == [[0, 0, E_MODALITY]] and want_st[0] == E_MODALITY and not want.any()
    finally:
        s.destroy()
        zero.close()
    # weights of 0xFFFFFFFF over a few thousand tokens and many pushes: pos and tot pass 2^32 between pushes (the spec
    # test), so both halves make the round trip through the state; equal non-zero weights give the TF record
    wide = F.wide_doc()
    heavy = Case.of("idf", oracle, gpu_ctx, [wide], share=1.0, heavy=True)
    s = heavy.streams(3)
    try:
        chunked = [F.cut(wide, [97]), F.cut(wide, [1]  * 40 + [4000]), F.cut(wide, [1537])]
        assert len(chunked[0]) > 100
        want, want_st = _check(heavy, s, [wide] * 3, chunked, RAW)
        tf_rec, tf_st = tf.expected([wide], RAW)
        assert want_st[0] == tf_st[0] == 0 and np.array_equal(want[0], tf_rec[0])
    finally:
        s.destroy()
        heavy.close()
    toks = iref.words(F.EDGE_DOC, RAW)
    equal = Case(oracle, gpu_ctx, {iref.key(t): 3 * F.Q16_ONE for t in toks[::2]}, 3 * F.Q16_ONE)   # table and default agree
    s = equal.streams(1)
    try:
        want, _ = _check(equal, s, [F.EDGE_DOC], [F.cut(F.EDGE_DOC, [17])], RAW)
        assert np.array_equal(want, tf.expected([F.EDGE_DOC], RAW)[0])
    finally:
        s.destroy()
        equal.close()


@pytest.mark.parametrize("kind", KINDS)
def test_window_limit(oracle, gpu_ctx, kind):
    """The window of a SimHash stream is the single token: 1405 canonical bytes always hash, more than the 1536-byte batch
    never does (sticky UCFP_E_UNSUPPORTED, zero record), between the two: status 0 and the exact record, or a nonzero
    status and a zero record."""
    docs = F.window_docs()
    case = Case.of(kind, oracle, gpu_ctx, list(docs.values()))
    try:
        ok = docs["ok"]
        cuts = list(range(700, 764))
        s = case.streams(64)
        try:
            _, want_st = _check(case, s, [ok] * 64, [[ok[:c], ok[c:]] for c in cuts], RAW)
            assert (want_st == 0).all()
        finally:
            s.destroy()
        big = docs["over"]
        off_st = (T._run("simhash", [big], RAW, 5, gpu_ctx) if case.table is None
                  else case.table._simhash_docs(gpu_ctx, [big], RAW, T.TOK_WORD))[1]
        assert off_st[0] == E_UNSUPPORTED
        hist = [[]]
        s = case.streams(1)
        try:
            rec, st = _advance(s, [F.cut(big, [400])], RAW, hist)         # the token spans pushes
            assert st[0] == E_UNSUPPORTED and not rec.any()
            first = hist[0].index(E_UNSUPPORTED)
            assert 0 < first < len(hist[0]) - 1 and set(hist[0][:first]) == {0} and set(hist[0][first:]) == {E_UNSUPPORTED}
        finally:
            s.destroy()
        between = [docs["between_lo"], docs["between_hi"]]
        exact = F.expected_tf(oracle, between, RAW) if case.weights is None else F.expected_ref(between, RAW, case.weights, case.default)
        assert (exact[1] == 0).all()
        s = case.streams(4)
        try:
            rec, st = _advance(s, [F.cut(d, sizes) for d in between for sizes in ([400], [5000])], RAW)
            for i in range(4):
                assert (st[i] == 0 and np.array_equal(rec[i], exact[0][i // 2])) or (st[i] != 0 and not rec[i].any()), (i, st[i])
        finally:
            s.destroy()
    finally:
        case.close()


def test_needs_host_is_sticky_and_wins(oracle, gpu_ctx):
    """A byte >= 0x80 in a RAW_ASCII stream, the held-back byte included; later pushes change nothing; NEEDS_HOST wins over
    the UCFP_E_MODALITY a stream of zero-weight tokens would end in."""
    docs = [b"plain ascii words caf\xc3\xa9 and more words after it to the very end",
            b"the high byte is the last of its chunk\xe9 and the text goes on and on",
            b"nil nada \xe9 zero nothing at all"]
    chunked = [[d[:12], d[12:30], d[30:45], d[45:]] for d in docs[:1]] + [[d[:20], d[20:39], d[39:50], d[50:]] for d in docs[1:2]] + \
              [[docs[2][:5], docs[2][5:12], docs[2][12:20], docs[2][20:]]]
    for c in chunked:
        assert max(c[0]) < 0x80 and max(c[1]) >= 0x80
    assert chunked[1][1][-1] == 0xe9        # held back by push 2, yet seen by it
    for case in (Case(oracle, gpu_ctx), Case(oracle, gpu_ctx, *F.ZERO_WEIGHTS)):
        hist = [[], [], []]
        s = case.streams(3)
        try:
            want, want_st = _check(case, s, docs, chunked, RAW, hist)
            assert list(want_st) == [NEEDS_HOST] * 3 and not want.any()
            assert hist == [[0, NEEDS_HOST, NEEDS_HOST, NEEDS_HOST]] * 3
        finally:
            s.destroy()
            case.close()


@pytest.mark.parametrize("kind", KINDS)
def test_pretokenized_and_utf8_streams(oracle, gpu_ctx, kind):
    pre = [b"ab\x00cd e\x00 \x00 f g h i", b"a  b   c    d e  f", b"tok1 tok2 tok3 tok4 tok5 tok6", b"\xc3\xa9t\xc3\xa9 \xe4\xb8\xad \xe6\x96\x87 a b c"]
    pre_chunks = [[b"ab\x00", b"cd e\x00 \x00", b" f g h i"], [b"a  b ", b"  c ", b"   d e", b"  f"],
                  [b"tok1 tok2 ", b"tok3 tok4", b" tok5 tok6"], [b"\xc3", b"\xa9t\xc3\xa9 \xe4\xb8", b"\xad \xe6\x96\x87 a b c"]]
    mixed = F.MIXED.encode("utf-8")
    for piece in ("l'été", "x ’e", "a:b", "\u00ad", "\u200b", "ﬁ", "カタカナ", "漢字"):
        assert piece in F.MIXED
    case = Case.of(kind, oracle, gpu_ctx, [mixed], UTF8)       # PRETOKENIZED tokens that are not in the table weigh the default
    try:
        s = case.streams(len(pre))
        try:
            _, want_st = _check(case, s, pre, pre_chunks, PRETOK)
            assert (want_st == 0).all()
        finally:
            s.destroy()
        # every two-chunk cut of mixed-script text: inside a UTF-8 sequence, between a letter and a MidLetter, ...
        cuts = list(range(len(mixed) + 1))
        assert any(mixed[c] & 0xC0 == 0x80 for c in cuts[:-1]) and mixed[mixed.index(b"l'") + 1:][:1] == b"'"
        s = case.streams(len(cuts), utf8=True, max_push_bytes=len(mixed) * len(cuts))
        try:
            _, want_st = _check(case, s, [mixed] * len(cuts), [[mixed[:c], mixed[c:]] for c in cuts], UTF8)
            assert (want_st == 0).all()
        finally:
            s.destroy()
        # a hand-back (a combining mark), and the three modes mixed in every push of one UTF-8 set
        marked = "ok wörds and some more plain words before the cafe\u0301 arrives, more é text".encode("utf-8")
        rng = np.random.default_rng(7)
        words = {RAW: "the quick brown fox it's 3.14 a:b 1,000;2 _a Upper end.".split(), UTF8: F.MIXED.split(),
                 PRETOK: iref.words(mixed, UTF8)}
        docs, modes = [marked], [UTF8]
        for i in range(30):
            m = i % 3
            w = words[m]
            picked = [w[int(v)] for v in rng.integers(0, len(w), 5 + int(rng.integers(0, 20)))]
            docs.append(b" ".join(picked) if m == PRETOK else " ".join(picked).encode("utf-8"))
            modes.append(m)
        chunked = [F.cut(d, [int(v) for v in rng.integers(1, 23, 8)]) for d in docs]
        hist = [[] for _ in docs]
        s = case.streams(len(docs), utf8=True, max_push_bytes=1 << 16)
        try:
            want, want_st = _check(case, s, docs, chunked, modes, hist)
            assert want_st[0] == NEEDS_HOST and not want[0].any() and (want_st[1:] == 0).all()
            first = hist[0].index(NEEDS_HOST)
            assert hist[0][0] == 0 and set(hist[0][first:]) == {NEEDS_HOST} and set(hist[0][:first]) == {0}
        finally:
            s.destroy()
    finally:
        case.close()


@pytest.mark.parametrize("kind", KINDS)
def test_slot_reuse(oracle, gpu_ctx, kind):
    """A slot that ended, or was closed, with non-zero counters and an unfinished token gives, reopened, the record of its
    new document alone."""
    old = [F.wide_doc()[:3000] + b" unfinishedtok", F.EDGE_DOC + b" tail"]
    new = [b"fresh words only here", b"another new document x.y 3,5"]
    case = Case.of(kind, oracle, gpu_ctx, old + new, share=1.0, heavy=(kind == "idf"))
    s = case.streams(2)
    try:
        a, b = s.open(RAW), s.open(RAW)
        s.push({a: old[0], b: old[1][:50]})
        got = s.push({b: old[1][50:]}, final=[b])                                   # b ends, a is closed mid-token
        want, want_st = case.expected([old[1]] + new, RAW)
        assert got[b][1] == 0 and got[b][0] == want[0].tobytes() and want[0].any()
        s.close(a)
        assert sorted([s.open(RAW), s.open(RAW)]) == sorted([a, b])
        got = s.push({a: new[0][:7], b: new[1][:9]})
        got = s.push({a: new[0][7:], b: new[1][9:]}, final=[a, b])
        for i, sl in enumerate((a, b)):
            assert got[sl][1] == want_st[1 + i] == 0 and got[sl][0] == want[1 + i].tobytes()
    finally:
        s.destroy()
        case.close()


@pytest.mark.parametrize("kind", KINDS)
def test_many_streams(oracle, gpu_ctx, kind):
    """1024 streams of random lengths and random cuttings in one set, ragged pushes with empty chunks among them."""
    rng = np.random.default_rng(4)
    N = 1024
    docs = [F.prose(rng, 40 + int(rng.integers(0, 120))) for _ in range(N)]
    chunked = []
    for d in docs:
        sizes = [int(v) for v in rng.integers(0, 60, 1 + int(rng.integers(0, 5)))]
        c, at = [], 0
        for n in sizes:
            c.append(d[at:at + n])
            at += n
        c.append(d[at:])
        chunked.append(c)
    case = Case.of(kind, oracle, gpu_ctx, docs)
    s = case.streams(N)
    try:
        _check(case, s, docs, chunked, RAW)
        assert s.open(RAW) == 0                               # every final freed its slot
    finally:
        s.destroy()
        case.close()


def test_push_dev_odd_addresses_on_a_side_stream(oracle, gpu_ctx, torch_cuda):
    """d_out has stride 8; the rows of non-final entries stay untouched."""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    docs = [F.prose(rng, 1500 + 2 * i + 1) for i in range(6)]
    case = Case.of("idf", oracle, gpu_ctx, docs)
    want, want_st = case.expected(docs, RAW)
    halves = [len(d) // 2 | 1 for d in docs]                 # odd lengths: every chunk but the first starts odd
    s = case.streams(8)
    side = torch.cuda.Stream()
    try:
        slots = [s.open(RAW) for _ in docs]
        first = slots[::2]                                   # these end in round 1, the others in round 2
        outs = []
        with torch.cuda.stream(side):
            for r in range(3):
                parts = [(d[:h], d[h:], b"")[r] for d, h in zip(docs, halves)]
                live = [i for i in range(len(docs)) if r < 2 or slots[i] not in first]
                buf = torch.from_numpy(np.frombuffer(b"\0" * (1 + r) + b"".join(parts[i] for i in live), np.uint8).copy()).cuda()
                d_bytes = buf[1 + r:]
                assert r != 0 or d_bytes.data_ptr() % 2 == 1
                d_out = torch.full((len(live), 8), 0xAB, dtype=torch.uint8, device="cuda")
                d_st = torch.full((len(live),), 99, dtype=torch.int32, device="cuda")
                fin = () if r == 0 else first if r == 1 else [slots[i] for i in live]
                s.push_dev([slots[i] for i in live], [len(parts[i]) for i in live], d_bytes, d_out if r else None, d_st,
                           final=fin, stream=side.cuda_stream)
                outs.append((live, d_out, d_st))
            side.synchronize()
        live, d_out, d_st = outs[1]
        out, st = d_out.cpu().numpy(), d_st.cpu().numpy()
        assert (st == 0).all()
        for row, i in enumerate(live):
            assert np.array_equal(out[row], want[i]) if slots[i] in first else (out[row] == 0xAB).all(), i
        live, d_out, d_st = outs[2]
        assert live == [1, 3, 5] and np.array_equal(d_out.cpu().numpy(), want[live]) and np.array_equal(d_st.cpu().numpy(), want_st[live])
        assert (outs[0][1].cpu().numpy() == 0xAB).all()
    finally:
        s.destroy()
        case.close()


def test_errors(oracle, gpu_ctx, torch_cuda):
    torch = torch_cuda
    lib = T._lib.load()
    docs = [b"alpha beta gamma delta epsilon zeta eta theta", b"one two three four five six seven eight nine"]
    d_bytes = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(4, dtype=torch.int32, device="cuda")
    # a table that is not final at a push: refused; after finalize the same push succeeds and the record is right
    table = T.IdfTable(ctx=gpu_ctx)
    assert (table.add([d.decode() for d in docs] + ["alpha one alpha"]) == 0).all() and not table.is_final and table
    n_docs, dfs = iref.fit([iref.words(d, RAW) for d in docs] + [[b"alpha", b"one", b"alpha"]])
    weights, default = iref.weights_of(n_docs, dfs)
    want, want_st = F.expected_ref(docs, RAW, weights, default)
    s = T.SimHashStreams(4, gpu_ctx, idf=table)
    try:
        a, b = s.open(RAW), s.open(RAW)
        with pytest.raises(InvalidArgument, match="not final"):
            s.push({a: docs[0][:10], b: docs[1][:13]})
        table.finalize()
        s.push({a: docs[0][:10], b: docs[1][:13]})
        # the byte limit, checked before anything is launched (d_bytes is NULL: a wrong limit could not read out of bounds)
        limit = T.SIMHASH_STREAM_LIMIT_BYTES
        for sl, pushed in ((a, 10), (b, 13)):
            with pytest.raises(InvalidArgument, match=r"2\^30 bytes.*UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES"):
                s.push_dev([sl], [limit], None, None, d_st)
            with pytest.raises(InvalidArgument, match=r"2\^30 bytes"):
                s.push_dev([sl], [limit - pushed], None, None, d_st)
            with pytest.raises(InvalidArgument, match="d_bytes is NULL"):
                s.push_dev([sl], [limit - pushed - 1], None, None, d_st)
        one_slot, one_count = np.array([a], np.uint32), np.array([limit], np.uint64)
        assert lib.ucfp_text_streams_push_dev(s.handle, one_slot.ctypes.data, one_count.ctypes.data, None, 1, None, None,
                                              d_st.data_ptr(), None) == -4
        assert b"2^30" in lib.ucfp_last_error()
        for bad, why in (([a, 4], "out of range"), ([a, 3], "not open"), ([b, a, b], "twice")):
            with pytest.raises(InvalidArgument, match=why):
                s.push_dev(bad, [1] * len(bad), d_bytes, None, d_st)
        with pytest.raises(UnsupportedError, match="RAW_UTF8"):
            s.open(UTF8)
        with pytest.raises(InvalidArgument, match="unknown text mode"):
            s.open(7)
        # the table loses its weights in the middle of the streams: the push is refused and changes nothing
        table.add(["alpha"])
        assert not table.is_final
        with pytest.raises(InvalidArgument, match="not final"):
            s.push({a: docs[0][10:], b: docs[1][13:]}, final=[a, b])
        keys = np.array(list(weights), np.uint64)
        table._set_q16(keys, np.array([weights[int(k)] for k in keys], np.uint32), default)     # the weights it had
        got = s.push({a: docs[0][10:], b: docs[1][13:]}, final=[a, b])
        for i, sl in enumerate((a, b)):
            assert got[sl][1] == want_st[i] == 0 and np.array_equal(np.frombuffer(got[sl][0], np.uint8), want[i])
        with pytest.raises(InvalidArgument, match="not open"):           # a final push freed the slot
            s.push({a: b"x"})
        assert lib.ucfp_text_streams_record_bytes(s.handle) == 8
    finally:
        s.destroy()
        table.close()
    h = C.c_void_p()
    assert lib.ucfp_text_streams_create_sim(gpu_ctx.handle, 4, 6, 4096, None, C.byref(h)) == -4 and b"flags" in lib.ucfp_last_error()
    for mpb in (0, (1 << 28) + 1):
        with pytest.raises(InvalidArgument, match="max_push_bytes"):
            T.SimHashStreams(4, gpu_ctx, utf8=True, max_push_bytes=mpb)
    with pytest.raises(UnsupportedError, match="IdfTable"):
        T.SimHashStreams(4, gpu_ctx, idf={"a": 1.0})
    m = T.MinHashStreams(2, 5, gpu_ctx)
    try:
        assert lib.ucfp_text_streams_record_bytes(m.handle) == 1032 == m.record_bytes
    finally:
        m.destroy()


SESSION_TEXTS = [
    ("ascii", "The quick brown fox's 3.14 jumps; over_the lazy dog. " * 12),
    ("utf8", "Ünï Straße l'été naïve café, Grüße aus Köln: Σίσυφος Привет мир. " * 6),
    ("utf8", "あいうえおカタカナ漢字、日本語の文章です。ＡＢ 漢字中文 東京タワー " * 8),
    ("host", "ascii first, then cafe\u0301 with a combining mark, " * 6 + "and the end"),
]


@pytest.mark.parametrize("which", range(len(SESSION_TEXTS)))
def test_session_equals_the_whole_text(gpu_ctx, which):
    route, text = SESSION_TEXTS[which]
    opts = T.TextOpts()
    raw = text.encode("utf-8")
    rng = np.random.default_rng(20 + which)
    table = T.IdfTable(ctx=gpu_ctx).fit([t for _, t in SESSION_TEXTS] + ["the fox and the dog", "café straße 日本語"])
    try:
        for idf, algorithm, whole in ((None, T.ALGORITHM_SIMHASH_TF, T.fingerprint_simhash_tf(text, opts, 7, 9)),
                                      (table, T.ALGORITHM_SIMHASH_IDF, T.fingerprint_simhash_idf(text, opts, table, 7, 9)),
                                      (None, T.ALGORITHM_SIMHASH_IDF, T.fingerprint_simhash_idf(text, opts, None, 7, 9))):
            for trial in range(3):
                sizes = [1, 2, 3] if trial == 0 else [int(v) for v in rng.integers(1, 90, 32)]
                sess = T.StreamingSimHashSession(opts, 7, 9, idf=idf, algorithm=algorithm)
                for c in F.cut(raw, sizes):
                    assert sess.push(c) == []
                (rec,) = sess.finalize()
                assert sess.route == route, (which, trial)
                assert (rec.fingerprint, rec.algorithm, rec.format_version, rec.config_hash) == \
                    (whole.fingerprint, whole.algorithm, whole.format_version, whole.config_hash), (which, trial, algorithm)
                assert (rec.tenant_id, rec.record_id, rec.text, len(rec.fingerprint)) == (7, 9, None, 8)
    finally:
        table.close()


def test_session_options_and_ingest(gpu_ctx):
    with pytest.raises(UnsupportedError):
        T.StreamingSimHashSession(T.TextOpts(tokenizer="grapheme"), 1, 2)
    with pytest.raises(UnsupportedError, match="IdfTable"):
        T.StreamingSimHashSession(T.TextOpts(), 1, 2, idf={"a": 1.0}, algorithm=T.ALGORITHM_SIMHASH_IDF)
    with pytest.raises(UnsupportedError):
        T.StreamingSimHashSession(T.TextOpts(), 1, 2, algorithm=T.ALGORITHM_MINHASH_128)
    text = "No Case Folding Here: Straße stays, ASCII Too. " * 8
    opts = T.TextOpts(canonicalizer=T.Canonicalizer(normalization="nfc", case_fold=False))
    sess = T.StreamingSimHashSession(opts, 1, 2)
    for c in F.cut(text.encode(), [7, 31, 2]):
        sess.push(c)
    assert sess.finalize()[0].fingerprint == T.fingerprint_simhash_tf(text, opts, 1, 2).fingerprint and sess.route == "host"
    parts = ["The first line of the body, ", "its second line — with an é —", " and the third one it's done."]
    body = "\r\n".join(json.dumps(p) for p in parts).encode() + b"\n\n"
    for algorithm, ref in (("simhash-tf", T.fingerprint_simhash_tf("".join(parts), T.TextOpts(), 3, 4)),
                           ("simhash-idf", T.fingerprint_simhash_idf("".join(parts), T.TextOpts(), None, 3, 4)),
                           (None, T.fingerprint_minhash_with("".join(parts), T.TextOpts(), 3, 4))):
        rec = T.ingest_stream_ndjson(body, T.TextOpts(), 3, 4, algorithm=algorithm)
        assert (rec.fingerprint, rec.algorithm, rec.config_hash, rec.format_version, rec.tenant_id, rec.record_id) == \
            (ref.fingerprint, ref.algorithm, ref.config_hash, ref.format_version, 3, 4), algorithm
    assert len(T.ingest_stream_ndjson(body, T.TextOpts(), 3, 4).fingerprint) == 1032          # today's call, today's record
    with pytest.raises(UnsupportedError):
        T.ingest_stream_ndjson(body, T.TextOpts(), 3, 4, algorithm="tlsh")
