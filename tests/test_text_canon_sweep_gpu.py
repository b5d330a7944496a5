"""GPU: the UTF-8 canonicaliser (ucfp_amd/csrc/text_canon_core.h: canon_place, canon_decide) over input spaces small enough
to enumerate -- every code point through the device's own table walk, every UTF-8 form of two, three and four bytes,
every sequence at every lane of two steps, and steps that make more than 64 and more than 128 canonical code points.
Well-formedness is Python's strict decoder; everything else is the restatement tests/text_canon_ref.py, which
test_text_canon_spec.py pins to `unicodedata` and `regex` for every code point.  Token blobs byte for byte, statuses equal."""
import functools
import time

import numpy as np
import pytest

import text_canon_ref as ref

pytestmark = pytest.mark.gpu

BLOCK = 0x2000
N_SCALARS, N_SURROGATES = 0x110000 - 0x800, 0x800


def _strict(doc: bytes) -> bool:
    try:
        doc.decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def _rows(a: np.ndarray):
    """The rows of a uint8 matrix that has no row ending in 0x00, as bytes objects."""
    a = np.ascontiguousarray(a, np.uint8)
    assert a[:, -1].all()
    return a.view("S%d" % a.shape[1]).ravel().tolist()


def _compare(docs, want, name):
    """canon_batch(docs) against [(tokens, status)]; prints the two times the summary of a sweep quotes."""
    from ucfp_amd import text
    t0 = time.perf_counter()
    toks, st = text.canon_batch(docs)
    t1 = time.perf_counter()
    print(f"{name}: {len(docs)} documents, canon_batch {1e3 * (t1 - t0):.1f} ms")
    want_st = np.array([s for _, s in want], np.int32)
    bad = np.flatnonzero(st != want_st)
    assert not bad.size, (name, bad[:5], docs[bad[0]], int(st[bad[0]]), int(want_st[bad[0]]))
    bad = [i for i in range(len(docs)) if toks[i] != want[i][0]]
    assert not bad, (name, bad[:5], docs[bad[0]], toks[bad[0]], want[bad[0]][0])
    return st


def _restated(docs, name):
    t0 = time.perf_counter()
    want = [ref.canon_bytes(d) for d in docs]
    print(f"{name}: restatement {time.perf_counter() - t0:.2f} s")
    return want


# ---- A: every code point ----
def _block_cps(b):
    return [cp for cp in range(b * BLOCK, (b + 1) * BLOCK) if not 0xD800 <= cp < 0xE000]


@functools.lru_cache(maxsize=None)
def _block(b):
    docs = [ref.context_document(chr(cp)) for cp in _block_cps(b)]
    return docs, _restated(docs, f"A block {b}")


def test_sweep_a_counts():
    low = sum(len(_block_cps(b)) for b in range(0x20000 // BLOCK))
    assert low == 0x20000 - N_SURROGATES and low + (0x110000 - 0x20000) == N_SCALARS == 1_112_064 and N_SURROGATES == 2048


@pytest.mark.parametrize("b", range(0x20000 // BLOCK))
def test_every_code_point_below_0x20000_in_every_context(b):
    """The device's walk over d_stage1 / d_stage2 / d_pool and the flags it writes, for every entry of the table: each
    context reads one field of it (test_text_canon_spec.py shows that no two entries look alike in all of them)."""
    docs, want = _block(b)
    assert len(docs) == len(_block_cps(b)) == (BLOCK - N_SURROGATES if b == 0xC000 // BLOCK else BLOCK)
    covered = sum(ref.lookup(cp) is not None for cp in _block_cps(b))
    st = _compare(docs, want, f"A block {b}")
    assert int((st == 0).sum()) == covered          # an uncovered code point hands its whole document back


def test_every_code_point_from_0x20000_is_handed_back():
    cps = np.arange(0x20000, 0x110000, dtype=np.uint32)
    a = np.empty((cps.size, 10), np.uint8)
    a[:, :3], a[:, 7:] = np.frombuffer(b"ok ", np.uint8), np.frombuffer(b" ok", np.uint8)
    a[:, 3], a[:, 4] = 0xF0 | cps >> 18, 0x80 | (cps >> 12 & 0x3F)
    a[:, 5], a[:, 6] = 0x80 | (cps >> 6 & 0x3F), 0x80 | (cps & 0x3F)
    assert a.shape[0] == 0x110000 - 0x20000 == 983_040
    for i in (0, 12345, cps.size - 1):
        assert a[i].tobytes() == b"ok " + chr(int(cps[i])).encode("utf-8") + b" ok"
    from ucfp_amd import text
    toks, st = text.canon_batch(_rows(a))
    assert st.size == cps.size and (st == ref.NEEDS_HOST).all() and not any(toks)


def test_every_surrogate_encoding_is_handed_back():
    cps = np.arange(0xD800, 0xE000, dtype=np.uint32)
    a = np.empty((cps.size, 9), np.uint8)
    a[:, :3], a[:, 6:] = np.frombuffer(b"ok ", np.uint8), np.frombuffer(b" ok", np.uint8)
    a[:, 3], a[:, 4], a[:, 5] = 0xE0 | cps >> 12, 0x80 | (cps >> 6 & 0x3F), 0x80 | (cps & 0x3F)
    assert a.shape[0] == N_SURROGATES and a[0].tobytes() == b"ok \xed\xa0\x80 ok" and a[-1].tobytes() == b"ok \xed\xbf\xbf ok"
    docs = _rows(a)
    assert not any(_strict(d) for d in docs)
    from ucfp_amd import text
    toks, st = text.canon_batch(docs)
    assert st.size == N_SURROGATES and (st == ref.NEEDS_HOST).all() and not any(toks)


def test_hash_status_merge_over_a_block_of_tiny_documents():
    """Thousands of tiny documents, covered and handed back side by side, through the RAW_UTF8 MinHash call: the canon
    pass's status merged into the hash pass's (the construction of test_text_utf8_gpu._expect, from the shared restatement)."""
    from ucfp_amd import text
    docs, want = _block(0)
    st = np.array([s for _, s in want], np.int32)
    assert 0 < int((st == ref.NEEDS_HOST).sum()) < len(docs)
    rec, hs = text._run("minhash", [t for t, _ in want], text.PRETOKENIZED, 5)
    rec[st == ref.NEEDS_HOST] = 0
    hs = np.where(st == ref.NEEDS_HOST, ref.NEEDS_HOST, hs).astype(np.int32)
    g, gs = text._run("minhash", docs, text.RAW_UTF8, 5)
    assert np.array_equal(gs, hs), np.flatnonzero(gs != hs)[:5]
    assert np.array_equal(g, rec), np.flatnonzero((g != rec).any(axis=1))[:5]


# ---- B: every UTF-8 form ----
T3 = [0x00, 0x2F, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC2, 0xE0, 0xF0, 0xFF]
T4 = [0x00, 0x7F, 0x80, 0x90, 0xBF, 0xC0]


def _grid(*axes):
    return np.stack([g.ravel() for g in np.meshgrid(*[np.array(a, np.uint8) for a in axes], indexing="ij")], axis=1)


def _forms(width):
    if width == 2:
        return _grid(range(256), range(256))
    if width == 3:
        return _grid([0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF], range(256), T3)
    return _grid([0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xF7, 0xF8, 0xFF], range(256), T4, T4)


@pytest.mark.parametrize("width,count", [(2, 65536), (3, 6 * 256 * 14), (4, 8 * 256 * 36)])
def test_every_utf8_form(width, count):
    """Each string between `ab ` and ` cd`, and at the document's end: handed back exactly when the strict decoder raises."""
    s = _forms(width)
    assert s.shape == (count, width) and len({r.tobytes() for r in s}) == count
    mid = np.empty((count, 3 + width + 3), np.uint8)
    mid[:, :3], mid[:, 3:3 + width], mid[:, 3 + width:] = np.frombuffer(b"ab ", np.uint8), s, np.frombuffer(b" cd", np.uint8)
    docs = _rows(mid) + [b"ab " + r.tobytes() for r in s]
    assert len(docs) == 2 * count and docs[count] == b"ab " + bytes(s[0])
    strict = [_strict(d) for d in docs]
    want = _restated([d for d, ok in zip(docs, strict) if ok], f"B width {width}")[::-1]
    want = [want.pop() if ok else (b"", ref.NEEDS_HOST) for ok in strict]       # handed back exactly when the decoder raises
    assert 0 < sum(strict) < len(docs) and 0 < sum(st == 0 for _, st in want) <= sum(strict)
    _compare(docs, want, f"B width {width}")


def test_every_proper_prefix_of_a_valid_sequence_at_the_end():
    """Every lead byte C2 .. F4 with every continuation that can follow it, cut by the document's end."""
    pre = set()
    for lead in range(0xC2, 0xF5):
        width = 4 if lead >= 0xF0 else 3 if lead >= 0xE0 else 2
        lo, hi = {0xE0: (0xA0, 0xBF), 0xED: (0x80, 0x9F), 0xF0: (0x90, 0xBF), 0xF4: (0x80, 0x8F)}.get(lead, (0x80, 0xBF))
        if width == 2:
            whole = [bytes([lead, 0x80])]
        elif width == 3:
            whole = [bytes([lead, b1, 0x80]) for b1 in range(lo, hi + 1)]
        else:
            whole = [bytes([lead, b1, b2, 0x80]) for b1 in range(lo, hi + 1) for b2 in range(0x80, 0xC0)]
        for f in whole:
            assert _strict(f), f
            pre.update(f[:n] for n in range(1, width))
    pre = sorted(pre)
    assert len(pre) == 51 + (14 * 64 + 2 * 32) + (3 * 64 + 48 + 16) * 65 and not any(_strict(b"ab " + p) for p in pre)
    docs = [b"ab " + p for p in pre]
    _compare(docs, [(b"", ref.NEEDS_HOST)] * len(docs), "B prefixes")


# ---- C: every sequence at every lane ----
VALID = ["é", "日", "\U0001d400", "㎯", "…", "¼", "\U0001f110", "ﬃ", "­", "é日", "\U0001d400é"]
MALFORMED = [b"\x80", b"\xc3", b"\xe6\x97", b"\xf0\x9f\x87", b"\xc3\xa9\xa9", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
             b"\xc0\xaf", b"\xff", b"\xf0\x9d\x90\x80\x80",          # the list of the issue; the last: a fifth continuation byte
             b"\xe6", b"\xf0", b"\xf0\x9f", b"\x80\x80", b"\xe6\x97\xa5\xa5", b"\xe0\x9f\xbf", b"\xf0\x8f\xbf\xbf", b"\xf5\x80\x80\x80",
             b"\xe6\x97\xc3\xa9", b"\xf0\x9f\x87\xe6\x97\xa5"]           # a cut sequence run into by a whole one


@pytest.mark.parametrize("filler", [b"x", b"ab "], ids=["x", "ab"])
def test_every_sequence_at_every_lane(filler):
    """Each sequence behind 0 .. 131 bytes of filler, ` tail` behind it: every split of it across a step edge, a lead at lanes
    61 .. 63 whose continuation bytes are wrong or missing in the next step, a continuation byte at lanes 0 .. 2 that a
    lead of the step before claims or does not."""
    seqs = [s.encode("utf-8") for s in VALID] + MALFORMED
    assert len(seqs) >= 30 and all(_strict(s) for s in seqs[:len(VALID)]) and not any(_strict(s + b" ") for s in MALFORMED)
    docs = [(filler * 132)[:off] + s + b" tail" for s in seqs for off in range(132)]
    want = _restated(docs, f"C filler {filler!r}")
    assert sum(st == 0 for _, st in want) == 132 * len(VALID)
    _compare(docs, want, f"C filler {filler!r}")


# ---- D: dense steps ----
def _dense_families():
    fam = {"copies %04X" % cp: ref.dense_copies(cp) for cp in ref.expanders()}
    fam["dots"] = ref.dense_dots()
    for form in range(3):
        fam["open %d" % form] = ref.dense_open_segments(form)
    fam["mixed"] = ref.dense_mixed()
    return fam


def test_dense_set_reaches_every_round():
    """From the restatement alone: the dense documents put boundaries, kept tokens and dropped segments at canonical indices
    [0, 64), [64, 128) and [128, 192) of some step, and close a segment without an alphanumeric -- as a token and as a
    dropped one -- in a later round of the step that opened it and in the step after."""
    e = chr(ref.expanders()[0])
    made = ref.canon_bytes((e * 22).encode("utf-8"))
    assert len((e * 22).encode("utf-8")) <= 66 and 22 * len(ref.lookup(ord(e))[0]) >= 129 and made[1] == 0
    fams = _dense_families()
    assert len(fams) == 6 + 1 + 3 + 1 and sum(map(len, fams.values())) == 6 * 384 + 144 + 3 * 4830 + 48
    seen, closes = set(), set()

    def later(a, b):       # where b is decided, seen from a
        return "later round" if b[0] == a[0] and b[1] // 64 > a[1] // 64 else "next step" if b[0] == a[0] + 1 else "other"

    for d in fams["copies %04X" % ord(e)][::9] + fams["open 0"][::5] + fams["open 1"][::5] + fams["dots"]:
        m = ref.decide_map(d)
        bounds = [g for g, v in enumerate(m) if v[2]] + [len(m)]
        for (step, idx, bnd, kept, alnum) in m:
            seen.add(("boundary" if bnd else "inside", idx // 64))
            seen.add(("kept" if kept else "dropped", idx // 64))
        for g0, g1 in zip(bounds, bounds[1:]):
            if m[g0][3]:       # a token: from where it opened to its first alphanumeric, the provisional keep is carried
                closes.add((True, later(m[g0], next(v for v in m[g0:g1] if v[4]))))
            elif g1 < len(m):  # dropped: the boundary that closes it rewinds what was stored since it opened
                closes.add((False, later(m[g0], m[g1])))
    for r in range(3):
        assert {("boundary", r), ("kept", r), ("dropped", r)} <= seen, (r, sorted(seen))
    assert {(k, w) for k in (True, False) for w in ("later round", "next step")} <= closes, sorted(closes)


@pytest.mark.parametrize("i", range(6))
def test_dense_copies(i):
    cp = ref.expanders()[i]
    docs = ref.dense_copies(cp)
    assert len(docs) == 6 * 64
    _compare(docs, _restated(docs, "D copies %04X" % cp), "D copies %04X" % cp)


def test_dense_dots():
    docs = ref.dense_dots()
    want = _restated(docs, "D dots")
    assert all(w == (b"a", 0) for w in want)
    _compare(docs, want, "D dots")


@pytest.mark.parametrize("form", range(3))
def test_dense_open_segments(form):
    docs = ref.dense_open_segments(form)
    assert len(docs) == 23 * 70 * 3
    _compare(docs, _restated(docs, f"D open {form}"), f"D open {form}")


def test_dense_mixed_and_the_window_limit():
    """Random dense documents and one token of expander-made letters at the window limit and one byte over it, records too.
    (The densest expander's own canonical form holds a boundary, so the token is made of the densest one whose code
    points all join.)"""
    from test_text_utf8_gpu import _check
    from ucfp_amd import text
    docs = ref.dense_mixed()
    half = [sum(len(ch.encode()) for ch in d.decode() if ord(ch) in ref.expanders()) * 2 >= len(d) for d in docs]
    assert all(half) and len(docs) == 48
    j = chr(ref.joining_expander())
    per = len(ref.lookup(ord(j))[0])
    w = text.MAX_WINDOW_BYTES
    limit = [(j * (w // per) + "a" * (w % per)).encode(), (j * (w // per) + "a" * (w % per + 1)).encode()]
    assert [len(ref.canon_bytes(d)[0]) for d in limit] == [w, w + 1] and b" " not in ref.canon_bytes(limit[1])[0]
    _check(docs + limit, kinds=[("minhash", 5), ("simhash", 1)])
    _, st = text._run("minhash", limit[:1], text.RAW_UTF8, 5)
    assert st[0] == 0
