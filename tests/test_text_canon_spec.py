"""Text mode RAW_UTF8 without a GPU: the compiled code-point table against U1 recomputed here, and the table-driven
restatement (tests/text_canon_ref.py) against the host path it must equal."""
import random
import unicodedata

import pytest

import text_canon_ref as ref
from ucfp_amd.text import Canonicalizer, _host_tokens

regex = pytest.importorskip("regex")


@pytest.fixture(scope="module", autouse=True)
def _versions():
    want = ref.table_versions()
    have = (unicodedata.unidata_version, regex.__version__)
    if want != have:
        pytest.skip(f"the table is bound to unicodedata {want[0]} / regex {want[1]}; this interpreter has {have[0]} / {have[1]}")


WB = ["ALetter", "Hebrew_Letter", "Numeric", "Katakana", "ExtendNumLet", "MidLetter", "MidNum", "MidNumLet", "Single_Quote",
      "Double_Quote"]


def _probe(names):
    pats = [(w, regex.compile(r"\p{WB=%s}" % w)) for w in names]

    def f(ch):
        for w, p in pats:
            if p.match(ch):
                return w
        return "Other"
    return f


def test_table_equals_u1_for_every_code_point():
    canon = Canonicalizer()
    back = set(range(0x1161, 0x1176)) | set(range(0x11A8, 0x11C3))
    for cp in range(0x110000):
        d = unicodedata.decomposition(chr(cp))
        if d and not d.startswith("<") and len(d.split()) == 2:
            back.add(int(d.split()[1], 16))
    excluded, wb = _probe(["Extend", "Regional_Indicator"]), _probe(WB)

    def safe(ch):
        return unicodedata.combining(ch) == 0 and ord(ch) not in back

    def u1(cp):
        if cp >= 0x20000:
            return None
        ch = chr(cp)
        if unicodedata.category(ch) in ("Cn", "Cs", "Co"):
            return None
        n1 = unicodedata.normalize("NFKC", ch)
        m = canon.apply(ch)
        if not all(safe(x) for x in ch + n1 + n1.casefold() + m):
            return None
        if any(excluded(x) != "Other" for x in m) or len(m.encode()) > 3 * len(ch.encode()) or any(ord(x) >= 0x20000 for x in m):
            return None
        return m

    covered = 0
    for cp in range(0x110000):
        want, got = u1(cp), ref.lookup(cp)
        assert (want is None) == (got is None), hex(cp)
        if want is None:
            continue
        covered += 1
        assert "".join(map(chr, got[0])) == want, hex(cp)
        if unicodedata.category(chr(cp)) == "Cf":
            assert want == ""
        for x in want:
            mx, fx = ref.lookup(ord(x))
            assert mx == (ord(x),), (hex(cp), hex(ord(x)))                       # idempotent
            assert bool(fx & 16) == x.isalnum(), (hex(cp), hex(ord(x)))
            assert (fx & 15) == (["Other"] + WB).index(wb(x)), (hex(cp), hex(ord(x)))
            assert bool(fx & 32) == (_host_tokens("'" + x) == ["'" + x]), (hex(cp), hex(ord(x)))
        if len(want) == 1:
            assert got[1] == ref.lookup(ord(want))[1]
    assert covered > 75000


def test_restatement_equals_the_host_path():
    canon = Canonicalizer()
    rng = random.Random(20260719)
    for it in range(100_000):
        s = ref.random_string(rng, 1, 14)
        assert ref.tokens(s) == _host_tokens(canon.apply(s)), [hex(ord(c)) for c in s]


@pytest.mark.parametrize("s", ["x 'e y", "_a", "\u02c2\u02c2a", "a\u2019e", "a.b", "\u05d0\"\u05d1", "a_1", "1,5", "rad\u2215s2 \u33af",
                               "\u65e5\u672c\u8a9e\u30ab\u30bf\u30ab\u30caabc", "a\u200d:\u200db", "", "\u200b", "__ _", "\ufb03"])
def test_restatement_on_named_cases(s):
    assert ref.tokens(s) == _host_tokens(Canonicalizer().apply(s))


def test_malformed_utf8_and_uncovered_code_points_go_back_to_the_host():
    for bad in (b"\xc0\xaf", b"\xe0\x80\xaf", b"\xf0\x80\x80\xaf",      # overlong
                b"\xed\xa0\x80", b"\xed\xbf\xbf",                        # surrogates
                b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xff",       # above 0x10FFFF / no lead byte
                b"\x80", b"a\xbfb", b"\xc3\xa9\xa9",                     # stray continuation bytes
                b"\xc3", b"ab\xe6\x97", b"\xf0\x9f\x87"):                # cut by the document's end
        assert ref.canon_bytes(b"ok " + bad) == (b"", ref.NEEDS_HOST), bad
    for cp in (0x0301, 0x1161, 0x1F1E6, 0x0130, 0xFDFA, 0xE0001, 0x20000, 0x0378):
        assert ref.lookup(cp) is None, hex(cp)
        assert ref.canon_bytes(("ok " + chr(cp) + " ok").encode("utf-8")) == (b"", ref.NEEDS_HOST), hex(cp)
    assert ref.canon_bytes("Stra\u00dfe \uff21\uff22 \u2163".encode("utf-8")) == ("strasse ab iv".encode(), 0)


def test_host_only_entry_points_need_no_gpu():
    import ctypes as C
    from ucfp_amd import _lib
    lib = _lib.load()
    assert lib.ucfp_text_canon_bound(0) == 0 and lib.ucfp_text_canon_bound(4096) == 4 * 4096
    assert lib.ucfp_text_canon_bound(2**64 - 1) == 2**64 - 1                  # saturates
    assert lib.ucfp_text_canon_batch(None, None, None, 0, None, 0, None, None) == -4 and b"ctx" in lib.ucfp_last_error()
    assert lib.ucfp_text_canon_batch_dev(None, None, None, 0, None, None, None, None) == -4
    assert lib.ucfp_text_minhash_batch(None, None, None, 0, 2, 5, None, None) == -4
    out, n, fl = (C.c_uint32 * 8)(), C.c_uint32(9), C.c_uint32(9)
    assert lib.ucfp_text_utab_lookup(0x110000, out, C.byref(n), C.byref(fl)) == 0 and n.value == 0 and fl.value == 0
    assert lib.ucfp_text_utab_lookup(ord("A"), None, None, None) == 1        # every out pointer is optional
    assert lib.ucfp_text_utab_lookup(ord("A"), out, C.byref(n), C.byref(fl)) == 1 and (out[0], n.value, fl.value) == (97, 1, 1 | 16 | 32)
    assert lib.ucfp_text_utab_lookup(0xAD, out, C.byref(n), C.byref(fl)) == 1 and n.value == 0     # soft hyphen: Cf, deleted


# ---- what tests/test_text_canon_sweep_gpu.py relies on, from the restatement alone ----
def test_contexts_tell_every_pair_of_table_entries_apart():
    """The contexts of the every-code-point sweep are not blind: any two (class, alnum, vowel) triples that occur among
    the table's canonical code points give different tokens in at least one context."""
    flags = ref.canonical_flags()
    assert len(flags) >= 16 and {f & 15 for f in flags} == set(range(11))        # every class occurs
    sig = {f: ref.context_signature(f) for f in flags}
    same = [(a, b) for i, a in enumerate(flags) for b in flags[i + 1:] if sig[a] == sig[b]]
    assert not same, same
    doc = ref.context_document("é")
    assert doc.count(b"  ") == len(ref.CONTEXTS) - 1 and ref.canon_bytes(doc)[1] == 0


def test_expanders_are_found_in_the_table():
    ex = ref.expanders()
    assert {0x33AF, 0x2152, 0x00BC, 0x1F110, 0x2026} <= set(ex) and ex[0] == 0x33AF and ref.quiet_expander() == 0x2026
    made = {cp: (len(chr(cp).encode()), len(ref.lookup(cp)[0])) for cp in ex}
    assert made[0x33AF] == (3, 6) and made[0x2152] == (3, 4) and made[0xBC] == (2, 3) and made[0x1F110] == (4, 3) and made[0x2026] == (3, 3)
    for cp in range(0x20000):                  # nothing in the table is denser than the densest of its width
        r = ref.lookup(cp)
        if r is not None and cp >= 0x80:
            w = len(chr(cp).encode("utf-8", "surrogatepass"))
            assert len(r[0]) <= max(n for c, (ww, n) in made.items() if ww == w), hex(cp)
    assert not any(ref.lookup(x)[1] & 16 for x in ref.lookup(ref.quiet_expander())[0])
    # 22 copies of the densest: three rounds of 64 in one step and the lead of the next
    doc = (chr(ex[0]) * 22).encode()
    assert len(doc) <= 66 and len(ref.canonical(map(ord, doc.decode()))) >= 129
    m = ref.decide_map(doc)
    assert len(m) == 132 and [v[:2] for v in m[:131]] == [(0, i) for i in range(131)] and m[131][:2] == (1, 0)
    j = ref.joining_expander()
    assert ref.tokens(chr(j) * 50) == ["".join(map(chr, ref.lookup(j)[0])) * 50]


BOUND_BLOCK = 0x4000


@pytest.mark.parametrize("b", range(0x20000 // BOUND_BLOCK))
def test_token_bytes_stay_within_the_workspace_bound(b, capsys):
    """ucfp_text_canon_bound sizes the workspace the emit pass writes into: every covered code point alone, between each
    of four separators and eight times over stays within it."""
    from ucfp_amd import _lib
    bound = _lib.load().ucfp_text_canon_bound
    worst = (0.0, "")
    for cp in range(b * BOUND_BLOCK, (b + 1) * BOUND_BLOCK):
        if ref.lookup(cp) is None:
            continue
        c = chr(cp)
        for s in [c, c * 8] + [sep + c + sep for sep in (" ", "a", "1", "日")]:
            src = s.encode("utf-8")
            out, st = ref.canon_bytes(src)
            assert st == 0 and len(out) <= bound(len(src)), (hex(cp), s)
            worst = max(worst, (len(out) / len(src), s))
    with capsys.disabled():
        print(f"\ncanon bound, code points {b * BOUND_BLOCK:#x} ..: worst token bytes / source bytes = {worst[0]:.3f} for {worst[1]!r}")
