"""UTF-8 streams without a GPU: the plain-Python restatement of the streaming canonicaliser
(tests/text_canon_stream_ref.py) against the offline restatement (tests/text_canon_ref.py) on the whole document --
held-back raw bytes, one undecided canonical code point, consumed Cf, partial emission of an open token, provisional
bytes under the open-segment cap."""
import random

import pytest

import text_canon_ref as ref
import text_canon_stream_ref as sref
from ucfp_amd.text import STREAM_OPEN_SEGMENT_BYTES, STREAMS_UTF8   # the feature under test

CF = "\u00ad\u200b\u200d\u2060\ufeff"
LETTERS = "abe\u00e9\u03b1\u0436\u05d0\u05d1"
HEBREW = "\u05d0\u05d1\u05e9"


def _biased(rng) -> str:
    """Generator in the style of test_text_canon_spec.py's, biased toward what a cut can break: MidLetter / MidNum between
    letters and digits, quotes after Hebrew letters, apostrophe + vowel, `_` runs and Cf runs."""
    parts = []
    for _ in range(rng.randint(1, 8)):
        r = rng.random()
        if r < 0.30:
            parts.append(ref.random_string(rng, 1, 4))
        elif r < 0.40:
            parts.append(rng.choice(LETTERS) + rng.choice(":.'\u00b7\u2019\u2027") + rng.choice(LETTERS + "1 "))
        elif r < 0.50:
            parts.append(rng.choice("0179") + rng.choice(",;.'\u066c") + rng.choice("05a "))
        elif r < 0.60:
            parts.append(rng.choice(HEBREW) + rng.choice("'\"") + rng.choice([rng.choice(HEBREW), "", "a", " "]))
        elif r < 0.70:
            parts.append(rng.choice(["", "x ", "l"]) + rng.choice("'\u2019") + rng.choice("aeiou\u00e9xz "))
        elif r < 0.80:
            parts.append("_" * rng.randint(1, 6) + rng.choice(["", "a", " ", "1", "\u30ab"]))
        elif r < 0.90:
            parts.append(rng.choice(CF) * rng.randint(1, 5))
        else:
            parts.append(rng.choice(" \n-"))
    return "".join(parts)


def _cut_sets(rng, n: int):
    """The cuts a document of n bytes is tried with: a short one at every byte and one byte at a time, a longer one at
    random places (repeats give empty chunks)."""
    if n <= 12:
        return [[c] for c in range(n + 1)] + [list(range(1, n))]
    return [sorted(rng.randint(0, n) for _ in range(rng.randint(1, 5))) for _ in range(2)] + [list(range(1, n))]


def test_pieces_of_any_cut_equal_the_offline_string():
    rng = random.Random(20261019)
    ok = 0
    for it in range(20_000):
        doc = _biased(rng).encode("utf-8")
        want = ref.canon_bytes(doc)
        ok += want[1] == 0
        for cuts in _cut_sets(rng, len(doc)):
            assert sref.stream_canon(doc, cuts) == want, (doc, cuts)
    assert ok > 15_000          # the generator stays inside the covered set: the property is about tokens, not hand-backs


@pytest.mark.parametrize("s", ["l'\u00e9t\u00e9", "x \u2019e", "1,000;2", "a:b", "_a", "__ ", "\u05d0\"\u05d1 \u05d0'", "a\u200b:\u200bb",
                               "\ufb01n \uff21\uff22", "\u65e5\u672c\u8a9e\u30ab\u30bf\u30ab\u30ca", "", "\u200b", "a" + "\u200b" * 100 + "b"])
def test_named_cases_cut_at_every_byte_and_byte_by_byte(s):
    doc = s.encode("utf-8")
    want = ref.canon_bytes(doc)
    assert want[1] == 0
    for c in range(len(doc) + 1):
        assert sref.stream_canon(doc, [c]) == want, c
    assert sref.stream_canon(doc, list(range(1, len(doc)))) == want


def test_malformed_and_uncovered_text_is_handed_back_not_before_it_is_seen():
    for bad in (b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xff", b"\x80", b"\xc3\xa9\xa9",
                "\u0301".encode(), "\U0001F1E6".encode(), "\U00020000".encode()):
        doc = b"ok " + bad + b" ok"
        for c in range(len(doc) + 1):
            st = sref.CanonStream()
            _, s1 = st.push(doc[:c], False)
            _, s2 = st.push(doc[c:], True)
            assert s2 == sref.NEEDS_HOST and (s1 == 0 or c > 3), (bad, c)
    for cutoff in (b"ab\xc3", b"ab\xe6\x97", b"ab\xf0\x9f\x87"):         # incomplete: held at a non-final push, malformed at the end
        st = sref.CanonStream()
        assert st.push(cutoff, False) == (b"a", 0)            # `b` is the undecided code point, the sequence is held
        assert st.push(b"", True) == (b"", sref.NEEDS_HOST)
    st = sref.CanonStream()
    assert st.push(b"caf\xc3", False)[1] == 0 and st.push(b"\xa9", True)[1] == 0


def _rule_trips(doc: bytes, cuts) -> bool:
    """The open-segment condition stated on the prefix alone: at a push boundary all canonical code points but the last
    are decided; the decided tail since the last boundary is pending iff none of it is alphanumeric."""
    for c in cuts:
        p = doc[:c]
        x = ref.canonical(map(ord, p[:len(p) - sref.incomplete_tail(p)].decode("utf-8")))
        dec = len(x) - 1
        b = max([i for i in range(1, dec) if not ref._joined(x, i)], default=0)
        seg = x[b:dec]
        if seg and not any(fl & 16 for _, fl in seg) and 1 + sum(len(chr(cp).encode()) for cp, _ in seg) > sref.OPEN_SEGMENT_BYTES:
            return True
    return False


def test_open_segment_cap_trips_exactly_when_the_rule_says_so():
    assert sref.OPEN_SEGMENT_BYTES == 256
    rng = random.Random(7)
    tripped = 0
    for it in range(400):
        ch = rng.choice("_\u02c2")
        doc = (rng.choice(["", "ab ", "\u00e9"]) + ch * rng.randint(100, 330) + rng.choice(["a", " x", "", "\u200b"])).encode("utf-8")
        cuts = sorted(rng.randint(0, len(doc)) for _ in range(rng.randint(1, 3)))
        trip = _rule_trips(doc, cuts)
        tripped += trip
        assert sref.stream_canon(doc, cuts) == ((b"", sref.NEEDS_HOST) if trip else ref.canon_bytes(doc)), (doc, cuts)
    assert 50 < tripped < 350
    doc = b"_" * 300 + b"a"
    assert sref.stream_canon(doc, []) == ref.canon_bytes(doc) == (doc, 0)
    assert sref.stream_canon(doc, [280]) == (b"", sref.NEEDS_HOST)
    assert sref.stream_canon(doc, [250]) == (doc, 0)
    assert sref.stream_canon(doc, [256]) == (doc, 0) and sref.stream_canon(doc, [257]) == (b"", sref.NEEDS_HOST)   # ' ' + 255 decided
    st = sref.CanonStream()
    assert st.push(doc[:280], False) == (b"", sref.NEEDS_HOST) and st.push(b"a", False) == (b"", sref.NEEDS_HOST)   # sticky


def test_the_library_and_the_wrapper_name_the_same_condition():
    """Host-only entry points of the feature: usable without a device."""
    from ucfp_amd import _lib
    lib = _lib.load()
    assert STREAM_OPEN_SEGMENT_BYTES == sref.OPEN_SEGMENT_BYTES
    assert lib.ucfp_text_streams_state_bytes_ex(0) == lib.ucfp_text_streams_state_bytes()
    extra = lib.ucfp_text_streams_state_bytes_ex(STREAMS_UTF8) - lib.ucfp_text_streams_state_bytes()
    assert sref.OPEN_SEGMENT_BYTES < extra <= sref.OPEN_SEGMENT_BYTES + 64     # the provisional bytes and a few words
    import ctypes as C
    h = C.c_void_p()
    assert lib.ucfp_text_streams_create_ex(None, 0, 1, STREAMS_UTF8, 4096, C.byref(h)) == -1      # k first, as create
    assert lib.ucfp_text_streams_create_ex(None, 5, 1, 2, 4096, C.byref(h)) == -4 and b"flags" in lib.ucfp_last_error()
    assert lib.ucfp_text_streams_create_ex(None, 5, 1, STREAMS_UTF8, 4096, None) == -4
