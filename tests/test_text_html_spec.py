"""DESIGN.md T12 without a GPU: the plain-Python restatement of rules M1-M8 (tests/text_html_ref.py) against the standard
library's html.parser on generated pages, a pinned table of hand-written vectors, the length bound, and the compiled
table of named references (ucfp_text_html_entity) against html.entities."""
import ctypes as C
import random
from html.entities import name2codepoint
from html.parser import HTMLParser

import pytest

import text_html_ref as ref

VECTORS = ref.VECTORS


def test_vectors():
    for page, text, flags in VECTORS:
        assert ref.html_to_text(page) == (text, flags), page


class _Harness(HTMLParser):
    """html.parser as an independent check: the same inline set and the same white-space fold on top of its events."""

    def __init__(self):
        super().__init__(convert_charrefs=True)
        self.out = []
        self.raw = None

    def _tag(self, tag):
        if tag not in ref.INLINE:
            self.out.append((" ", True))

    def handle_starttag(self, tag, attrs):
        self._tag(tag)
        if tag in ("script", "style"):
            self.raw = tag

    def handle_endtag(self, tag):
        self._tag(tag)
        if tag == self.raw:
            self.raw = None

    def handle_startendtag(self, tag, attrs):
        self._tag(tag)

    def handle_data(self, data):
        if self.raw is None:
            self.out += [(ch, ch in "\t\n\f\r ") for ch in data]

    def handle_comment(self, data):
        self.out.append((" ", True))

    handle_decl = handle_pi = unknown_decl = handle_comment


def _html_parser_text(page: str) -> bytes:
    h = _Harness()
    h.feed(page)
    h.close()
    out, pending = [], False
    for ch, ws in h.out:
        if ws:
            pending = True
            continue
        if pending and out:
            out.append(" ")
        pending = False
        out.append(ch)
    return "".join(out).encode("utf-8")


def test_restatement_equals_html_parser_on_generated_pages():
    rng = random.Random(7)
    bad = []
    for i in range(5000):
        page = ref.gen_page(rng, blocks=rng.randrange(1, 5), words=rng.randrange(1, 7))
        got, flags = ref.html_to_text(page.encode("utf-8"))
        if got != _html_parser_text(page) or flags & ref.FLAG_OPEN_MARKUP:
            bad.append(i)
    assert not bad, f"{len(bad)} of 5000 pages disagree, first {bad[:5]}"


def test_generated_pages_hold_every_construct():
    """The comparison above means something only while the generator makes what DESIGN.md T12 lists."""
    rng = random.Random(7)
    pages = "".join(ref.gen_page(rng) for _ in range(200))
    for needle in ("<!DOCTYPE", "<?", "<!--", "--x", "</scripty>", '="a>b"', "='a>b'", "it's", 'say "hi"', "/>", "&#x", "&#X",
                   "&amp;", "1 < 2", "漢"):
        assert needle in pages, needle
    for needle in ("<script", "<style", "</script\n>", "<br", "<strong", "<my-el"):          # tag names come in mixed case
        assert needle in pages.lower(), needle
    assert pages.lower().count("<script") > pages.count("<script")


def test_output_is_never_longer_than_the_input():
    rng = random.Random(11)
    worst = 0
    for _ in range(10000):
        doc = ref.fuzz_doc(rng)
        text, _ = ref.html_to_text(doc)
        assert len(text) <= len(doc), doc
        worst = max(worst, len(text) - len(doc))
    assert worst == 0                      # some string passes through whole
    for page, n in ((b"<p>", 0), (b"a<p>b", 3), (b"&ni;", 3), (b"&#65536;", 4)):
        assert len(ref.html_to_text(page)[0]) == n


@pytest.fixture(scope="module")
def lib():
    from ucfp_amd import _lib
    return _lib.load()


def _entity(lib, name: bytes):
    cp = C.c_uint32(0xDEAD)
    ok = lib.ucfp_text_html_entity(name, len(name), C.byref(cp))
    return ok, cp.value


def test_compiled_entity_table_is_pythons(lib):
    names = dict(name2codepoint, apos=0x27)
    assert len(names) == 253 and max(map(len, names)) == 8 and max(names.values()) == 0x2666
    for name, cp in names.items():
        assert _entity(lib, name.encode()) == (1, cp), name
        cut = name[:-1]
        if cut not in names:
            assert _entity(lib, cut.encode()) == (0, 0), cut
        for other in (name.upper(), name.lower(), name.swapcase()):
            if other not in names:
                assert _entity(lib, other.encode()) == (0, 0), other
    for junk in (b"", b"bogus", b"thetasymx", b"amp;", b"l\0t", b"lt\0"):
        assert _entity(lib, junk) == (0, 0), junk
    assert lib.ucfp_text_html_entity(b"lt", 2, None) == 1 and lib.ucfp_text_html_entity(None, 2, None) == 0
    assert ref.ENTITIES == names


def test_bound_is_the_identity(lib):
    for n in (0, 1, 63, 4096, 1 << 40, (1 << 64) - 1):
        assert lib.ucfp_text_html_bound(n) == n


def test_committed_table_is_what_the_generator_writes(capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_text_html_tab", os.path.join(root, "tools", "gen_text_html_tab.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.main()
    assert capsys.readouterr().out == open(os.path.join(root, "include", "ucfp_text_html_tab.h")).read()
