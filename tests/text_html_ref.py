"""Plain-Python restatement of DESIGN.md T12 (rules M1-M8): HTML bytes -> text bytes, as ucfp_text_html_batch computes them.

    html_to_text(doc: bytes) -> (text bytes, flags)      flags bit 0: a byte >= 0x80 in the output; bit 1: ended in markup

It imports nothing from ucfp_amd: the kernel (ucfp_amd/csrc/text_html.hip) is compared with it byte for byte, and
tests/test_text_html_spec.py compares it with the standard library's html.parser on generated pages.  It walks the
document serially, one rule at a time; the kernel resolves 64 bytes at once from ballots.
"""
from html.entities import name2codepoint

WS = frozenset(b"\t\n\f\r ")
DELIM = WS | frozenset(b"/>")
INLINE = frozenset(("a abbr b bdi bdo big cite code data del dfn em font i ins kbd label mark q s samp small span strike "
                    "strong sub sup time tt u var wbr").split())
ENTITIES = dict(name2codepoint, apos=0x27)           # M7: the 252 names of HTML 4, and apos
FLAG_NON_ASCII, FLAG_OPEN_MARKUP = 1, 2
_DIGITS = frozenset(b"0123456789")
_HEX = frozenset(b"0123456789abcdefABCDEF")


def _letter(doc: bytes, i: int) -> bool:
    return i < len(doc) and (0x41 <= doc[i] <= 0x5A or 0x61 <= doc[i] <= 0x7A)


def tag_class(doc: bytes, at: int) -> str:
    """M4: the class of the tag whose name starts at doc[at] -- "inline", "script", "style" or "break"."""
    for name in INLINE | {"script", "style"}:
        end = at + len(name)
        if doc[at:end].lower() == name.encode() and end < len(doc) and doc[end] in DELIM:
            return name if name in ("script", "style") else "inline"
    return "break"


def tag_end(doc: bytes, i: int) -> int:
    """M3: the index of the `>` that ends the tag whose extent starts at doc[i] (the byte after `<`), or -1."""
    state = "TAG"
    while i < len(doc):
        c = doc[i]
        if state == "TAG":
            if c == 0x3E:
                return i
            if c == 0x3D:
                state = "EQ"
        elif state == "EQ":
            if c == 0x3E:
                return i
            if c == 0x22:
                state = "DQ"
            elif c == 0x27:
                state = "SQ"
            elif c not in WS and c != 0x3D:
                state = "TAG"
        elif state == "DQ":
            if c == 0x22:
                state = "TAG"
        elif c == 0x27:
            state = "TAG"
        i += 1
    return -1


def reference(doc: bytes, i: int):
    """M7: doc[i] is `&`.  -> (code point, bytes of the reference) or None."""
    semi = doc.find(b";", i + 1, i + 10)
    if semi < 0:
        return None
    body = doc[i + 1:semi]
    if body[:1] == b"#":
        if body[1:2] in (b"x", b"X"):
            digits, ok, base = body[2:], _HEX, 16
            if not 1 <= len(digits) <= 6:
                return None
        else:
            digits, ok, base = body[1:], _DIGITS, 10
            if not 1 <= len(digits) <= 7:
                return None
        if any(d not in ok for d in digits):
            return None
        cp = int(digits, base)
        if cp == 0 or 0xD800 <= cp <= 0xDFFF or cp > 0x10FFFF:
            cp = 0xFFFD
        return cp, semi + 1 - i
    try:
        name = body.decode("ascii")
    except UnicodeDecodeError:
        return None
    if name in ENTITIES:
        return ENTITIES[name], semi + 1 - i
    return None


def _raw_end(doc: bytes, i: int, name: bytes) -> int:
    """M5: the first `</name` (ci) at or after i that ws, `/` or `>` follows, or -1."""
    low = doc.lower()
    pat = b"</" + name
    while True:
        at = low.find(pat, i)
        if at < 0:
            return -1
        end = at + len(pat)
        if end < len(doc) and doc[end] in DELIM:
            return at
        i = at + 1


def html_to_text(doc: bytes):
    doc = bytes(doc)
    n = len(doc)
    pieces = []            # the stream of M1-M7: (bytes, is ws)
    flags = 0
    i = 0
    while i < n:
        c = doc[i]
        if c == 0x3C:
            nxt = doc[i + 1] if i + 1 < n else 0
            if nxt in (0x21, 0x3F):                                    # M2
                if doc[i:i + 4] == b"<!--":
                    at = doc.find(b"-->", i + 4)
                    end = at + 2 if at >= 0 else -1
                else:
                    end = doc.find(b">", i + 1)
                if end < 0:
                    flags |= FLAG_OPEN_MARKUP
                    break
                pieces.append((b" ", True))
                i = end + 1
                continue
            is_end = nxt == 0x2F
            if _letter(doc, i + 2 if is_end else i + 1):               # M1, M3-M6
                cls = tag_class(doc, i + 2 if is_end else i + 1)
                end = tag_end(doc, i + 1)
                if end < 0:
                    flags |= FLAG_OPEN_MARKUP
                    break
                if cls != "inline":
                    pieces.append((b" ", True))
                i = end + 1
                if cls in ("script", "style") and not is_end:          # M5
                    at = _raw_end(doc, i, cls.encode())
                    if at < 0:
                        flags |= FLAG_OPEN_MARKUP
                        break
                    end = tag_end(doc, at + 1)
                    if end < 0:
                        flags |= FLAG_OPEN_MARKUP
                        break
                    pieces.append((b" ", True))
                    i = end + 1
                continue
        elif c == 0x26:                                                # M7
            r = reference(doc, i)
            if r is not None:
                cp, used = r
                pieces.append((chr(cp).encode("utf-8", "surrogatepass"), cp in WS))
                i += used
                continue
        pieces.append((doc[i:i + 1], c in WS))
        i += 1
    out = bytearray()                                                  # M8
    pending = False
    for b, ws in pieces:
        if ws:
            pending = True
            continue
        if pending and out:
            out += b" "
        pending = False
        out += b
    if any(x >= 0x80 for x in out):
        flags |= FLAG_NON_ASCII
    return bytes(out), flags


def html_to_text_batch(docs):
    """-> (texts, offsets list of n + 1, flags list): the arrays ucfp_text_html_batch fills."""
    texts, flags, offs = [], [], [0]
    for d in docs:
        t, f = html_to_text(d)
        texts.append(t)
        flags.append(f)
        offs.append(offs[-1] + len(t))
    return texts, offs, flags


FFFD = "�".encode()

# ---- pinned vectors (page, text, flags): tests/test_text_html_spec.py holds the restatement to them,
# tests/test_text_html_gpu.py the kernel ----
VECTORS = [
    (b"a < b", b"a < b", 0),
    (b"<p", b"", 2),
    (b"x<!-- y", b"x", 2),
    (b"<b>bo</b>ld", b"bold", 0),
    (b"<p>a</p><p>b</p>", b"a b", 0),
    (b"&lt;p&gt;", b"<p>", 0),
    (b"&#0;&#xD800;&#1114112;&bogus;&amp", FFFD * 3 + b"&bogus;&amp", 1),
    (b"<a title=it's>t</a>", b"t", 0),
    (b"</ >x", b"</ >x", 0),
    (b"<!-->x-->y", b"y", 0),
    (b"<scr<script>z</script>ipt>w", b"z ipt>w", 0),
    (b"<a-b>x", b"x", 0),
    (b"<SCRIPT>a</scripty></script >b", b"b", 0),
    (b" \t\n\f\r ", b"", 0),
    # further corners of each rule
    (b"", b"", 0),
    (b"<", b"<", 0),
    (b"a</", b"a</", 0),
    (b"<3 and <- and <>", b"<3 and <- and <>", 0),
    (b"<!--->x-->y", b"y", 0),
    (b"a<!---->b", b"a b", 0),
    (b"a<![CDATA[x>y]]>z", b"a y]]>z", 0),
    (b"a<?php echo 1 ?>b", b"a b", 0),
    (b'<p class="a>b">x', b"x", 0),
    (b"<p class='a>b\">c'>x", b"x", 0),
    (b'<p class = "a>b">x', b"x", 0),
    (b"<p class=a\"b>x", b"x", 0),
    (b'<p a="1"b="2>">x', b"x", 0),
    (b"a<br>b<br/>c<wbr>d<WBR/>e", b"a b cde", 0),
    (b"a<strongx>b</strong>c<strong >d", b"a bcd", 0),
    (b"x<style>p > a {}</style>y", b"x y", 0),
    (b"x<script/>y</script>z", b"x z", 0),
    (b"x<style>y</script>z", b"x", 2),
    (b"x<script>y</script", b"x", 2),
    (b"x<script>y</script z", b"x", 2),
    (b"a</script>b", b"a b", 0),
    (b"x<b", b"x", 2),
    (b"&amp;&apos;&quot;&thetasym;&ni;", b"&'\"" + "ϑ∋".encode(), 1),
    (b"&#65;&#x41;&#X41;&#0000065;&#x000041;", b"AAAAA", 0),
    (b"&#00000065;&#x0000041;&#;&#x;&#xG;&#6a;", b"&#00000065;&#x0000041;&#;&#x;&#xG;&#6a;", 0),
    (b"&#65536;&#x10FFFF;&#9999999;", "\U00010000\U0010ffff�".encode(), 1),
    (b"&#128;&#150;", "\x80\x96".encode(), 1),
    (b"a&#32;&#9;&#10;b&nbsp;c", b"a b\xc2\xa0c", 1),
    (b"&#32;a&#32;", b"a", 0),
    (b"&AMP;&Lt;&aMp;", b"&AMP;&Lt;&aMp;", 0),
    (b"&a&amp;&<b>&lt;</b>", b"&a&&<", 0),
    (b"a\x0bb\xa0c", b"a\x0bb\xa0c", 1),
    (b"\xff\xfe\x80", b"\xff\xfe\x80", 1),
    (b"<p>\xe6\xbc\xa2</p>", b"\xe6\xbc\xa2", 1),
    (b"<p title='\xc3\xa9'>e</p>", b"e", 0),
    # a 0x00 is a byte like any other: no delimiter, no part of a name
    (b"a<b\0>c", b"a c", 0),
    (b"a<em\0>c<\0b>", b"a c<\0b>", 0),
    (b"a<B\0 >c</b\0>d", b"a c d", 0),
    (b"<style>x</style\0>y", b"", 2),
    (b"<style>x</style\0></style>y", b"y", 0),
    (b"<script\0>x</script>y", b"x y", 0),
    (b"&lt\0;&amp\0\0;&\0lt;&#6\x005;&#x\x0041;", b"&lt\0;&amp\0\0;&\0lt;&#6\x005;&#x\x0041;", 0),
    (b"a\0b \0 c", b"a\0b \0 c", 0),
]


# ---- generators for the tests (tests/test_text_html_spec.py, tests/test_text_html_gpu.py) ----

# the alphabet of the random strings: weighted towards what the automaton and the reference matcher look at
FUZZ_ALPHABET = ([b"<", b">", b'"', b"'", b"=", b"-", b"!", b"?", b"/", b"&", b";", b"#", b"x"] * 3
                 + [b"script", b"style", b"SCRIPT", b"</", b"<!--", b"-->", b"&amp;", b"&lt", b"lt;", b"&#", b"strong", b"div"]
                 + [b" ", b" ", b"\n", b"\t", b"\r", b"\f", b"a", b"b", b"p", b"i", b"Q", b"0", b"1", b"9", b"F", b"e"]
                 + ["é".encode(), "ß".encode(), b"\xc2\xa0"]
                 # bytes are bytes: 0x00 (packs as nothing into a name), a control byte that is no ws, lone UTF-8 pieces
                 + [b"\0", b"\0", b"\x0b", b"\x80", b"\xbf", b"\xc3", b"\xff"])


def fuzz_doc(rng, max_pieces: int = 60) -> bytes:
    """A random string over FUZZ_ALPHABET; `rng` is a random.Random."""
    return b"".join(rng.choice(FUZZ_ALPHABET) for _ in range(rng.randrange(max_pieces + 1)))


_BLOCK = ["p", "div", "h1", "h2", "ul", "li", "table", "tr", "td", "section", "blockquote", "my-el", "article"]
_INLINE = sorted(INLINE - {"wbr"})
_VOID = ["br", "hr", "img", "input", "wbr"]
_WORDS = ("the quick brown fox jumps over the lazy dog while seven wizards quietly mix potions near a frozen lake "
          "and nobody expects any answer before dawn breaks again").split()
_UTF8 = ["é", "ü", "ß", "漢", "字", "語", "Ж", "😀"]
# generated pages are compared with html.parser, whose HTML 5 table gives `lang` and `rang` other code points than
# HTML 4 does (U+27E8 / U+27E9 for U+2329 / U+232A): the two names are pinned by the entity test instead
_NAMES = sorted(set(ENTITIES) - {"lang", "rang"})
_SAFE_CP = [9, 10, 32, 0x21, 0x3C, 0x3E, 0x26, 0x7E, 0xA1, 0xE9, 0x24F, 0x4E00, 0x4E2D, 0x6587, 0xFFFD, 0x1F600, 0x10FFFD]


def _mixed_case(rng, name: str) -> str:
    return "".join(ch.upper() if rng.random() < 0.3 else ch for ch in name)


def _attrs(rng) -> str:
    out = ""
    for _ in range(rng.randrange(3)):
        key = rng.choice(["class", "id", "title", "href", "data-x"])
        if rng.random() < 0.5:
            out += ' %s="%s"' % (key, rng.choice(["a", "a>b", "it's", "x y", "a=b", "<i>", ""]))
        else:
            out += " %s='%s'" % (key, rng.choice(["a", "a>b", 'say "hi"', "x y", "a=b", "</p>", ""]))
    return out


def _reference(rng) -> str:
    r = rng.random()
    if r < 0.5:
        return "&%s;" % rng.choice(_NAMES)
    cp = rng.choice(_SAFE_CP)
    if r < 0.75:
        return "&#%d;" % cp
    return ("&#x%X;" if rng.random() < 0.5 else "&#X%x;") % cp


def _text_run(rng, words: int, utf8: bool = True, refs: bool = True) -> str:
    out = []
    for _ in range(words):
        r = rng.random()
        if r < 0.06 and refs:
            out.append(_reference(rng))
        elif r < 0.10 and utf8:
            out.append(rng.choice(_UTF8) * rng.randrange(1, 4))
        elif r < 0.12:
            out.append("1 < 2")
        else:
            out.append(rng.choice(_WORDS))
    return rng.choice([" ", "  ", "\n", " \t"]).join(out)


def _comment(rng) -> str:
    body = " "
    for _ in range(rng.randrange(5)):
        body += rng.choice(["note", ">", "<b>", "--x", "a -- b", "</p>", "->"]) + " "
    return "<!--" + body + "-->"


def _raw_element(rng) -> str:
    name = rng.choice(["script", "style"])
    body = " ".join(rng.choice(["if (a < b) {", "c > d", 'x = "</p>";', "</scripty>", "</styles>", "p > a { color: red }", "}"]) for _ in range(rng.randrange(6)))
    return "<%s%s>%s</%s%s>" % (_mixed_case(rng, name), _attrs(rng), body, _mixed_case(rng, name), rng.choice(["", " ", "\n"]))


def _element(rng, depth: int, words: int, utf8: bool, refs: bool) -> str:
    r = rng.random()
    if depth <= 0 or r < 0.35:
        return _text_run(rng, max(1, words), utf8, refs)
    if r < 0.42:
        return _comment(rng)
    if r < 0.47:
        return _raw_element(rng)
    if r < 0.55:
        return "<%s%s%s>" % (_mixed_case(rng, rng.choice(_VOID)), _attrs(rng), rng.choice(["", "/", " /"]))
    name = _mixed_case(rng, rng.choice(_INLINE if r < 0.78 else _BLOCK))
    inner = "".join(_element(rng, depth - 1, words, utf8, refs) for _ in range(rng.randrange(1, 4)))
    return "<%s%s>%s</%s>" % (name, _attrs(rng), inner, name)


def gen_page(rng, blocks: int = 6, words: int = 8, utf8: bool = True, refs: bool = True) -> str:
    """A well-formed page built from the constructs DESIGN.md T12 lists for the html.parser comparison: nested inline and
    block elements in mixed case, void tags with and without `/`, quoted attributes holding `>`, `"` and `'`, comments
    holding `>` and `--`, script and style bodies holding `<`, `>`, `</p>` and `</scripty>`, a DOCTYPE, a processing
    instruction, named, decimal and hex references with `;`, literal UTF-8, and `1 < 2`."""
    head = rng.choice(["<!DOCTYPE html>", "<!doctype html>\n", ""]) + rng.choice(['<?xml version="1.0"?>', "<?php x ?>", ""])
    body = "".join("<%s%s>%s</%s>\n" % (b, _attrs(rng), _element(rng, 3, words, utf8, refs), b)
                   for b in (_mixed_case(rng, rng.choice(_BLOCK)) for _ in range(blocks)))
    return head + "<html><body>" + body + "</body></html>"
