"""Generates include/ucfp_text_utab.h: the code-point table behind text mode UCFP_TEXT_RAW_UTF8.

For every code point c below 0x20000 the table says whether c is COVERED (U1) and, if so, its canonical form
M(c) = Canonicalizer().apply(c) (NFKC + case fold + NFKC, Cf removed) together with what the tokeniser needs to know of
every canonical code point: its Word_Break class (U4), whether it is `str.isalnum`, and whether it is one of the vowels
of the `regex` module's apostrophe tailoring.  Classes and vowels are PROBED from `regex` (the module the host path
segments with), not copied from a list; every clause of U1 is asserted.

The table is bound to the versions of `unicodedata` and `regex` it was generated with; both are written into the header.

    python tools/gen_text_utab.py > include/ucfp_text_utab.h

Entry word (uint32), one per code point, reached through a two-stage table of 64-entry blocks:
    bit 31      covered
    bits 30-29  kind: 0 = M(c) is c itself, 1 = M(c) is the ONE code point in bits 16-0, 2 = M(c) is `len` (bits 19-17,
                0 .. 6, 0 for a deleted Cf) words of the pool starting at index bits 16-0
    bit 28      alnum   } of M(c) when it is one code point (kinds 0 and 1); zero for kind 2, whose pool words carry
    bit 27      vowel   } the flags of each canonical code point in the same bits, over the code point in bits 16-0
    bits 26-23  class   }
"""
import os
import sys
import unicodedata as U

import regex

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ucfp_amd.text import Canonicalizer, _host_tokens  # noqa: E402

LIMIT = 0x20000
SHIFT = 6
# class numbers of the canonical code points (U4); everything else is 0
CLASSES = ["Other", "ALetter", "Hebrew_Letter", "Numeric", "Katakana", "ExtendNumLet", "MidLetter", "MidNum", "MidNumLet",
           "Single_Quote", "Double_Quote"]
EXCLUDED = ["Extend", "Regional_Indicator"]
_PATS = {w: regex.compile(r"\p{WB=%s}" % w) for w in CLASSES[1:] + EXCLUDED}

B_COVERED, B_ALNUM, B_VOWEL, S_KIND, S_CLASS, S_LEN = 1 << 31, 1 << 28, 1 << 27, 29, 23, 17


def word_break(ch: str) -> str:
    for w, p in _PATS.items():
        if p.match(ch):
            return w
    return "Other"


def back_combiners():
    """Code points that can combine with what precedes them although their combining class is 0: the second element of a
    canonical decomposition pair, and the Hangul V / T jamo."""
    back = set()
    for cp in range(0x110000):
        d = U.decomposition(chr(cp))
        if d and not d.startswith("<"):
            parts = d.split()
            if len(parts) == 2:
                back.add(int(parts[1], 16))
    back.update(range(0x1161, 0x1176))
    back.update(range(0x11A8, 0x11C3))
    return back


def covered_map():
    """{c: M(c)} for every covered code point (U1)."""
    canon = Canonicalizer()
    back = back_combiners()

    def safe(ch):
        return U.combining(ch) == 0 and ord(ch) not in back

    m_of = {}
    for cp in range(LIMIT):
        ch = chr(cp)
        if U.category(ch) in ("Cn", "Cs", "Co"):
            continue
        m = canon.apply(ch)
        n1 = U.normalize("NFKC", ch)
        if not (safe(ch) and all(map(safe, n1)) and all(map(safe, n1.casefold())) and all(map(safe, m))):
            continue
        if any(word_break(x) in EXCLUDED for x in m):
            continue
        if len(m.encode()) > 3 * len(ch.encode()):
            continue
        if any(ord(x) >= LIMIT for x in m):
            continue
        m_of[cp] = m
    return m_of


def main():
    m_of = covered_map()
    canon = Canonicalizer()
    outputs = sorted({x for m in m_of.values() for x in m})
    # the clauses of U1 that the kernel and the restatement lean on
    for cp, m in m_of.items():
        if U.category(chr(cp)) == "Cf":
            assert m == "", hex(cp)
        assert len(m) <= 6, hex(cp)
        # The 4x bound of ucfp_text_canon_bound: a token costs its bytes and one separator.  Charge a token's separator to
        # the source code point that holds the token's first alphanumeric.  Context can only ADD joins (every clause of U4
        # is a no-boundary rule), so c is charged at most once per token of M(c) segmented on its own.
        ntok = len(_host_tokens(m)) if len(m) > 1 else 1
        assert len(m.encode()) + ntok <= 4 * len(chr(cp).encode()), hex(cp)
    for x in outputs:                       # M is idempotent on its outputs
        assert m_of.get(ord(x)) == x, hex(ord(x))
        assert canon.apply(x) == x
    assert all(m_of[c] == chr(c).lower() for c in range(0x80)), "ASCII is covered and only lower-cased"
    vowels = {x for x in outputs if _host_tokens("'" + x) == ["'" + x]}
    assert vowels == {x for x in outputs if _host_tokens("’" + x) == ["’" + x]}
    assert len(vowels) == 20, sorted(vowels)

    def flags(x):
        return (B_ALNUM if x.isalnum() else 0) | (B_VOWEL if x in vowels else 0) | (CLASSES.index(word_break(x)) << S_CLASS)

    pool, pool_at, entries = [], {}, [0] * LIMIT
    for cp, m in m_of.items():
        if m == chr(cp):
            entries[cp] = B_COVERED | flags(m)
        elif len(m) == 1:
            entries[cp] = B_COVERED | (1 << S_KIND) | flags(m) | ord(m)
        else:
            if m not in pool_at:
                pool_at[m] = len(pool)
                pool.extend(ord(x) | flags(x) for x in m)
            entries[cp] = B_COVERED | (2 << S_KIND) | (len(m) << S_LEN) | pool_at[m]
    assert len(pool) < (1 << S_LEN)
    blk = 1 << SHIFT
    stage1, stage2, seen = [], [], {}
    for b in range(LIMIT >> SHIFT):
        key = tuple(entries[b * blk:(b + 1) * blk])
        if key not in seen:
            seen[key] = len(seen)
            stage2.extend(key)
        stage1.append(seen[key])
    assert len(seen) < 65536

    def rows(vals, fmt, per):
        for i in range(0, len(vals), per):
            print("  " + ",".join(fmt % v for v in vals[i:i + per]) + ", \\")

    print("/* GENERATED by tools/gen_text_utab.py -- do not edit by hand. */")
    print("#ifndef UCFP_TEXT_UTAB_H")
    print("#define UCFP_TEXT_UTAB_H")
    print(f"/* Bound to python unicodedata {U.unidata_version} and regex {regex.__version__}: {len(m_of)} covered code points below")
    print(f" * 0x{LIMIT:X}, {len(outputs)} canonical code points, vowels of the apostrophe tailoring:")
    print(" * " + " ".join("U+%04X" % ord(v) for v in sorted(vowels)) + ".")
    print(" * Entry word of code point c = STAGE2[STAGE1[c >> SHIFT] << SHIFT | (c & (1 << SHIFT) - 1)]: bit 31 covered;")
    print(" * bits 30-29 kind (0: M(c) = c, 1: M(c) = the code point in bits 16-0, 2: bits 19-17 words of POOL from index")
    print(" * bits 16-0); bit 28 alnum, bit 27 vowel, bits 26-23 Word_Break class of M(c) for kinds 0 and 1.  A POOL word is")
    print(" * one canonical code point (bits 16-0) under the same three flag fields.  Classes: " +
          ", ".join(f"{i} {c}" for i, c in enumerate(CLASSES)) + ". */")
    print(f'#define UCFP_TEXT_UTAB_UNIDATA "{U.unidata_version}"')
    print(f'#define UCFP_TEXT_UTAB_REGEX "{regex.__version__}"')
    print(f"#define UCFP_TEXT_UTAB_COVERED {len(m_of)}u")
    print(f"#define UCFP_TEXT_UTAB_LIMIT 0x{LIMIT:X}u")
    print(f"#define UCFP_TEXT_UTAB_SHIFT {SHIFT}")
    print(f"#define UCFP_TEXT_UTAB_STAGE1_N {len(stage1)}")
    print(f"#define UCFP_TEXT_UTAB_STAGE2_N {len(stage2)}")
    print(f"#define UCFP_TEXT_UTAB_POOL_N {len(pool)}")
    print("#define UCFP_TEXT_UTAB_STAGE1_INIT { \\")
    rows(stage1, "%d", 32)
    print("}")
    print("#define UCFP_TEXT_UTAB_STAGE2_INIT { \\")
    rows(stage2, "0x%X", 16)
    print("}")
    print("#define UCFP_TEXT_UTAB_POOL_INIT { \\")
    rows(pool, "0x%X", 16)
    print("}")
    print("#endif")


if __name__ == "__main__":
    main()
