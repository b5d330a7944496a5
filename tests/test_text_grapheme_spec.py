"""The grapheme tokeniser and caller-segmented tokens without a GPU: the restatement's device rule
(tests/text_grapheme_ref.py: one cluster per canonical code point, CR LF one, the G3 hand-back) against the host path it
must equal (`Canonicalizer.apply`, then \\X), the compiled grapheme set against G3 recomputed here, the token form
against the oracle's PRETOKENIZED mode, and the host-only entry points."""
import random
import unicodedata

import numpy as np
import pytest

import oracle
import text_canon_ref as canon_ref
import text_grapheme_ref as ref
from ucfp_amd import _lib

regex = pytest.importorskip("regex")


@pytest.fixture(scope="module", autouse=True)
def _versions():
    want = canon_ref.table_versions()
    have = (unicodedata.unidata_version, regex.__version__)
    if want != have:
        pytest.skip(f"the table is bound to unicodedata {want[0]} / regex {want[1]}; this interpreter has {have[0]} / {have[1]}")


@pytest.fixture(scope="module")
def g3():
    """(covered for graphemes, U1-covered but excluded), recomputed from `regex` for every code point."""
    good, excluded = [], []
    for cp in range(0x110000):
        r = canon_ref.lookup(cp)
        if r is None:
            continue
        (excluded if any(ref.gcb_excluded(chr(x)) for x in r[0]) else good).append(cp)
    return good, excluded


def test_grapheme_covered_equals_g3_for_every_code_point(g3):
    good, excluded = g3
    lib = _lib.load()
    goodset = set(good)
    for cp in range(0x110000):
        assert bool(lib.ucfp_text_grapheme_covered(cp)) == (cp in goodset), hex(cp)
    assert lib.ucfp_text_grapheme_covered(0x110000) == 0 and lib.ucfp_text_grapheme_covered(0xFFFFFFFF) == 0
    assert (len(good), len(excluded)) == (74935, 435)
    for cp in (0x0D4E, 0x111C2, 0x1100, 0x1160, 0x1176, 0x11C3, 0xA960, 0xD7B0):      # Prepend letters, L / V / T jamo
        assert cp in excluded, hex(cp)
    for cp in (0x0301, 0x1F1E6, 0x1161, 0x11A8):                                       # U1 already keeps these out
        assert canon_ref.lookup(cp) is None, hex(cp)
    for cp in (0x0D, 0x0A, 0x00, 0x20, 0xAD, 0xAC00, 0x4E00, 0xE9, 0xFB03):
        assert cp in goodset, hex(cp)


def test_device_rule_equals_the_host_clusters(g3):
    good, excluded = g3
    pools = canon_ref.class_pools()
    cf = [cp for cp in good if canon_ref.lookup(cp)[0] == ()]
    goodset = set(good)
    rng = random.Random(20261019)
    handed_back = 0
    for it in range(20_000):
        out = []
        for _ in range(rng.randint(0, 14)):
            r = rng.random()
            if r < 0.15:
                out.append(rng.choice("\r\n"))
            elif r < 0.25:
                out.append(rng.choice("aZ 0.\t\x00\x7f'"))
            elif r < 0.30:
                out.append(chr(rng.choice(cf)))
            elif r < 0.32:
                out.append(chr(rng.choice(excluded)))
            else:
                out.append(chr(rng.choice(rng.choice(pools))))
        s = "".join(out)
        got = ref.device_clusters(s.encode("utf-8"), ref.RAW_UTF8)
        if all(ord(ch) in goodset for ch in s):
            assert got == ref.host_clusters(s), [hex(ord(c)) for c in s]
        else:
            handed_back += 1
            assert got is None, [hex(ord(c)) for c in s]
    assert 1000 < handed_back < 10_000


def test_ascii_mode_is_the_utf8_mode_on_ascii_and_equals_the_host():
    rng = random.Random(7)
    for it in range(3000):
        doc = bytes(rng.choice(b"\r\n\r\nabcXYZ 09_.,'\x00\t\x7f") for _ in range(rng.randint(0, 20)))
        a = ref.device_clusters(doc, ref.RAW_ASCII)
        assert a == ref.device_clusters(doc, ref.RAW_UTF8) == ref.host_clusters(doc.decode("ascii")), doc
    assert ref.device_clusters(b"a\x80", ref.RAW_ASCII) is None
    assert ref.device_clusters(b"\r\n\n\r\r\n", ref.RAW_ASCII) == [b"\r\n", b"\n", b"\r", b"\r\n"]
    assert ref.device_clusters("\ufb03".encode(), ref.RAW_UTF8) == [b"f", b"f", b"i"]
    for bad in (b"\xc0\xaf", b"ab\xe6\x97", b"\xed\xa0\x80", "e\u0301".encode(), "\u1100".encode(), "\U0001F1E6".encode()):
        assert ref.device_clusters(bad, ref.RAW_UTF8) is None, bad


@pytest.mark.parametrize("k", [1, 2, 5, 64])
def test_token_form_equals_the_oracle_pretokenized_on_space_free_tokens(k):
    rng = random.Random(k)
    alphabet = "abcdefgh\u00e9\u65e5\x00\t.,"
    for n_tok in (0, 1, k - 1, k, k + 1, 3 * k + 7):
        toks = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 9))).encode("utf-8") for _ in range(n_tok)]
        doc = b" ".join(toks)
        o, st = oracle.text_minhash_batch([doc], mode=ref.PRETOKENIZED, k=k)
        assert ref.minhash_tokens(toks, k) == (o[0].tobytes(), int(st[0])), (k, n_tok)
        # empty tokens are no tokens, wherever they stand
        holes = [b""] + [t for tok in toks for t in (tok, b"")] + [b""]
        assert ref.minhash_tokens(holes, k) == (o[0].tobytes(), int(st[0]))
        o, st = oracle.text_simhash_batch([doc], mode=ref.PRETOKENIZED)
        assert ref.simhash_tokens(toks) == (o[0].tobytes(), int(st[0])), n_tok
        assert ref.simhash_tokens(holes) == (o[0].tobytes(), int(st[0]))


def test_a_token_may_hold_spaces_and_nuls():
    a, _ = ref.minhash_tokens([b"a b", b"c"], 2)
    b, _ = ref.minhash_tokens([b"a", b"b c"], 2)
    assert a == b                                      # G5: both shingles are the bytes "a b c" (the join is not injective)
    assert ref.minhash_tokens([b"a b", b"c"], 1)[0] != ref.minhash_tokens([b"a", b"b", b"c"], 1)[0]
    assert ref.simhash_tokens([b" "])[1] == 0 and ref.simhash_tokens([b"\x00"])[1] == 0
    assert ref.minhash_tokens([], 5) == (bytes(1032), ref.E_MODALITY) == ref.minhash_tokens([b"", b""], 5)


def test_host_only_entry_points_need_no_gpu():
    lib = _lib.load()
    to = np.array([0, 1, 3, 3, 7], np.uint64)
    dt = np.array([0, 2, 2, 4], np.uint64)
    assert lib.ucfp_text_tokens_validate(to.ctypes.data, dt.ctypes.data, 3) == 0
    assert lib.ucfp_text_tokens_validate(None, None, 0) == 0
    assert lib.ucfp_text_tokens_validate(None, dt.ctypes.data, 3) == -4
    bad = to.copy()
    bad[2] = 0                                        # a decreasing pair of token offsets
    assert lib.ucfp_text_tokens_validate(bad.ctypes.data, dt.ctypes.data, 3) == -4 and b"tok_offsets" in lib.ucfp_last_error()
    bad = dt.copy()
    bad[1] = 3                                        # a decreasing pair of document bounds
    assert lib.ucfp_text_tokens_validate(to.ctypes.data, bad.ctypes.data, 3) == -4 and b"doc_tokens" in lib.ucfp_last_error()
    # tokens outside [doc_tokens[0], doc_tokens[n]] are not the call's business
    sub = np.array([1, 3], np.uint64)
    weird = np.array([9, 1, 3, 3, 0], np.uint64)
    assert lib.ucfp_text_tokens_validate(weird.ctypes.data, sub.ctypes.data, 1) == 0
    # a NULL context is the caller's bug, before any device work
    assert lib.ucfp_text_minhash_batch_ex(None, None, None, 0, 0, 1, 5, None, None) == -4 and b"ctx" in lib.ucfp_last_error()
    assert lib.ucfp_text_simhash_batch_ex(None, None, None, 0, 0, 1, None, None) == -4
    assert lib.ucfp_text_minhash_batch_ex_dev(None, None, None, 0, 0, 1, 5, None, None, None) == -4
    assert lib.ucfp_text_simhash_batch_ex_dev(None, None, None, 0, 0, 1, None, None, None) == -4
    assert lib.ucfp_text_minhash_tokens_batch(None, None, None, None, 0, 5, None, None) == -4
    assert lib.ucfp_text_simhash_tokens_batch(None, None, None, None, 0, None, None) == -4
    assert lib.ucfp_text_minhash_tokens_batch_dev(None, None, None, None, 0, 5, None, None, None) == -4
    assert lib.ucfp_text_simhash_tokens_batch_dev(None, None, None, None, 0, None, None, None) == -4


def test_python_surface_without_a_gpu():
    from ucfp_amd import text
    from ucfp_amd.errors import UnsupportedError
    assert text.TextOpts(tokenizer="grapheme", k=3).tokenizer_tag() == "shingle-k=3/grapheme-uax29"
    for tok in ("cjk-jp", "cjk-ko"):
        with pytest.raises(UnsupportedError, match="minhash_tokens"):
            text._prepare("abc", text.TextOpts(tokenizer=tok))
    blob, to, dt = text._pack_tokens([[b"a b", b""], [], [b"\x00"]])
    assert to.tolist() == [0, 3, 3, 4] and dt.tolist() == [0, 2, 2, 3] and blob[:4].tobytes() == b"a b\x00"
    assert callable(text.minhash_tokens) and callable(text.simhash_tokens)


def test_token_tables_from_plain_c(tmp_path):
    """tests/c/text_tokens.c: the header's new entries compile as C11 and the host validation of the token tables, the
    grapheme set and the argument checks answer from a gcc-built driver."""
    import os
    import shutil
    import subprocess
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_lib.SO_PATH)
    exe = str(tmp_path / "text_tokens")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"),
                        os.path.join(root, "tests", "c", "text_tokens.c"), "-o", exe, "-L", libdir, "-l:libucfp_hip.so",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.split() == ["valid", "0", "empty", "0", "null", "-4", "tok_decreasing", "-4", "doc_decreasing", "-4", "slice", "0",
                                "tokens_null_ctx", "-4", "ex_null_ctx", "-4", "covered_a", "1", "covered_cr", "1",
                                "covered_hangul_syllable", "1", "covered_jamo_l", "0", "covered_prepend", "0", "covered_combining", "0"]
