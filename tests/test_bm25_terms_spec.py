"""The BM25 terms rule without a device: the restatement (tests/bm25_terms_ref.py) against terms.tokenize on
ASCII, terms.term_key against the restatement's key over every XXH3 length class, the pair bound, and the checks that the
entries make before anything runs."""
import ctypes as C

import numpy as np
import pytest

import bm25_terms_ref as ref
from ucfp_amd import _lib, terms

E_INVALID = -4


def test_word_class_is_is_alphanumeric_on_ascii():
    for cp in range(128):
        assert ref.is_word(cp) == terms.is_alphanumeric(chr(cp)), cp
    assert not any(ref.is_word(b) for b in range(128, 256))


def test_tokens_equal_tokenize_on_ascii():
    rng = np.random.default_rng(23)
    alphabet = np.frombuffer(b"abcdefXYZ0123456789_'.:,; \t\n-@/\x00\x7f", np.uint8)
    seen = set()
    for i in range(2000):
        n = int(rng.integers(0, 120))
        doc = bytes(alphabet[rng.integers(0, alphabet.size, n)]) if i % 4 else bytes(rng.integers(0, 128, n, dtype=np.uint8))
        want = terms.tokenize(doc.decode("ascii"))
        assert [t.decode("ascii") for t in ref.tokens(doc)] == want, doc
        seen.update(doc)
    assert {ord(c) for c in "_'.9aZ"} <= seen
    assert ref.tokens(b"a_b it's 3.14 A1b2") == [b"a", b"b", b"it", b"s", b"3", b"14", b"a1b2"]


def test_term_key_is_the_restatement_key():
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789", np.uint8)
    for n in range(241):                              # XXH3: 0, 1-3, 4-8, 9-16, 17-128, 129-240
        t = bytes(letters[rng.integers(0, letters.size, n)])
        assert terms.term_key(t.decode("ascii")) == ref.key(t), n
    assert terms.term_key("straße") == ref.key("straße".encode("utf-8"))


def test_max_pairs_bounds_the_tokens_of_any_offset_table():
    lib = _lib.load()
    rng = np.random.default_rng(7)
    for _ in range(300):
        n = int(rng.integers(0, 40))
        lens = rng.integers(0, 50, n)
        if n and rng.random() < 0.3:
            lens[:] = 1                               # all odd: the bound is met exactly
        total = int(lens.sum())
        need = int(((lens + 1) // 2).sum())           # a document of len bytes has at most ceil(len / 2) tokens
        got = int(lib.ucfp_bm25_terms_max_pairs(total, n))
        assert got == (total + n) // 2 and got >= need, (lens, got, need)
    # the bound is reached: "a a a" style documents of odd length
    docs = [b"a", b"a b", b"a b c d e"]
    assert sum(len(ref.tokens(d)) for d in docs) == lib.ucfp_bm25_terms_max_pairs(sum(map(len, docs)), len(docs))


def test_argument_checks_need_no_device():
    lib = _lib.load()
    blob = (C.c_uint8 * 16)(*b"one two two 3.14")
    offs = np.array([0, 16], np.uint64)
    cap = int(lib.ucfp_bm25_terms_max_pairs(16, 1))
    keys, tfs = np.full(cap, 7, np.uint64), np.full(cap, 7, np.uint32)
    po, st = np.full(2, 7, np.uint64), np.full(1, 7, np.int32)
    fake = (C.c_uint8 * 4096)()                        # a non-NULL context that no check may look into
    ctx = C.addressof(fake)
    b, o, k, t, p, s = C.addressof(blob), offs.ctypes.data, keys.ctypes.data, tfs.ctypes.data, po.ctypes.data, st.ctypes.data

    def dev(ctx=ctx, b=b, o=o, n=1, nb=16, form=0, k=k, t=t, cap=cap, p=p, s=s):
        return lib.ucfp_bm25_terms_batch_dev(ctx, b, o, n, nb, form, k, t, cap, p, s, None)

    def host(ctx=ctx, b=b, o=o, n=1, form=0, k=k, t=t, cap=cap, p=p, s=s):
        return lib.ucfp_bm25_terms_batch(ctx, b, o, n, form, k, t, cap, p, s)

    for call in (dev, host):
        assert call(ctx=None, form=9, k=None, cap=0) == E_INVALID       # NULL ctx comes first ...
        assert b"ctx" in lib.ucfp_last_error()
        assert call(form=2) == E_INVALID and b"form" in lib.ucfp_last_error()
        assert call(form=-1) == E_INVALID
        assert call(cap=cap - 1) == E_INVALID and b"cap_pairs" in lib.ucfp_last_error()
        for name in ("b", "o", "k", "t", "p", "s"):
            assert call(**{name: None}) == E_INVALID, name
        assert call(form=1, t=None, cap=cap - 1) == E_INVALID           # SEQUENCE: tfs may be NULL, the bound still holds
    assert dev(n=1 << 31) == E_INVALID
    assert dev(nb=1 << 33, cap=1 << 40) == E_INVALID
    # nothing was written
    assert (keys == 7).all() and (tfs == 7).all() and (po == 7).all() and (st == 7).all()


def test_unknown_key_mode_is_refused_before_the_context():
    from ucfp_amd.errors import InvalidArgument
    from ucfp_amd.index import Bm25Index, GpuIndex
    with pytest.raises(InvalidArgument):
        Bm25Index(keys="bogus", ctx=object())
    with pytest.raises(InvalidArgument):
        Bm25Index(keys="bogus")
    with pytest.raises(InvalidArgument):
        GpuIndex(bm25_keys="bogus")
    with pytest.raises(InvalidArgument):
        terms.terms_batch(["a"], form="bogus")
