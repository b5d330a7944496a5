"""MinHash with any slot count H, the parts that need no GPU: the restatement in tests/minhash_h_ref.py
against the oracle at H = 128, its prefix property, the host-only ucfp_minhash_agree_h and the validation of H."""
import ctypes as C

import numpy as np
import pytest

from ucfp_amd import _lib, index, text
from ucfp_amd.errors import InvalidArgument, UnsupportedError

import minhash_h_ref as ref

FOX = b"the quick brown fox jumps over the lazy dog"


def _ascii_tokens(oracle, doc: bytes):
    stream, nt = oracle.text_canon(doc, 0)
    assert nt >= 0
    return stream.split(b" ") if nt else []


def _random_ascii_docs(n, seed):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJ0123456789      .,'_:;-\n", np.uint8)
    return [alphabet[rng.integers(0, alphabet.size, int(rng.integers(0, 400)))].tobytes() for _ in range(n)]


def test_restatement_equals_the_oracle_at_128(oracle):
    docs = [FOX] + _random_ascii_docs(300, 1)
    for k in (1, 5):
        o_rec, o_st = oracle.text_minhash_batch(docs, mode=0, k=k)
        for i, d in enumerate(docs):
            rec, st = ref.minhash_tokens_h(_ascii_tokens(oracle, d), k, 128)
            assert st == int(o_st[i]), (i, d)
            assert rec == o_rec[i].tobytes(), (i, d)


def test_prefix_property_of_the_restatement(oracle):
    toks = _ascii_tokens(oracle, FOX * 7)
    full, st = ref.minhash_tokens_h(toks, 5, 1024)
    assert st == 0
    for h in (16, 64, 128, 144, 1024):
        rec, st = ref.minhash_tokens_h(toks, 5, h)
        assert st == 0 and len(rec) == 8 + 8 * h
        assert rec == full[:8 + 8 * h]
    assert ref.minhash_tokens_h([], 5, 144) == (bytes(8 + 8 * 144), -1)


@pytest.mark.parametrize("h", [16, 80, 1024])
def test_agree_h_is_host_code(h):
    lib = _lib.load()
    rng = np.random.default_rng(h)
    a = rng.integers(0, 2**64, h, dtype=np.uint64)
    for same in (0, 1, h // 3, h - 1, h):
        b = a ^ np.uint64(1)
        keep = rng.permutation(h)[:same]
        b[keep] = a[keep]
        ra = ref.records_of(a, h, header=rng.integers(0, 256, 8))[0].tobytes()    # the headers take no part
        rb = ref.records_of(b, h)[0].tobytes()
        assert ref.agree_h(ra, rb, h) == same
        assert int(lib.ucfp_minhash_agree_h(ra, rb, h)) == same
        assert text.minhash_agree(ra, rb) == same
    assert int(lib.ucfp_minhash_agree_h(None, rb, h)) == 0


def test_agree_h_at_128_is_the_old_entry():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, (40, 128), dtype=np.uint64)      # few values: many chance agreements
    b = rng.integers(0, 4, (40, 128), dtype=np.uint64)
    for ra, rb in zip(ref.records_of(a, 128), ref.records_of(b, 128)):
        ra, rb = ra.tobytes(), rb.tobytes()
        assert int(lib.ucfp_minhash_agree_h(ra, rb, 128)) == int(lib.ucfp_minhash_agree(ra, rb)) == ref.agree_h(ra, rb, 128)


@pytest.mark.parametrize("h", [0, 8, 17, 1040])
def test_invalid_slot_counts_are_refused_on_the_host(h):
    lib = _lib.load()
    rec = bytes(8 + 8 * 1040)
    assert int(lib.ucfp_minhash_agree_h(rec, rec, h)) == 0                 # a valid h would give h
    with pytest.raises(InvalidArgument):
        text.minhash_tokens([[b"a"]], 5, h=h)
    with pytest.raises(InvalidArgument):
        text.minhash_batch(["a b c"], text.TextOpts(h=h))
    with pytest.raises(InvalidArgument):
        text.minhash_bytes(h)
    with pytest.raises(InvalidArgument):
        index.MinHashIndex(0, ctx=object(), h=h)                           # refused before the context is looked at
    with pytest.raises(InvalidArgument):
        text.minhash_slots(bytes(8 + 8 * h))
    # the C entries: ctx comes first in the validation order, so a NULL ctx answers before h is looked at
    out = C.c_void_p()
    assert lib.ucfp_minhash_index_create_h(None, 0, h, C.byref(out)) == -4 and not out.value


def test_records_of_different_slot_counts_are_not_compared():
    with pytest.raises(InvalidArgument):
        text.minhash_agree(bytes(8 + 8 * 64), bytes(8 + 8 * 128))


def test_what_stays_at_128_says_so():
    for make in (lambda: text.StreamingMinHashSession(text.TextOpts(h=64), 1, 2),
                 lambda: text.dedup_corpus(["a b c"], 0.8, text.TextOpts(h=256)),
                 lambda: text.TextBatcher("minhash", text.TextOpts(h=64), ctx=object())):
        with pytest.raises(UnsupportedError, match="H = 128"):
            make()
    with pytest.raises(UnsupportedError, match="H = 128"):
        text._records(np.zeros((3, 8 + 8 * 64), np.uint8))
