"""MinHash search, the parts that need no GPU: the numpy restatement against a scalar transcription of the
spec, the host function ucfp_minhash_agree against the restatement, the new symbols, and the `minhash` / `min_similarity`
fields of a query body."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import minhash_index_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ucfp_minhash_index_create", "ucfp_minhash_index_destroy", "ucfp_minhash_index_upsert",
           "ucfp_minhash_index_upsert_dev", "ucfp_minhash_index_delete", "ucfp_minhash_index_size",
           "ucfp_minhash_index_flush", "ucfp_minhash_index_query", "ucfp_minhash_index_query_dev", "ucfp_minhash_agree"]


def _scalar_agree(a: bytes, b: bytes) -> int:
    return sum(1 for i in range(128) if a[8 + 8 * i:16 + 8 * i] == b[8 + 8 * i:16 + 8 * i])


def _scalar_topk(ids, recs, query, k, min_agree):
    hits = []
    for i, r in zip(ids, recs):
        a = _scalar_agree(bytes(query), bytes(r))
        if a >= min_agree:
            hits.append((-a, int(i)))
    hits.sort()
    return [(i, -na) for na, i in hits[:k]]


def _small_records(rng, n):
    """Records whose slots come from two values per position, so agreements spread and tie."""
    base = rng.integers(0, 1 << 63, 128, dtype=np.uint64)
    pick = rng.integers(0, 2, (n, 128), dtype=np.uint64)
    return ref.records_of(base[None, :] ^ pick, header=rng.integers(0, 256, (n, 8), dtype=np.uint8))


def test_restatement_against_scalar_transcription():
    rng = np.random.default_rng(17)
    for _ in range(300):
        n, nq = int(rng.integers(0, 12)), int(rng.integers(1, 4))
        k, min_agree = int(rng.integers(1, 9)), int(rng.choice([0, 1, 60, 64, 70, 128]))
        recs = _small_records(rng, n + nq)
        rows, queries = recs[:n], recs[n:]
        if n and rng.integers(0, 2):
            rows[rng.integers(0, n)] = queries[0]          # an exact copy: agree = 128
        ids = rng.permutation(np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B1))
        A = ref.agree_matrix(queries, rows)
        g_ids, g_ag, g_sc, g_n = ref.topk_from_agree(ids, A, k, min_agree)
        for q in range(nq):
            want = _scalar_topk(ids.tolist(), rows, queries[q], k, min_agree)
            assert int(g_n[q]) == len(want)
            assert [(int(g_ids[q, j]), int(g_ag[q, j])) for j in range(len(want))] == want
            for j, (_, a) in enumerate(want):
                assert g_sc[q, j] == np.float32(a) / np.float32(128.0)
            assert (g_ids[q, len(want):] == ref.INVALID_ID).all() and (g_ag[q, len(want):] == ref.EMPTY32).all()
            assert (g_sc[q, len(want):] == -1.0).all()


def _pairs(rng, n):
    """n pairs of slot arrays [n, 128] built to cover the edge cases of the comparison; the first rows are the named ones."""
    a = rng.integers(0, 1 << 64, (n, 128), dtype=np.uint64)
    b = a.copy()
    # differences at a random subset of positions, each in one half of the slot only, or in both
    diff = rng.random((n, 128)) < rng.random((n, 1))
    kind = rng.integers(0, 3, (n, 128))
    flip = np.where(kind == 0, np.uint64(1) << rng.integers(0, 32, (n, 128)).astype(np.uint64),
                    np.where(kind == 1, np.uint64(1) << rng.integers(32, 64, (n, 128)).astype(np.uint64),
                             rng.integers(1, 1 << 64, (n, 128), dtype=np.uint64)))
    b ^= np.where(diff, flip, np.uint64(0))
    b[0] = a[0]                                             # equal records
    b[1] = a[1] ^ np.uint64(1 << 32)                        # every slot differs in the high dword only
    b[2] = a[2] ^ np.uint64(1)                              # every slot differs in the low dword only
    a[3], b[3] = np.uint64(0), np.uint64(0)                 # slot values 0 and 2^64 - 1
    a[4], b[4] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)
    a[5], b[5] = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
    b[6] = a[6]
    a[6, ::2], b[6, ::2] = np.uint64(0), np.uint64(0xFFFFFFFF)   # half the slots differ
    a[7] = np.arange(128, dtype=np.uint64) + np.uint64(1000)
    b[7] = np.roll(a[7], 1)                                 # the same values at other indexes: must not count
    b[8] = a[8][::-1]
    return a, b


def test_host_agree_against_restatement():
    from ucfp_amd import _lib, text
    lib = _lib.load()
    rng = np.random.default_rng(23)
    n = 20_000
    a, b = _pairs(rng, n)
    ra = ref.records_of(a, header=rng.integers(0, 256, (n, 8), dtype=np.uint8))    # differing headers must not matter
    rb = ref.records_of(b, header=rng.integers(0, 256, (n, 8), dtype=np.uint8))
    want = (ref.slots_of(ra) == ref.slots_of(rb)).sum(axis=1)
    assert want[0] == 128 and want[1] == 0 and want[2] == 0 and want[3] == 128 and want[4] == 128 and want[5] == 0
    assert want[6] == 64 and want[7] == 0
    assert len(set(want.tolist())) > 100                   # the pairs spread over the range
    pa, pb = ra.ctypes.data, rb.ctypes.data
    got = np.array([lib.ucfp_minhash_agree(pa + i * 1032, pb + i * 1032) for i in range(n)])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    assert lib.ucfp_minhash_agree(None, pb) == 0 and lib.ucfp_minhash_agree(pa, None) == 0
    A = ref.agree_matrix(ra[:40], rb[:40])
    assert np.array_equal(np.diag(A), want[:40])
    assert text.minhash_agree(ra[6].tobytes(), rb[6].tobytes()) == 64
    from ucfp_amd.errors import InvalidArgument
    with pytest.raises(InvalidArgument):
        text.minhash_agree(b"\0" * 1031, b"\0" * 1032)


def test_symbols_in_header_and_library():
    from ucfp_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ucfp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} is not declared in ucfp_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES
        # every entry point cites the design section
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*[a-z0-9_ ]*\b%s\s*\(" % s, hdr, flags=re.S)
        assert m and "A17" in m.group(1), f"{s} does not cite A17"


def _body(**kw):
    return dict({"tenant_id": 3, "modality": "Text", "k": 5}, **kw)


def test_query_request_minhash_forms():
    from ucfp_amd.core import HitSource, QueryRequest
    from ucfp_amd.errors import InvalidArgument
    assert HitSource.MinHash == "minhash"
    rec = bytes(np.random.default_rng(5).integers(0, 256, 1032, dtype=np.uint8))
    for form in (rec.hex(), rec.hex().upper(), list(rec), rec, bytearray(rec)):
        req = QueryRequest.from_json(_body(minhash=form))
        assert req.minhash == rec and req.min_similarity is None and req.k == 5 and req.tenant_id == 3
    req = QueryRequest.from_json(_body(minhash=rec.hex(), min_similarity=0.5, algorithm="minhash-lsh-h128"))
    assert req.min_similarity == 0.5 and req.algorithm == "minhash-lsh-h128"
    assert QueryRequest.from_json(_body(minhash=rec.hex(), min_similarity=1)).min_similarity == 1.0
    for bad in (rec.hex()[:-2], rec.hex() + "00", list(rec)[:-1], list(rec) + [0], rec[:-1], rec + b"\0", "", [],
                "zz" + rec.hex()[2:], rec.hex()[:-1] + "g", [256] + list(rec)[1:], [-1] + list(rec)[1:],
                [True] + list(rec)[1:], [1.0] + list(rec)[1:], 7, {"a": 1}):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json(_body(minhash=bad))
    for bad in (0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), "0.5", True, [0.5]):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json(_body(minhash=rec.hex(), min_similarity=bad))
    with pytest.raises(InvalidArgument):
        QueryRequest.from_json(_body(vector=[1.0, 0.0], min_similarity=0.5))        # only with `minhash`
    with pytest.raises(InvalidArgument):
        QueryRequest.from_json(_body(min_similarity=0.5))
    with pytest.raises(InvalidArgument):
        QueryRequest.from_json(_body(minhash=rec.hex(), algorithm="tlsh-128-1"))
    # bodies without the new fields parse as before
    req = QueryRequest.from_json(_body(vector=[1.0, 0.0]))
    assert req.minhash is None and req.min_similarity is None
