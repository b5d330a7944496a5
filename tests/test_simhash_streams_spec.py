"""SimHash streams without a GPU: the fixtures of tests/test_simhash_streams_gpu.py have the properties
those tests rely on (checked through the CPU oracle and simhash_idf_ref), the host-only entries answer, and the byte
limit of the header is the one ucfp_amd.text exposes."""
import ctypes as C
import os
import re

import numpy as np

import simhash_idf_ref as iref
import simhash_streams_fixtures as F
from ucfp_amd import _lib
from ucfp_amd import text as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tie_document(oracle):
    toks = iref.words(F.TIE_DOC, F.RAW)
    assert len(toks) == 2 and toks[0] != toks[1]
    differ = iref.key(toks[0]) ^ iref.key(toks[1])
    assert differ != 0
    rec, st = oracle.text_simhash_batch([F.TIE_DOC], F.RAW)
    assert st[0] == 0
    bits = int.from_bytes(rec[0].tobytes(), "little")
    assert bits & differ == 0                                   # a tie clears the bit
    assert bits == iref.key(toks[0]) & iref.key(toks[1])        # the other bits: both set, or both clear
    ref_rec, ref_st = F.expected_ref([F.TIE_DOC], F.RAW)
    assert ref_st[0] == 0 and np.array_equal(ref_rec, rec)      # the two restatements agree on the TF record


def test_zero_and_wide_documents():
    weights, default = F.ZERO_WEIGHTS
    toks = iref.words(F.ZERO_DOC, F.RAW)
    assert toks and all(weights.get(iref.key(t), default) == 0 for t in toks)
    assert iref.simhash_weighted(toks, weights, default) == (bytes(8), F.E_MODALITY)
    wide = iref.words(F.wide_doc(), F.RAW)
    heavy, default = F.weights_for([wide], share=1.0, heavy=True)
    assert 2000 <= len(wide) <= 4000 and all(heavy[iref.key(t)] == F.W_MAX for t in wide)
    tot = sum(heavy[iref.key(t)] for t in wide)
    pos = [sum(heavy[iref.key(t)] for t in wide if (iref.key(t) >> b) & 1) for b in range(64)]
    assert tot > 1 << 32 and sum(p > 1 << 32 for p in pos) >= 32 and tot < 1 << 63
    assert any(p & 0xFFFFFFFF for p in pos) and tot & 0xFFFFFFFF    # both halves carry bits
    rec, st = iref.simhash_weighted(wide, heavy, default)
    assert st == 0
    assert F.expected_ref([F.wide_doc()], F.RAW)[0][0].tobytes() == rec   # equal non-zero weights: the TF record


def test_flush_documents_and_long_tokens(oracle):
    docs, chunked = F.flush_docs()
    assert len(docs) == 9
    for d, c in zip(docs, chunked):
        assert b"".join(c) == d
    for d, c in zip(docs[:8], chunked[:8]):
        assert len(d) == 8192 and len(iref.words(d, F.RAW)) > 256
        assert c.count(b"") == 3 and c[3] == c[4] == c[-2] == b"" and c[-1] != b""    # empty non-final pushes, two in a row
    assert [len(c[0]) for c in chunked[:7]] == [63, 64, 65, 255, 256, 257, 1535]
    long_doc = docs[8]
    toks = iref.words(long_doc, F.RAW)
    assert len(toks[3]) == F.LONG_TOKEN_BYTES == 1000 and long_doc[F.LONG_TOKEN_AT:F.LONG_TOKEN_AT + 1000] == toks[3]
    spans = [x for x in range(0, len(long_doc), F.LONG_TOKEN_CHUNK)
             if x < F.LONG_TOKEN_AT + 1000 and x + F.LONG_TOKEN_CHUNK > F.LONG_TOKEN_AT]
    assert len(spans) == 4
    assert T.MAX_WINDOW_BYTES == iref.MAX_WINDOW_BYTES == F.WINDOW_TOKEN_BYTES["ok"] == 1405
    for name, d in F.window_docs().items():
        stream, ntok = oracle.text_canon(d, F.RAW)
        longest = max(len(t) for t in stream.split(b" "))
        assert ntok > 0 and longest == F.WINDOW_TOKEN_BYTES[name]
        assert d[F.WINDOW_HEAD:F.WINDOW_HEAD + longest] == max(stream.split(b" "), key=len)
    assert F.WINDOW_TOKEN_BYTES["over"] > 1536 >= F.WINDOW_TOKEN_BYTES["between_hi"] > F.WINDOW_TOKEN_BYTES["between_lo"] > 1405


def test_weight_tables_cover_about_seventy_percent():
    toks = [iref.words(F.EDGE_DOC, F.RAW)]
    weights, default = F.weights_for(toks)
    assert default == F.Q16_ONE and 0.55 <= F.weighted_share(toks, weights) <= 0.85
    assert any(w == 0 for w in weights.values()) and len(set(weights.values())) > 5
    rec_w, st_w = F.expected_ref([F.EDGE_DOC], F.RAW, weights, default)
    rec_tf, st_tf = F.expected_ref([F.EDGE_DOC], F.RAW)
    assert st_w[0] == st_tf[0] == 0 and not np.array_equal(rec_w, rec_tf)     # the table changes the record
    assert iref.words(F.MIXED.encode("utf-8"), F.UTF8) is not None               # the device covers the mixed-script text


def test_host_only_entries_need_no_gpu():
    lib = _lib.load()
    tf, idf = lib.ucfp_text_streams_state_bytes_sim(0, 0), lib.ucfp_text_streams_state_bytes_sim(0, 1)
    assert 1536 + 64 * 4 < tf < idf < lib.ucfp_text_streams_state_bytes()        # less than a MinHash stream carries
    assert idf - tf == 64 * 4                                                    # 64-bit sums instead of 32-bit counts
    canon = lib.ucfp_text_streams_state_bytes_ex(T.STREAMS_UTF8) - lib.ucfp_text_streams_state_bytes_ex(0)
    for weighted, base in ((0, tf), (1, idf)):
        assert lib.ucfp_text_streams_state_bytes_sim(T.STREAMS_UTF8, weighted) == base + canon
    assert lib.ucfp_text_streams_record_bytes(None) == 0
    assert lib.ucfp_text_streams_state_bytes() == lib.ucfp_text_streams_state_bytes_ex(0)     # the MinHash values stand
    # creation checks its arguments before it needs a device
    h = C.c_void_p()
    assert lib.ucfp_text_streams_create_sim(None, 4, 6, 4096, None, C.byref(h)) == -4 and b"flags" in lib.ucfp_last_error()
    assert lib.ucfp_text_streams_create_sim(None, 4, T.STREAMS_UTF8, 0, None, C.byref(h)) == -4
    assert b"max_push_bytes" in lib.ucfp_last_error()
    assert lib.ucfp_text_streams_create_sim(None, 4, 0, 0, None, None) == -4 and b"out" in lib.ucfp_last_error()
    assert lib.ucfp_text_streams_create_sim(None, 4, 0, 0, None, C.byref(h)) in (-3, -4) and not h.value


def test_byte_limit_constant():
    hdr = open(os.path.join(ROOT, "include", "ucfp_hip.h")).read()
    m = re.search(r"#define\s+UCFP_TEXT_SIMHASH_STREAM_LIMIT_BYTES\s+(0x[0-9a-fA-F]+|\d+)", hdr)
    assert m and int(m.group(1), 0) == T.SIMHASH_STREAM_LIMIT_BYTES == 1 << 30
    # the derivation: n bytes -> at most 4 n canonical bytes -> at most (4 n + 1) // 2 tokens, and 2 x count fits 32 bits
    n = T.SIMHASH_STREAM_LIMIT_BYTES - 1
    tokens = (int(_lib.load().ucfp_text_canon_bound(n)) + 1) // 2
    assert tokens < 1 << 31 and 2 * tokens < 1 << 32 and tokens * F.W_MAX < 1 << 63
    assert (int(_lib.load().ucfp_text_canon_bound(n + 1)) + 1) // 2 >= 1 << 31       # and no larger limit would do
