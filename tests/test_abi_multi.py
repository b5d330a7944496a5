"""CPU-side checks of the multi-tenant search entries (DESIGN M1, M5): exported, declared in ucfp_hip.h and _lib.py, and a NULL
index or batcher is refused with UCFP_E_INVALID before any device call."""
import ctypes as C
import os
import re

from ucfp_amd import _lib, index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ucfp_index_search_multi", "ucfp_index_search_multi_dev", "ucfp_index_search_multi_limits",
       "ucfp_index_search_batcher_create_multi", "ucfp_index_search_batcher_submit_tenant")
E_INVALID = -4


def test_multi_symbols_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "ucfp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _lib.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), f"{s} is not declared in ucfp_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"


def test_multi_entries_refuse_null_handles_on_the_host():
    lib = _lib.load()
    t = (C.c_uint32 * 1)(0)
    q = (C.c_uint64 * 1)(0)
    ids = (C.c_uint64 * 1)(7)
    cnt = (C.c_uint32 * 1)(7)
    assert lib.ucfp_index_search_multi(None, t, q, 1, 1, ids, None, None, cnt) == E_INVALID
    assert b"index" in lib.ucfp_last_error()
    assert lib.ucfp_index_search_multi_dev(None, t, q, 1, 1, ids, None, None, cnt, None) == E_INVALID
    assert (ids[0], cnt[0]) == (7, 7)
    assert lib.ucfp_index_search_batcher_create_multi(None, 16, 0, C.byref(C.c_void_p())) == E_INVALID
    assert lib.ucfp_index_search_batcher_submit_tenant(None, 0, q, 1, ids, None, None, cnt) == E_INVALID


def test_multi_limits_are_host_constants():
    T, Q, cap = index.search_multi_limits()
    assert T >= 64 and Q >= 1 and cap >= 0
    lib = _lib.load()
    assert lib.ucfp_index_search_multi_limits(None, None, None) == 0
