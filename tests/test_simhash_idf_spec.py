"""TF.IDF SimHash without a device: the host-only entries of the IDF block against the restatement
(tests/simhash_idf_ref.py), and the restatement against what it must reduce to."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from ucfp_amd import _lib

import simhash_idf_ref as ref
import text_grapheme_ref as gref

HERE = os.path.dirname(os.path.abspath(__file__))


def _edges():
    xs = list(range(1, 5001))
    for k in range(1, 64):
        xs += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    xs.append((1 << 64) - 1)
    rng = np.random.default_rng(23)
    xs += [int(v) for v in rng.integers(1, 1 << 63, 10_000, dtype=np.uint64)]
    xs += [int(v) | (1 << 63) for v in rng.integers(0, 1 << 63, 10_000, dtype=np.uint64)]
    return xs


def test_log2_q16_entry_equals_the_restatement():
    lib = _lib.load()
    for x in _edges():
        assert lib.ucfp_idf_log2_q16(x) == ref.log2_q16(x), x


def test_log2_q16_is_monotone_and_within_one_unit():
    prev = 0
    for x in range(1, 200_001):
        v = ref.log2_q16(x)
        assert v >= prev, x
        prev = v
    for x in _edges()[5000:] + list(range(1, 2000)):
        d = ref.log2_q16(x) - 65536 * math.log2(x)
        # float64 log2 of a 64-bit integer is good to ~1e-11 units at this scale: the bound is (-1, 0] with that slack
        assert -1 - 1e-6 < d <= 1e-6, (x, d)


def test_weight_q16_entry_equals_the_restatement():
    lib = _lib.load()
    big = (1 << 32) - 1
    pairs = [(0, 0), (1, 0), (1, 1), (10, 0), (10, 10), (10, 3), (big, 0), (big, big), (big, 1), (big, big - 1), (1000, 999)]
    for n, df in pairs:
        w = lib.ucfp_idf_weight_q16(n, df)
        assert w == ref.weight_q16(n, df), (n, df)
        assert w >= 0x10000, (n, df)
    assert ref.weight_q16(10, 10) == 0x10000
    assert abs(ref.weight_q16(10, 0) / 65536 - 4.459) < 1e-3
    rng = np.random.default_rng(5)
    for _ in range(2000):
        n = int(rng.integers(0, 1 << 40))
        df = int(rng.integers(0, n + 1))
        w = lib.ucfp_idf_weight_q16(n, df)
        assert w == ref.weight_q16(n, df) and w >= 0x10000


def test_token_key_entry_is_xxh3():
    lib = _lib.load()
    rng = np.random.default_rng(3)
    for n in range(0, 301):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert lib.ucfp_text_token_key(b, n) == gref.xxh3(b), n


def test_equal_weights_are_tf():
    rng = np.random.default_rng(11)
    for i in range(200):
        n = int(rng.integers(0, 40))
        toks = [bytes(rng.integers(97, 123, int(rng.integers(0, 6)), dtype=np.uint8)) for _ in range(n)]
        for w in (1, 0x10000, 0xFFFFFFFF):
            assert ref.simhash_weighted(toks, {}, w) == gref.simhash_tokens(toks), (i, w)


def test_restatement_rules():
    a, b, c = b"alpha", b"beta", b"gamma"
    ka, kb = ref.key(a), ref.key(b)
    # a tie clears the bit: two tokens of equal weight keep only the bits both have
    rec, st = ref.simhash_weighted([a, b], {}, 7)
    assert st == 0 and int.from_bytes(rec, "little") == ka & kb
    # weight 0 removes a token; only such tokens: no record
    assert ref.simhash_weighted([a, b], {kb: 0}, 5) == (ka.to_bytes(8, "little"), 0)
    assert ref.simhash_weighted([b, b], {kb: 0}, 5) == (bytes(8), -1)
    # fit: a token repeated in a document counts once, a document without tokens not at all
    n, df = ref.fit([[a, a, b], [a, c], None, [], [b""]])
    assert n == 2 and df == {ka: 2, kb: 1, ref.key(c): 1}


def test_host_entries_standalone_under_sanitizers(tmp_path):
    """tests/native/idf_log2_check.cpp: the host-only unit built as plain C++ with ASan + UBSan, its own main."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "idf_log2_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "native", "idf_log2_check.cpp"), os.path.join(root, "ucfp_amd", "csrc", "idf_host.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def test_idf_block_from_plain_c(tmp_path):
    """tests/c/idf_table.c: the IDF block compiles as C11; the host-only entries and the argument checks answer from a
    gcc-built driver."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(HERE)
    libdir = os.path.dirname(_lib.SO_PATH)
    exe = str(tmp_path / "idf_table")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"),
                        os.path.join(HERE, "c", "idf_table.c"), "-o", exe, "-L", libdir, "-l:libucfp_hip.so",
                        f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.split()[0::2] == ["log2_1", "log2_2", "log2_3", "log2_max", "weight_all", "weight_empty", "weight_unseen", "key_empty",
                                      "key_differs", "create_null_ctx", "add_null_table", "add_tokens_null_table", "set_null_table",
                                      "finalize_null_table", "size_null_table", "export_null_table", "simhash_null_ctx",
                                      "simhash_tokens_null_ctx"]
