"""The planner of the multi-tenant search (ucfp_amd/csrc/multi_plan.h) is plain host code: drive it here, without a GPU, under
AddressSanitizer and UndefinedBehaviorSanitizer, against a naive model (tests/native/multi_plan_check.cpp).  The permutation
is a permutation; the segments partition it by tenant in stable order; every (query, row) pair lies in exactly one work item;
nq = 0 and 1, all tenants equal, all distinct, tenants without rows, sizes at the tile and chunk edges, and the refusals
(2^40 rows in a segment: more items than a 32-bit grid holds)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "multi_plan_check.cpp")


def test_multi_plan_against_a_model_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "multi_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
