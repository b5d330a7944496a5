"""The integer rule of the resampling Wang / Panako stream sets (ucfp_amd/csrc/stream_resample.h) is plain
host code: drive it here, without a GPU, under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/native/wang_stream_sr_check.cpp).  Every read of the assemble step lands inside a carry buffer of carry_cap floats
or inside the chunk, and the assembled samples equal the offline resampler's bit for bit under random cuttings."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "wang_stream_sr_check.cpp")


def test_resample_plan_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "wang_stream_sr_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
