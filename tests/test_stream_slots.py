"""The slot table of the stream sets (ucfp_amd/csrc/stream_slots.h) is plain host code: drive it here, without a GPU,
under AddressSanitizer and UndefinedBehaviorSanitizer, against a naive model (tests/native/stream_slots_check.cpp).  Same
verdict and message as the model for every acquire, release and slot list; the lowest free slot; nothing seen by a newly
acquired slot; `seen` all zero after every operation."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "stream_slots_check.cpp")


def test_stream_slots_against_a_model_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "stream_slots_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok") and "runtime error" not in r.stderr, r.stdout + r.stderr
