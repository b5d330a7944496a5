"""The PNG decoder on the device against deflate streams and filter rows that no encoder writes (tests/deflate_writer.py; what each
family covers is asserted in test_deflate_writer_spec.py).  Every file goes through image.decode_pngs; pixels are compared bit for
bit with the writer's expected image, which the oracle and Pillow confirm; a file that must be refused sits between two valid
files of different content, whose pixels are checked too -- the files' workspaces are neighbours on the device."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import deflate_writer as dw

pytestmark = pytest.mark.gpu


def _light(families):
    return [c.light() for c in dw.corpus() if c.family in families]


def _run(gpu_ctx, oracle, families, neighbours=()):
    from ucfp_amd import image
    cases = _light(families) + [c.light() for c in dw.corpus() if c.name in neighbours]
    for c in cases:
        if c["status"] == dw.OK:                       # (the oracle takes it: its pixels are the expected ones)
            rc, px = oracle.png_decode(c["png"])
            assert rc == oracle.PNG_OK and np.array_equal(px, c["pixels"]), c["name"]
    wrong = dw.check(image, gpu_ctx, cases)
    assert not wrong, wrong[:20]
    return cases


def test_f1_long_codes_and_wide_symbols(gpu_ctx, oracle):
    """Both codes 1, 2, ..., 14, 15, 15 bits long, the long ones on literals, on lengths and on distances in turn; a block of 43- to
    48-bit symbols at every bit phase (one 64-bit window per symbol must hold them)."""
    assert len(_run(gpu_ctx, oracle, {"F1"})) >= 7


def test_f2_block_seams_and_headers(gpu_ctx, oracle):
    """Hundreds of small blocks of every kind, runs of empty blocks starting at every bit phase, stored blocks of 1 .. 65 535 bytes
    behind every bit phase, dynamic headers run-length coded as zlib never does."""
    assert len(_run(gpu_ctx, oracle, {"F2"})) >= 6


def test_f3_window_and_match_list_geometry(gpu_ctx, oracle):
    """Every length x distance around the 2 KiB window and the three copy paths at every alignment; merged and unmerged runs of
    matches on every place of the lane and round seams of the token words; two-bit matches."""
    assert len(_run(gpu_ctx, oracle, {"F3"})) >= 36


def test_f4_invalid_streams_between_valid_neighbours(gpu_ctx, oracle):
    """One field wrong per stream: status -1, neighbours intact.  A lone code that is not one bit long goes to the host (1); its
    one-bit twin decodes (0)."""
    cases = _run(gpu_ctx, oracle, {"F4", "F4twin"}, neighbours=("f1_ladder_0_grey", "f1_wide", "f3_two_bit", "f2_seams_0_grey"))
    st = {c["name"]: c["status"] for c in cases}
    for kind in ("ll", "dist"):
        assert st[f"f4_lone_{kind}_code_1_bit"] == 0 and st[f"f4_lone_{kind}_code_2_bit"] == 1 and st[f"f4_lone_{kind}_code_15_bit"] == 1
    assert sum(1 for s in st.values() if s == -1) >= 31


def test_f5_filter_rows_of_every_type_size_and_layout(gpu_ctx, oracle):
    """Random filtered bytes (arbitrary residuals, Paeth ties) under chosen filter types: every type on row 0 and on the rows around the
    64-row hand-over, heights and widths around the 64-pixel block, all five file layouts; filter types 5 and 255 are refused."""
    cases = _run(gpu_ctx, oracle, {"F5"})
    assert sum(1 for c in cases if c["status"] == dw.BAD) == 8 and len(cases) >= 110


@pytest.mark.parametrize("n", [1300, 6100])
def test_streams_in_the_two_and_one_wave_shapes(gpu_ctx, oracle, n):
    """The two-pass form gives a file 4, 2 or 1 waves by the files of a launch (<= 1200 / <= 3000 / beyond), and a batch of 1600 or more
    decodes as two halves: the corpus tiled to 1300 files is one launch of two waves per file (256-bit subsequences), tiled to 6100 it
    is two launches of 3050 files, one wave per file."""
    from ucfp_amd import image
    wrong = dw.check(image, gpu_ctx, _light({"F1", "F2", "F3", "F4", "F4twin"}), tile=n)
    assert not wrong, wrong[:20]


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("png_streams") / "f1_f4.pickle"
    with open(p, "wb") as f:
        pickle.dump(_light({"F1", "F2", "F3", "F4", "F4twin"}), f)
    return str(p)


# (setting, tiles).  UCFP_PNG_TWO_PASS = 2 / 4 / 8 forces that many waves per file, 0 is the one-kernel form, and 1 leaves the choice to
# the batch size: four waves for the corpus as it is.  What runs, corpus untiled unless said:
#   png_huff_kernel<128, 4> <512, 2> <256, 8> <256, 4> (chain cap 1) <256, 4> (no warm-up) <128, 8> <512, 8>
#   png_huff_kernel<128, 1> and <512, 1>: one launch of 3100 files (UCFP_PNG_NO_SPLIT keeps the batch whole), besides <128, 4> and <512, 4>
#   png_inflate_kernel<RoundCfg<512>> (118 files), <RoundCfg<256>> (600), <RoundCfg<128>> (1100)
# <256, 2> and <256, 1> run in test_streams_in_the_two_and_one_wave_shapes, <256, 4> in the family tests.
SETTINGS = [({"UCFP_PNG_TWO_PASS": "1", "UCFP_PNG_HUFF_BITS": "128"}, []), ({"UCFP_PNG_TWO_PASS": "2", "UCFP_PNG_HUFF_BITS": "512"}, []),
            ({"UCFP_PNG_TWO_PASS": "8"}, []), ({"UCFP_PNG_TWO_PASS": "4", "UCFP_PNG_HUFF_MAX_ITER": "1"}, []),
            ({"UCFP_PNG_TWO_PASS": "4", "UCFP_PNG_HUFF_WARM": "0"}, []), ({"UCFP_PNG_TWO_PASS": "0"}, [600, 1100]),
            ({"UCFP_PNG_TWO_PASS": "8", "UCFP_PNG_HUFF_BITS": "128"}, []), ({"UCFP_PNG_TWO_PASS": "8", "UCFP_PNG_HUFF_BITS": "512"}, []),
            ({"UCFP_PNG_NO_SPLIT": "1", "UCFP_PNG_HUFF_BITS": "128"}, [3100]), ({"UCFP_PNG_NO_SPLIT": "1", "UCFP_PNG_HUFF_BITS": "512"}, [3100])]


@pytest.mark.parametrize("env,tiles", SETTINGS, ids=["-".join(f"{k[9:].lower()}{v}" for k, v in e.items()) for e, _ in SETTINGS])
def test_streams_in_every_instantiation(corpus_file, env, tiles):
    """F1 .. F4 through every instantiation of the inflate stage.  The switches are read once per process: a fresh child per setting,
    with a timeout of its own, never retried."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, 'tests'); import deflate_writer as dw; dw.child_main(sys.argv[1], [int(t) for t in sys.argv[2:]])"
    r = subprocess.run([sys.executable, "-c", code, corpus_file, *map(str, tiles)], cwd=root, env={**os.environ, **env},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (env, r.stdout[-1500:], r.stderr[-1500:])
