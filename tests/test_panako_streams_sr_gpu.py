"""Panako streams at any sample rate on the device: a set from ucfp_panako_streams_create_sr takes its feed
at 1 .. 384 kHz and emits, whatever the cutting, the record of ucfp_audio_panako_batch_dev at that rate byte for byte;
its live windows feed GpuIndex.identify_live.  The cases are shared with the Wang set (tests/wang_streams_sr_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr
import wang_streams_sr_cases as cases
from wang_streams_sr_cases import DENSE, GPU_RATES, WIDE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kind():
    return cases.Kind("panako")


@pytest.mark.parametrize("cfg", [dict(), DENSE, WIDE], ids=["default", "dense", "wide"])
@pytest.mark.parametrize("sr", GPU_RATES)
def test_cut_invariance(gpu_ctx, kind, sr, cfg):
    cases.cut_invariance(kind, gpu_ctx, sr, cfg)


def test_offline_reference_is_the_cpu_restatement(gpu_ctx, kind, oracle):
    """The reference of these tests against the CPU: panako_ref over oracle.resample_linear of the feed."""
    x = cases.feed(48000, 3.0, 2)
    got = kind.batch([x], 48000, ctx=gpu_ctx)[0]
    assert np.array_equal(got, pr.panako_ref(oracle, oracle.resample_linear(x, 48000, 8000)))


def test_one_sample_pushes_across_frame_and_second_boundaries(gpu_ctx, kind):
    cases.one_sample_pushes_at_44100(kind, gpu_ctx)


def test_pushes_that_release_no_sample(gpu_ctx, kind):
    cases.pushes_that_release_nothing(kind, gpu_ctx)


def test_create_sr_at_8000_is_the_old_set(gpu_ctx, kind):
    cases.same_as_old_entry_at_8000(kind, gpu_ctx)


def test_65_streams_at_different_phases(gpu_ctx, kind):
    cases.many_streams_at_different_phases(kind, gpu_ctx)


def test_slot_reuse_leaves_no_carried_input(gpu_ctx, kind):
    cases.slot_reuse(kind, gpu_ctx)


def test_failed_calls_change_nothing(gpu_ctx, kind, torch_cuda):
    cases.failed_calls_change_nothing(kind, gpu_ctx, torch_cuda)


def test_chunk_limit_counts_8k_samples_too(gpu_ctx, kind):
    cases.upsampled_chunk_limit(kind, gpu_ctx)


def test_create_sr_errors_on_a_device(gpu_ctx):
    from ucfp_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    for sr in (999, 384001):
        assert lib.ucfp_panako_streams_create_sr(gpu_ctx.handle, sr, None, 4, 0, C.byref(h)) == cases.UCFP_E_MODALITY
        assert b"sample rate" in lib.ucfp_last_error()
    assert lib.ucfp_panako_streams_create_sr(gpu_ctx.handle, 48000, None, 4, 8193, C.byref(h)) == cases.UCFP_E_INVALID
    assert lib.ucfp_panako_streams_create(gpu_ctx.handle, 48000, None, 4, 0, C.byref(h)) == cases.UCFP_E_MODALITY
    assert not h.value


@pytest.mark.parametrize("W", [63, 625])
def test_windows_follow_the_stream(gpu_ctx, kind, W):
    cases.windows_follow_the_stream(kind, gpu_ctx, W)


def test_identify_live_from_a_48000_feed(gpu_ctx, kind):
    cases.identify_live(kind, gpu_ctx, 48000)


def test_streaming_session_resamples_on_request(gpu_ctx, kind):
    cases.sessions(kind, gpu_ctx)
