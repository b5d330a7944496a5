"""GPU parity for Panako triplets: every result of the HIP path (through the C ABI) has the shape and the
bytes of the numpy restatement in tests/panako_ref.py over the oracle's peaks."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr

pytestmark = pytest.mark.gpu

WIDE = dict(target_zone_t=512, target_zone_f=1024, peaks_per_sec=256, min_anchor_mag_db=-120.0)


def _cfg(audio, c: pr.Cfg):
    return audio.PanakoConfig(*c.astuple())


def _same(g, o, what=None):
    assert g.dtype == np.uint32 and g.shape == o.shape, (what, g.shape, o.shape)
    assert g.tobytes() == o.tobytes(), what


@pytest.mark.parametrize("kind,seconds", [("noise", 0.5), ("noise", 4.0), ("chirps", 10.0), ("sine440", 4.0),
                                          ("quiet", 1.0)])
def test_defaults_match_reference(gpu_ctx, oracle, kind, seconds):
    from ucfp_amd import audio
    x = pr.signal(kind, seconds, seed=int(seconds * 10))
    o = pr.panako_ref(oracle, x)
    g = audio.panako_hashes(x, 8000, ctx=gpu_ctx)
    _same(g, o, kind)
    if kind == "quiet":
        assert o.shape[0] == 0          # peaks exist, but none passes the anchor floor
    elif kind != "sine440" and seconds >= 4:
        assert o.shape[0] > 200


@pytest.mark.parametrize("n", [0, 1023, 1024])
def test_lengths_around_one_frame(gpu_ctx, oracle, n):
    from ucfp_amd import audio
    x = pr.signal("noise", 1.0, seed=n)[:n]
    _same(audio.panako_hashes(x, 8000, ctx=gpu_ctx), pr.panako_ref(oracle, x), n)


@pytest.fixture(scope="module")
def chirp_peaks(oracle):
    x = pr.signal("chirps", 6.0, seed=3)
    return x, pr.peaks(oracle, x, WIDE["peaks_per_sec"])


@pytest.mark.parametrize("fan_out", [1, 2, 3, 4, 6, 7, 10, 11, 55, 56, 64])
def test_fan_out_at_every_stored_target_count(gpu_ctx, chirp_peaks, fan_out):
    """C(m, 2) = 1, 3, 6, 10, 55, 66: the fan_out values at and after which one more stored target is needed."""
    from ucfp_amd import audio
    x, (t, k, p) = chirp_peaks
    c = pr.Cfg(fan_out, WIDE["target_zone_t"], WIDE["target_zone_f"], WIDE["peaks_per_sec"], WIDE["min_anchor_mag_db"])
    per = []
    o = pr.triplets(t, k, p, c, per)
    assert max(per) == fan_out                       # the cap is what is being tested
    _same(audio.panako_hashes(x, 8000, _cfg(audio, c), ctx=gpu_ctx), o, fan_out)


@pytest.mark.parametrize("cfg", [(5, 3, 2, 30, -50.0), (5, 8, 40, 256, -120.0)])
def test_tight_zones(gpu_ctx, oracle, cfg):
    """Zones that cut off most targets.  A peak is the maximum of its +-7 frame, +-15 bin neighbourhood (A5), so the
    zone (3, 2) lies inside it and admits nothing; (8, 40) reaches just past it and admits a few."""
    from ucfp_amd import audio
    c = pr.Cfg(*cfg)
    total = 0
    for kind, seconds in (("chirps", 10.0), ("noise", 4.0)):
        x = pr.signal(kind, seconds, seed=11)
        o = pr.panako_ref(oracle, x, c)
        wide = pr.panako_ref(oracle, x, pr.Cfg(5, 96, 96, c.peaks_per_sec, c.min_anchor_mag_db))
        assert o.shape[0] < wide.shape[0] // 4       # the zones cut off most targets
        total += o.shape[0]
        _same(audio.panako_hashes(x, 8000, _cfg(audio, c), ctx=gpu_ctx), o, kind)
    assert (total == 0) == (cfg[1] == 3)


def test_long_clip_spans_many_workgroups(gpu_ctx, oracle):
    from ucfp_amd import audio
    x = pr.signal("noise", 120.0, seed=12)
    t, k, p = pr.peaks(oracle, x, 30)
    assert t.size > 3000                             # count, scan and emit run over more than 256 peaks per pass
    _same(audio.panako_hashes(x, 8000, ctx=gpu_ctx), pr.triplets(t, k, p, pr.Cfg()))


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(300)
    secs = rng.uniform(0.0, 3.0, 300)
    return rng, secs


@pytest.mark.parametrize("sr", [8000, 44100])
def test_ragged_batch(gpu_ctx, oracle, torch_cuda, ragged, sr):
    """300 clips of 0 .. 3 s in one call: per-clip bytes (so no triplet crosses a clip and t is relative to its clip)
    and the per-clip offsets."""
    from ucfp_amd import _lib, audio
    torch = torch_cuda
    _, secs = ragged
    rng = np.random.default_rng(sr)
    lens = (secs * sr).astype(np.int64)
    one = -(-1024 * sr // 8000)                      # source samples that give exactly one 8 kHz frame
    lens[:3] = [0, one - 1, one] if sr != 8000 else [0, 1023, 1024]
    clips = []
    for i, n in enumerate(lens):
        tt = np.arange(int(n)) / sr
        x = 0.2 * rng.standard_normal(int(n)) if i % 2 else \
            0.3 * np.sin(2 * np.pi * (300 + 7 * i + 200 * tt) * tt) + 0.02 * rng.standard_normal(int(n))
        clips.append(x.astype(np.float32))
    ref = [pr.panako_ref(oracle, c if sr == 8000 else oracle.resample_linear(c, sr, 8000)) for c in clips]
    assert ref[0].shape[0] == 0 and ref[1].shape[0] == 0 and sum(r.shape[0] for r in ref) > 10_000
    got = audio.panako_hashes_batch(clips, sr, ctx=gpu_ctx)
    assert len(got) == len(clips)
    for i, (g, o) in enumerate(zip(got, ref)):
        _same(g, o, (sr, i, clips[i].size))
    # the offsets of the device entry itself
    offs = np.zeros(len(clips) + 1, np.uint64)
    np.cumsum([c.size for c in clips], out=offs[1:])
    cap = int(_lib.load().ucfp_audio_panako_batch_max_hashes(int(offs[-1]), len(clips), sr, None))
    d_pcm = torch.from_numpy(np.concatenate(clips)).cuda()
    d_off = torch.from_numpy(offs.view(np.int64)).cuda()
    d_out = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    d_oo = torch.full((len(clips) + 1,), -1, dtype=torch.int64, device="cuda")
    audio.panako_hashes_batch_dev(d_pcm.data_ptr(), d_off.data_ptr(), int(offs[-1]), len(clips), sr, d_out.data_ptr(), cap,
                                  d_oo.data_ptr(), None, torch.cuda.current_stream().cuda_stream, gpu_ctx)
    torch.cuda.synchronize()
    want = np.zeros(len(clips) + 1, np.int64)
    np.cumsum([r.shape[0] for r in ref], out=want[1:])
    assert np.array_equal(d_oo.cpu().numpy(), want)
    assert d_out.cpu().numpy().view(np.uint32)[: want[-1]].tobytes() == np.concatenate(ref).tobytes()


def test_truncation(gpu_ctx, oracle, torch_cuda):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import InvalidArgument
    torch = torch_cuda
    x = pr.signal("noise", 4.0, seed=40)
    o = pr.panako_ref(oracle, x)
    cap, guard = o.shape[0] // 2 + 1, 64
    assert 0 < cap < o.shape[0]
    lib = _lib.load()
    d_pcm = torch.from_numpy(x).cuda()
    d_out = torch.full((cap + guard, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(lib.ucfp_audio_panako_dev(gpu_ctx.handle, d_pcm.data_ptr(), x.size, 8000, None, d_out.data_ptr(), cap,
                                         d_n.data_ptr(), torch.cuda.current_stream().cuda_stream or None))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert int(d_n.item()) == o.shape[0]                         # the count stays exact
    assert out[:cap].tobytes() == o[:cap].tobytes()
    assert (out[cap:] == 0x5A5A5A5A).all()                       # nothing behind cap is touched
    host = audio._aligned_records(cap + guard)
    host[:] = 0x5A5A5A5A
    n = C.c_size_t(0)
    rc = lib.ucfp_audio_panako(gpu_ctx.handle, x.ctypes.data, x.size, 8000, None, host.ctypes.data, cap, C.byref(n))
    assert rc == -4 and n.value == o.shape[0]                    # UCFP_E_INVALID with the first cap records
    assert host[:cap].tobytes() == o[:cap].tobytes() and (host[cap:] == 0x5A5A5A5A).all()
    with pytest.raises(InvalidArgument):
        _lib.check(rc)


def test_rejections(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import InvalidArgument, ModalityError
    torch = torch_cuda
    x = pr.signal("sine440", 1.0, sr=44100)
    with pytest.raises(ModalityError, match="8 kHz"):            # src/server/tests.rs:391
        audio.panako_hashes(x, 44100, ctx=gpu_ctx)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream or None
    d_pcm = torch.from_numpy(x).cuda()
    d_out = torch.zeros((4096, 4), dtype=torch.int32, device="cuda")
    d_n = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(ModalityError, match="8 kHz"):
        _lib.check(lib.ucfp_audio_panako_dev(gpu_ctx.handle, d_pcm.data_ptr(), x.size, 44100, None, d_out.data_ptr(), 4096,
                                             d_n.data_ptr(), st))
    y = pr.signal("noise", 1.0, seed=2)
    for field, bad in (("fan_out", (0, 65)), ("target_zone_t", (0, 513)), ("target_zone_f", (0, 1025)),
                       ("peaks_per_sec", (0, 257)), ("min_anchor_mag_db", (-120.5, 0.5, float("nan")))):
        for v in bad:
            with pytest.raises(ModalityError, match="ranges"):
                audio.panako_hashes(y, 8000, audio.PanakoConfig(**{field: v}), ctx=gpu_ctx)
            with pytest.raises(ModalityError, match="ranges"):
                audio.panako_hashes_batch([y], 8000, audio.PanakoConfig(**{field: v}), ctx=gpu_ctx)
    for lo_hi in (dict(fan_out=1, target_zone_t=1, target_zone_f=1, peaks_per_sec=1, min_anchor_mag_db=-120.0),
                  dict(fan_out=64, target_zone_t=512, target_zone_f=1024, peaks_per_sec=256, min_anchor_mag_db=0.0)):
        audio.panako_hashes(y, 8000, audio.PanakoConfig(**lo_hi), ctx=gpu_ctx)      # the range ends are inside
    # output buffers must be 16-byte aligned
    d_y = torch.from_numpy(y).cuda()
    assert d_out.data_ptr() % 16 == 0
    with pytest.raises(InvalidArgument, match="16-byte"):
        _lib.check(lib.ucfp_audio_panako_dev(gpu_ctx.handle, d_y.data_ptr(), y.size, 8000, None, d_out.data_ptr() + 8, 4000,
                                             d_n.data_ptr(), st))
    d_off = torch.tensor([0, y.size], dtype=torch.int64, device="cuda")
    with pytest.raises(InvalidArgument, match="16-byte"):
        _lib.check(lib.ucfp_audio_panako_batch_dev(gpu_ctx.handle, d_y.data_ptr(), d_off.data_ptr(), y.size, 1, 8000, None,
                                                   d_out.data_ptr() + 4, 4000, d_n.data_ptr(), st))
    host = audio._aligned_records(4097)
    n = C.c_size_t(0)
    with pytest.raises(InvalidArgument, match="16-byte"):
        _lib.check(lib.ucfp_audio_panako(gpu_ctx.handle, y.ctypes.data, y.size, 8000, None, host.ctypes.data + 8, 4000,
                                         C.byref(n)))
    torch.cuda.synchronize()


def test_workspace_is_shared_with_wang(gpu_ctx, oracle):
    """Wang, Panako, Wang on one context and one stream: the shared workspace and the audio_done event keep every
    result intact."""
    from ucfp_amd import audio
    x = pr.signal("chirps", 5.0, seed=21)
    y = pr.signal("noise", 7.0, seed=22)
    w1 = audio.wang_hashes_batch([x, y], 8000, ctx=gpu_ctx)
    p = audio.panako_hashes_batch([y, x], 8000, ctx=gpu_ctx)
    w2 = audio.wang_hashes_batch([x, y], 8000, ctx=gpu_ctx)
    for got in (w1, w2):
        for g, c in zip(got, (x, y)):
            o = oracle.wang(c)
            assert g.shape == o.shape and np.array_equal(g, o)
    _same(p[0], pr.panako_ref(oracle, y))
    _same(p[1], pr.panako_ref(oracle, x))


def test_record_fields(gpu_ctx, oracle):
    from ucfp_amd import audio
    from ucfp_amd.core import Modality
    x = pr.signal("chirps", 4.0, seed=1)
    rec = audio.fingerprint_panako(x, 8000, 3, 9)
    assert rec.algorithm == "audiofp-panako-v1" and rec.format_version == 1 and rec.config_hash == 0   # audio.rs:141-155
    assert (rec.tenant_id, rec.record_id, rec.modality) == (3, 9, Modality.Audio)
    assert len(rec.fingerprint) % 16 == 0 and rec.fingerprint == pr.panako_ref(oracle, x).tobytes()
    assert len(rec.fingerprint) > 0
    c = pr.Cfg(7, 50, 60, 40, -60.0)
    rec2 = audio.fingerprint_panako_with(x, 8000, _cfg(audio, c), 3, 9)
    assert rec2.algorithm == "audiofp-panako-v1" and rec2.fingerprint == pr.panako_ref(oracle, x, c).tobytes()
