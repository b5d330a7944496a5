"""GPU parity for the offline Haitsma extractor at its edges: the energy-chunk seam of the ragged
batch, clip tables past 1024 clips, the frame counts at which the single-stream path deals its frames differently, band
edges with empty, long and clamped bands, the rate limits, truncation by cap_frames, and calls that follow each other on
the shared workspace without a host synchronisation.  Every comparison is bit-exact against oracle.haitsma /
oracle.resample_linear; tests/test_haitsma_fp_spec.py holds the oracle itself against a float64 restatement, and its
prefix property is what lets the long cases here share one oracle run."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr

pytestmark = pytest.mark.gpu

SEAM = 131072                   # frames per energy chunk (4 * kChunkFrames in audio.hip)
FILL = 0x5A5A5A5A
E_MODALITY, E_INVALID = -1, -4


def _len(frames: int) -> int:
    """5 kHz samples that give exactly `frames` frames (and no sample more)."""
    return 2048 + 64 * (frames - 1)


def _first_len(frames: int, sr: int) -> int:
    """The shortest clip at `sr` whose 5 kHz image has `frames` frames: floor(n * 5000 / sr) >= _len(frames)."""
    return -(-_len(frames) * sr // 5000)


def _noise(n: int, seed: int) -> np.ndarray:
    return (0.2 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def long5k(oracle):
    """SEAM + 2 frames of noise at 5 kHz and their oracle frames: by the prefix property, the oracle of every prefix."""
    x = _noise(_len(SEAM + 2), 5)
    return x, oracle.haitsma(x, 5000)


@pytest.fixture(scope="module")
def filler8k(oracle):
    """A clip at 8 kHz whose oracle frame count F0 ends 12 frames short of the seam."""
    x = _noise(_first_len(SEAM - 12, 8000), 8)
    o = oracle.haitsma(x, 8000)
    assert o.size == SEAM - 12
    return x, o


class _Call:
    """One ucfp_audio_haitsma_batch_dev call in flight: the tensors it reads and writes stay alive here."""

    def results(self):
        """(per-clip frames, the whole d_out as uint32, d_out_offsets) -- synchronises."""
        oo = self.oo.cpu().numpy()
        out = self.out.cpu().numpy().view(np.uint32)
        return [out[oo[i]:oo[i + 1]] for i in range(self.n)], out, oo


def _prepare(torch, ctx, clips, sr, cfg=None, cap=None, guard=0, stream=None) -> _Call:
    """Uploads the batch and allocates its outputs on `stream` (default: the current one): d_out holds max(cap, 1) +
    guard words of FILL, d_out_offsets is prefilled with -1.  Nothing of the library runs yet."""
    from ucfp_amd import _lib
    arrs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
    offs = np.zeros(len(arrs) + 1, np.uint64)
    np.cumsum([a.size for a in arrs], out=offs[1:])
    k = _Call()
    k.ctx, k.sr, k.n, k.total = ctx, sr, len(arrs), int(offs[-1])
    k.cfg = cfg._c() if cfg is not None else None
    k.cap = int(_lib.load().ucfp_audio_haitsma_batch_max_frames(k.total, k.n, sr)) if cap is None else cap
    k.stream = stream or torch.cuda.current_stream()
    blob = np.concatenate(arrs) if k.total else np.zeros(1, np.float32)
    with torch.cuda.stream(k.stream):
        k.pcm = torch.from_numpy(blob).cuda()
        k.off = torch.from_numpy(offs.view(np.int64)).cuda()
        k.out = torch.full((max(k.cap, 1) + guard,), FILL, dtype=torch.int32, device="cuda")
        k.oo = torch.full((k.n + 1,), -1, dtype=torch.int64, device="cuda")
    return k


def _enqueue(k: _Call) -> _Call:
    """ucfp_audio_haitsma_batch_dev on the call's stream; returns without synchronising."""
    from ucfp_amd import _lib
    _lib.check(_lib.load().ucfp_audio_haitsma_batch_dev(
        k.ctx.handle, k.pcm.data_ptr(), k.off.data_ptr(), k.total, k.n, k.sr,
        C.byref(k.cfg) if k.cfg is not None else None, k.out.data_ptr(), k.cap, k.oo.data_ptr(), k.stream.cuda_stream or None))
    return k


def _launch(*args, **kwargs) -> _Call:
    return _enqueue(_prepare(*args, **kwargs))


def _same_batch(call: _Call, refs, what=None):
    """Each clip's frames and the whole d_out_offsets table equal the oracle's; nothing behind the last frame is written."""
    got, out, oo = call.results()
    want = np.zeros(len(refs) + 1, np.int64)
    np.cumsum([r.size for r in refs], out=want[1:])
    assert np.array_equal(oo, want), (what, oo[-4:], want[-4:])
    for i, (g, o) in enumerate(zip(got, refs)):
        assert np.array_equal(g, o), (what, i, o.size, int((g != o).sum()))
    assert (out[want[-1]:] == FILL).all(), what
    return want


# ---------------------------------------------------------------- single stream: frame counts at the dealing edges

@pytest.mark.parametrize("F", [1, 2, 7, 8, 9, 16, 17, 2047, 2048, 2049, 4097, SEAM - 1, SEAM, SEAM + 1, SEAM + 2])
def test_single_stream_frame_counts(gpu_ctx, long5k, F):
    """8 frames per workgroup, 256 workgroups (2048 frames) per sweep of the grid stride, 131 072 frames per energy chunk
    with one recomputed row of history behind it."""
    from ucfp_amd import audio
    x, o = long5k
    g = audio.haitsma_frames(x[:_len(F)], 5000, ctx=gpu_ctx)
    assert g.size == F and np.array_equal(g, o[:F]), (F, g.size)


@pytest.mark.parametrize("n,frames", [(0, 0), (2047, 0), (2048 + 63, 1)])
def test_single_stream_lengths_around_one_frame(gpu_ctx, long5k, n, frames):
    from ucfp_amd import audio
    x, o = long5k
    g = audio.haitsma_frames(x[:n], 5000, ctx=gpu_ctx)
    assert g.size == frames and np.array_equal(g, o[:frames])


# ---------------------------------------------------------------- batch: the chunk seam

SEAM_CASES = {
    "a: a clip's first frame at the seam": [_len(2), _len(5)],
    "b: a clip's second frame at the seam, zero-frame clips in front of it": [_len(1), 0, 2047, _len(4)],
    "c: the seam mid-clip": [_len(6)],
    "d: the second chunk is padding": [_len(2)],
    "e: the history row is padding": [_len(1)],
}


@pytest.mark.parametrize("case", list(SEAM_CASES), ids=lambda c: c[0])
def test_batch_across_the_chunk_seam(gpu_ctx, oracle, torch_cuda, long5k, case):
    """Clip 0 has 131 070 frames, so the clips behind it straddle the seam between the first and the second energy chunk:
    the second chunk recomputes the row of global frame 131 071 as its history, which is another clip's (a), the same
    clip's (b, c) or padding (e)."""
    x, o = long5k
    tail = [_noise(n, 100 + i) for i, n in enumerate(SEAM_CASES[case])]
    clips = [x[:_len(SEAM - 2)]] + tail
    refs = [o[:SEAM - 2]] + [oracle.haitsma(c, 5000) for c in tail]
    total = sum(r.size for r in refs)
    assert total == {"a": SEAM + 5, "b": SEAM + 3, "c": SEAM + 4, "d": SEAM, "e": SEAM - 1}[case[0]]
    call = _launch(torch_cuda, gpu_ctx, clips, 5000)
    assert call.cap > SEAM                      # the entry does walk a second chunk, whatever it holds
    want = _same_batch(call, refs, case)
    if case[0] == "a":
        assert want[2] == SEAM
    if case[0] == "b":
        assert want[4] + 1 == SEAM and want[2] == want[3] == want[4]


def test_batch_resampled_across_the_chunk_seam(gpu_ctx, oracle, torch_cuda, filler8k):
    """The same seam behind the batch resampler: the frames are cut from the workspace's 5 kHz copy, and the seam sits
    where the clips' own frame counts put it."""
    x, o = filler8k
    F0 = o.size
    assert F0 < SEAM
    short = [5, 0, 4, 3]
    assert F0 + sum(short) == SEAM
    lens = [_first_len(f, 8000) if f else 3000 for f in short] + [_first_len(4, 8000) + 1]
    tail = [_noise(n, 200 + i) for i, n in enumerate(lens)]
    refs = [o] + [oracle.haitsma(c, 8000) for c in tail]
    assert [r.size for r in refs[1:]] == short + [4]
    call = _launch(torch_cuda, gpu_ctx, [x] + tail, 8000)
    want = _same_batch(call, refs)
    assert want[5] == SEAM and want[6] == SEAM + 4      # the last clip's first frame is global frame 131 072


@pytest.mark.parametrize("lens", [[0], [0, 0, 0], [2047], [0, 2047, 1, 0]], ids=str)
def test_batch_without_a_frame(gpu_ctx, torch_cuda, lens):
    """No sample at all, or clips that are all too short: a table of zeros and no frame written."""
    call = _launch(torch_cuda, gpu_ctx, [_noise(n, 30 + n) for n in lens], 5000)
    _same_batch(call, [np.zeros(0, np.uint32)] * len(lens), lens)


# ---------------------------------------------------------------- batch: clip tables past one scan round

def _many_clips(n_clips: int, sr: int):
    rng = np.random.default_rng(n_clips)
    lens = rng.integers(0, 2301 * sr // 5000, n_clips)
    edge = [_first_len(1, sr) - 1, _first_len(1, sr), _first_len(2, sr) - 1, _first_len(2, sr)]   # 2047 2048 2111 2112 at 5 kHz
    for at in ((1022, 2046) if n_clips > 2049 else (1022,)):
        for j, n in enumerate(edge):
            if at + j < n_clips:
                lens[at + j] = n
    blob = _noise(int(lens.sum()), n_clips + 1)
    cuts = np.concatenate([[0], np.cumsum(lens)])
    return [blob[cuts[i]:cuts[i + 1]] for i in range(n_clips)]


@pytest.mark.parametrize("n_clips,sr", [(1023, 5000), (1024, 5000), (1025, 5000), (2500, 5000), (2500, 8000)])
def test_batch_of_more_than_1024_clips(gpu_ctx, oracle, torch_cuda, n_clips, sr):
    """The clip table is scanned 1024 clips per round with two running sums carried between the rounds; clips of 0, 1
    and 2 frames sit on both sides of every round's edge."""
    clips = _many_clips(n_clips, sr)
    refs = [oracle.haitsma(c, sr) for c in clips]
    sizes = [r.size for r in refs]
    assert sizes[1022] == 0 and (n_clips < 1026 or sizes[1023:1026] == [1, 1, 2])
    assert n_clips < 2500 or sizes[2046:2050] == [0, 1, 1, 2]
    assert sum(sizes) > n_clips // 16
    _same_batch(_launch(torch_cuda, gpu_ctx, clips, sr), refs, (n_clips, sr))


# ---------------------------------------------------------------- band edges

# the configurations of tests/test_haitsma_fp_spec.py (the last: bins 100 and 133 exactly) and three with (almost) every
# band empty
EDGE_CONFIGS = [(300.0, 2000.0), (1.0, 2500.0), (1.0, 40.0), (60.0, 2500.0), (2400.0, 2500.0),
                (5000.0 / 2048.0 * 100.0, 5000.0 / 2048.0 * 133.0), (1000.0, 1001.0), (2499.0, 2500.0), (1.0, 2.0)]
ALL_EMPTY = [(2499.0, 2500.0), (1.0, 2.0)]


@pytest.fixture(scope="module")
def ragged40():
    rng = np.random.default_rng(40)
    lens = rng.integers(0, 6000, 40)
    lens[:3] = [0, 2047, 2048]
    return [_noise(int(n), 400 + i) for i, n in enumerate(lens)]


@pytest.mark.parametrize("cfg", EDGE_CONFIGS, ids=lambda c: f"{c[0]:g}-{c[1]:g}")
def test_band_edges_on_the_device(gpu_ctx, oracle, ragged40, cfg):
    """Empty bands, a 216-bin band (the 8-wide summation loop and its tail), the clamp at bin 1024."""
    from ucfp_amd import audio
    c = audio.HaitsmaConfig(*cfg)
    x = _noise(15000, 41)
    o = oracle.haitsma(x, 5000, *cfg)
    g = audio.haitsma_frames(x, 5000, c, ctx=gpu_ctx)
    assert g.size == o.size == 1 + (15000 - 2048) // 64 and np.array_equal(g, o)
    got = audio.haitsma_frames_batch(ragged40, 5000, c, ctx=gpu_ctx)
    refs = [oracle.haitsma(clip, 5000, *cfg) for clip in ragged40]
    assert len(got) == 40 and sum(r.size for r in refs) > 200
    for i, (gi, oi) in enumerate(zip(got, refs)):
        assert gi.size == oi.size and np.array_equal(gi, oi), (cfg, i)
    if cfg in ALL_EMPTY:
        assert not g.any() and not np.concatenate(got).any()
    else:
        assert g.any()


# ---------------------------------------------------------------- rates

RATES = [1000, 4999, 5001, 11025, 22050, 48000, 96000, 384000]


@pytest.mark.parametrize("sr", RATES)
def test_rates(gpu_ctx, oracle, torch_cuda, sr):
    """Both entries from the batch entry's lowest rate (an upsampling by 5) to its highest, at the lengths around one
    frame."""
    from ucfp_amd import audio
    one = _first_len(1, sr)
    clips = [_noise(n, sr + i) for i, n in enumerate((0, 1, one, one - 1, sr // 2))]
    refs = [oracle.haitsma(c, sr) for c in clips]
    assert [r.size for r in refs] == [0, 0, 1, 0, 8]          # half a second is 2499 or 2500 samples at 5 kHz
    _same_batch(_launch(torch_cuda, gpu_ctx, clips, sr), refs, sr)
    for c, o in zip(clips, refs):
        g = audio.haitsma_frames(c, sr, ctx=gpu_ctx)
        assert g.size == o.size and np.array_equal(g, o), (sr, c.size)


def test_rate_limits(gpu_ctx, oracle, torch_cuda):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import ModalityError
    lib = _lib.load()
    x = _noise(4000, 9)
    for sr in (999, 384001, 0):
        with pytest.raises(ModalityError):
            audio.haitsma_frames_batch([x], sr, ctx=gpu_ctx)
        with pytest.raises(ModalityError):
            _launch(torch_cuda, gpu_ctx, [x], sr, cap=64)
        assert lib.ucfp_audio_haitsma_batch_max_frames(x.size, 1, sr) == 0
    torch_cuda.cuda.synchronize()
    # the single host entry takes any rate from 1 Hz on
    o = oracle.haitsma(x, 999)
    g = audio.haitsma_frames(x, 999, ctx=gpu_ctx)
    assert o.size == 1 + (4000 * 5000 // 999 - 2048) // 64 and np.array_equal(g, o)


# ---------------------------------------------------------------- the resampler entry

@pytest.mark.parametrize("sr_in,sr_out", [(8000, 5000), (5000, 8000), (1000, 5000), (384000, 5000), (7999, 8000),
                                          (44100, 44100)])
def test_resample_linear_dev(gpu_ctx, oracle, torch_cuda, sr_in, sr_out):
    from ucfp_amd import _lib
    torch = torch_cuda
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream or None
    x = _noise(65537, sr_in + sr_out)
    d_in = torch.from_numpy(x).cuda()
    for n in (0, 1, 2, 3, 1000, 65537):
        o = oracle.resample_linear(x[:n], sr_in, sr_out)
        m = n * sr_out // sr_in
        assert o.size == m == lib.ucfp_audio_resample_len(n, sr_in, sr_out)
        d_out = torch.full((m + 8,), 7.0, dtype=torch.float32, device="cuda")
        _lib.check(lib.ucfp_audio_resample_linear_dev(gpu_ctx.handle, d_in.data_ptr(), n, sr_in, sr_out, d_out.data_ptr(), m, st))
        torch.cuda.synchronize()
        g = d_out.cpu().numpy()
        assert g[:m].tobytes() == o.tobytes(), (sr_in, sr_out, n)
        assert (g[m:] == 7.0).all()
        if m:
            assert lib.ucfp_audio_resample_linear_dev(gpu_ctx.handle, d_in.data_ptr(), n, sr_in, sr_out, d_out.data_ptr(),
                                                      m - 1, st) == E_INVALID
    d_out = torch.zeros(64, dtype=torch.float32, device="cuda")
    for a, b in ((0, sr_out), (sr_in, 0), (384001, sr_out), (sr_in, 384001)):
        assert lib.ucfp_audio_resample_linear_dev(gpu_ctx.handle, d_in.data_ptr(), 8, a, b, d_out.data_ptr(), 64, st) == E_MODALITY
    torch.cuda.synchronize()
    assert not d_out.any().item()


# ---------------------------------------------------------------- truncation

def test_truncation(gpu_ctx, oracle, torch_cuda):
    """Frames past cap_frames are not written; d_out_offsets stays the full table."""
    from ucfp_amd import _lib
    torch = torch_cuda
    rng = np.random.default_rng(50)
    clips = [_noise(int(n), 500 + i) for i, n in enumerate(rng.integers(0, 7000, 50))]
    refs = [oracle.haitsma(c, 5000) for c in clips]
    flat = np.concatenate(refs)
    cap, guard = flat.size // 2 + 3, 64
    assert 100 < cap < flat.size - 100
    call = _launch(torch, gpu_ctx, clips, 5000, cap=cap, guard=guard)
    _, out, oo = call.results()
    want = np.zeros(51, np.int64)
    np.cumsum([r.size for r in refs], out=want[1:])
    assert np.array_equal(oo, want) and want[-1] == flat.size        # the table tells what was produced
    assert out.size == cap + guard and np.array_equal(out[:cap], flat[:cap])
    assert (out[cap:] == FILL).all()                                  # nothing from cap_frames on is touched
    # the single-stream device entry refuses a buffer that is one frame short, and writes nothing
    lib = _lib.load()
    x = clips[int(np.argmax([c.size for c in clips]))]
    F = 1 + (x.size - 2048) // 64
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.full((F + guard,), FILL, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream or None
    assert lib.ucfp_audio_haitsma_dev(gpu_ctx.handle, d_x.data_ptr(), x.size, None, d_out.data_ptr(), F - 1, st) == E_INVALID
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    _lib.check(lib.ucfp_audio_haitsma_dev(gpu_ctx.handle, d_x.data_ptr(), x.size, None, d_out.data_ptr(), F, st))
    torch.cuda.synchronize()
    g = d_out.cpu().numpy().view(np.uint32)
    assert np.array_equal(g[:F], oracle.haitsma(x, 5000)) and (g[F:] == FILL).all()


# ---------------------------------------------------------------- calls that follow each other without a host sync

def _stall(torch, stream):
    """Keeps `stream` busy for some milliseconds, so that the calls behind it are all enqueued before the first runs."""
    with torch.cuda.stream(stream):
        a = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
        for _ in range(100):
            a.mul_(1.0000001)
    return a


def test_two_configurations_back_to_back(gpu_ctx, oracle, torch_cuda, ragged40):
    """Every call copies its own 34 band edges to offset 0 of the shared workspace with an asynchronous copy out of one
    host array per thread: a call must not see the edges of the call behind it.  Inputs and outputs are on the device
    before the first call, and the host waits for nothing until all calls are enqueued."""
    from ucfp_amd import _lib, audio
    torch = torch_cuda
    lib = _lib.load()
    cfgs = [(300.0, 2000.0), (1.0, 2500.0), (2400.0, 2500.0)]
    refs = [[oracle.haitsma(c, 5000, *cfg) for c in ragged40] for cfg in cfgs[:2]]
    x = _noise(20000, 60)
    o3 = oracle.haitsma(x, 5000, *cfgs[2])
    assert not np.array_equal(np.concatenate(refs[0]), np.concatenate(refs[1]))
    assert not np.array_equal(o3, oracle.haitsma(x, 5000, *cfgs[1]))
    # one stream
    s = torch.cuda.Stream()
    k1 = _prepare(torch, gpu_ctx, ragged40, 5000, audio.HaitsmaConfig(*cfgs[0]), stream=s)
    k2 = _prepare(torch, gpu_ctx, ragged40, 5000, audio.HaitsmaConfig(*cfgs[1]), stream=s)
    with torch.cuda.stream(s):
        d_x = torch.from_numpy(x).cuda()
        d_o3 = torch.full((o3.size + 8,), FILL, dtype=torch.int32, device="cuda")
    c3 = audio.HaitsmaConfig(*cfgs[2])._c()
    keep = _stall(torch, s)
    _enqueue(k1)
    _enqueue(k2)
    _lib.check(lib.ucfp_audio_haitsma_dev(gpu_ctx.handle, d_x.data_ptr(), x.size, C.byref(c3), d_o3.data_ptr(), o3.size,
                                          s.cuda_stream))
    torch.cuda.synchronize()
    _same_batch(k1, refs[0], cfgs[0])
    _same_batch(k2, refs[1], cfgs[1])
    g3 = d_o3.cpu().numpy().view(np.uint32)
    assert np.array_equal(g3[:o3.size], o3) and (g3[o3.size:] == FILL).all()
    # two streams: the context's event orders the second call behind the first
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    k1 = _prepare(torch, gpu_ctx, ragged40, 5000, audio.HaitsmaConfig(*cfgs[0]), stream=s1)
    k2 = _prepare(torch, gpu_ctx, ragged40, 5000, audio.HaitsmaConfig(*cfgs[1]), stream=s2)
    torch.cuda.synchronize()
    keep = _stall(torch, s1)
    _enqueue(k1)
    _enqueue(k2)
    torch.cuda.synchronize()
    del keep
    _same_batch(k1, refs[0], ("two streams", cfgs[0]))
    _same_batch(k2, refs[1], ("two streams", cfgs[1]))


def test_workspace_is_shared_with_wang_and_panako(gpu_ctx, oracle, torch_cuda):
    """Haitsma, Wang, Panako, Haitsma on one context and one stream with no synchronisation in between: the shared
    workspace and the audio_done event keep every result intact (the Haitsma edge table lives at its offset 0)."""
    from ucfp_amd import _lib, audio
    torch = torch_cuda
    lib = _lib.load()
    clips = [pr.signal("chirps", 3.0, seed=21), pr.signal("noise", 4.0, seed=22)]
    offs = np.array([0, clips[0].size, clips[0].size + clips[1].size], np.int64)
    total = int(offs[-1])
    st = torch.cuda.current_stream().cuda_stream
    d_pcm = torch.from_numpy(np.concatenate(clips)).cuda()
    d_off = torch.from_numpy(offs).cuda()
    wcfg = audio.WangConfig()._c()
    wcap = int(lib.ucfp_audio_wang_batch_max_hashes(total, 2, 8000, C.byref(wcfg)))
    pcap = int(lib.ucfp_audio_panako_batch_max_hashes(total, 2, 8000, None))
    d_w = torch.zeros((wcap, 2), dtype=torch.int32, device="cuda")
    d_p = torch.zeros((pcap, 4), dtype=torch.int32, device="cuda")
    d_woo = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    d_poo = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    cfgs = [(300.0, 2000.0), (1.0, 2500.0)]
    h1 = _prepare(torch, gpu_ctx, clips, 8000, audio.HaitsmaConfig(*cfgs[0]))
    h2 = _prepare(torch, gpu_ctx, clips, 8000, audio.HaitsmaConfig(*cfgs[1]))
    _enqueue(h1)
    audio.wang_hashes_batch_dev(d_pcm.data_ptr(), d_off.data_ptr(), total, 2, 8000, d_w.data_ptr(), wcap, d_woo.data_ptr(),
                                None, st, gpu_ctx)
    audio.panako_hashes_batch_dev(d_pcm.data_ptr(), d_off.data_ptr(), total, 2, 8000, d_p.data_ptr(), pcap,
                                  d_poo.data_ptr(), None, st, gpu_ctx)
    _enqueue(h2)
    torch.cuda.synchronize()
    _same_batch(h1, [oracle.haitsma(c, 8000, *cfgs[0]) for c in clips], "first")
    _same_batch(h2, [oracle.haitsma(c, 8000, *cfgs[1]) for c in clips], "second")
    woo, poo = d_woo.cpu().numpy(), d_poo.cpu().numpy()
    w, p = d_w.cpu().numpy().view(np.uint32), d_p.cpu().numpy().view(np.uint32)
    assert woo[0] == 0 and poo[0] == 0 and woo[2] <= wcap and poo[2] <= pcap
    for i, c in enumerate(clips):
        ow, op = oracle.wang(c), pr.panako_ref(oracle, c)
        assert ow.shape[0] > 50 and op.shape[0] > 50
        assert np.array_equal(w[woo[i]:woo[i + 1]], ow), i
        assert np.array_equal(p[poo[i]:poo[i + 1]], op), i
