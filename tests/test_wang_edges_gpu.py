"""The Wang kernels (wang_stream_kernel -> wang_select_kernel -> wang_pair_kernel, and the stream and
Panako paths that share that front end) against `oracle.wang`, bit for bit, on the clips of tests/wang_cases.py: rows
with 32 candidates, seconds with 256 peaks, ranks decided by the (t, k) tie rule, equal cells at the edges of the
neighbourhood, targets at the edges of the zone, anchors at the floor, NaN / Inf / denormal input, truncation and
config rejection.  tests/test_wang_peaks_spec.py holds the oracle to a numpy restatement on the same clips."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr
import wang_cases as wc

pytestmark = pytest.mark.gpu

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4
FILL = 0x5A5A5A5A

DEFAULT = dict(fan_out=10, target_zone_t=63, target_zone_f=64, peaks_per_sec=30, min_anchor_mag_db=-50.0)
WIDE = dict(DEFAULT, fan_out=64, target_zone_t=512, target_zone_f=1024, min_anchor_mag_db=-200.0)
WIDE256 = dict(WIDE, peaks_per_sec=256)
NOFLOOR256 = dict(WIDE256, min_anchor_mag_db=-1000.0)       # the floor power underflows to 0: every peak is an anchor


def _ocfg(oracle, cfg):
    c = dict(DEFAULT, **cfg)
    return oracle.WangCfg(c["fan_out"], c["target_zone_t"], c["target_zone_f"], c["peaks_per_sec"], c["min_anchor_mag_db"])


_REF = {}


def _ref(oracle, x, cfg, key=None):
    """oracle.wang, computed once per (clip, config) of the module and never changed."""
    c = dict(DEFAULT, **cfg)
    key = (key if key is not None else id(x), tuple(sorted(c.items())))
    if key not in _REF:
        o = oracle.wang(x, _ocfg(oracle, c))
        o.setflags(write=False)
        _REF[key] = (o, x)                     # (the clip is kept alive with its id)
    return _REF[key][0]


def _same(g, o, what=None):
    assert g.dtype == np.uint32 and g.shape == o.shape, (what, g.shape, o.shape)
    bad = np.nonzero((g != o).any(axis=1))[0]
    assert bad.size == 0, (what, bad.size, bad[:4], g[bad[:4]], o[bad[:4]])


def _check(gpu_ctx, oracle, x, cfg, what=None):
    from ucfp_amd import audio
    o = _ref(oracle, x, cfg)
    _same(audio.wang_hashes(x, 8000, audio.WangConfig(**dict(DEFAULT, **cfg)), ctx=gpu_ctx), o, what)
    return o


# ---------------------------------------------------------------- density and ties

@pytest.mark.parametrize("zones", ["wide", "t64"])
@pytest.mark.parametrize("pps", [1, 30, 31, 255, 256])
@pytest.mark.parametrize("name", list(wc.LATTICES))
def test_dense_lattices_and_the_rank_rule(gpu_ctx, oracle, name, pps, zones):
    """32 candidates in a row, 256 in a second; on lattice_tied the survivors of the per-second cap are chosen by
    (t, k) alone, on lattice_distinct by the power alone, on lattice_partial by both."""
    cfg = dict(WIDE, peaks_per_sec=pps) if zones == "wide" else dict(DEFAULT, target_zone_t=64, peaks_per_sec=pps)
    o = _check(gpu_ctx, oracle, wc.LATTICES[name](), cfg, (name, pps, zones))
    if zones == "wide" and pps >= 30:
        assert o.shape[0] >= 30 * pps           # 3 s, and nearly every peak finds 64 targets or all the later peaks


def test_tied_lattice_under_the_defaults_has_no_hashes(gpu_ctx, oracle):
    """The 30 tied survivors of a second are its first 30 in (t, k) order: one row, so no pair with dt > 0."""
    o = _check(gpu_ctx, oracle, wc.lattice_tied(), DEFAULT)
    assert o.shape[0] == 0
    assert _ref(oracle, wc.lattice_tied(), dict(DEFAULT, peaks_per_sec=33)).shape[0] > 0   # a second row: pairs


# ---------------------------------------------------------------- neighbourhood edges

@pytest.mark.parametrize("cfg", [DEFAULT, WIDE256], ids=["default", "wide256"])
@pytest.mark.parametrize("clip", [f"period{p}" for p in wc.PERIODS] + [f"comb{p}" for p in wc.COMB_PERIODS])
def test_equal_cells_at_the_neighbourhood_edges(gpu_ctx, oracle, clip, cfg):
    """Bit-identical frames 7 frames apart (the later one loses), 8 and 9 apart (both stand); equal cells exactly 16 bins
    apart in one row (both stand)."""
    x = wc.period(int(clip[6:])) if clip.startswith("period") else wc.comb(int(clip[4:]))
    _check(gpu_ctx, oracle, x, cfg, clip)


@pytest.mark.parametrize("cfg", [DEFAULT, WIDE256], ids=["default", "wide256"])
@pytest.mark.parametrize("frames", [47, 48, 49, 55, 56, 57, 96, 97])
def test_segment_seams_under_ties(gpu_ctx, oracle, frames, cfg):
    """Segments of 48 frames, rounds of 12, a halo of 7: the comb's frames tie with frames of the neighbouring
    segment, and its peak rows have 32 candidates."""
    x = wc.comb(1024, frames)
    assert wc.frames_of(x.size) == frames
    o = _check(gpu_ctx, oracle, x, cfg, frames)
    assert cfg is DEFAULT or o.shape[0] > 1000


# ---------------------------------------------------------------- zone edges, anchor floor

ZONES = list(wc.ZONES)


def _zone_cfg(z):
    return dict(fan_out=z[0], target_zone_t=z[1], target_zone_f=z[2], peaks_per_sec=z[3], min_anchor_mag_db=z[4])


@pytest.fixture(scope="module")
def zone_counts(oracle):
    """Hash counts of the oracle: the 7-versus-8 frame and the 15-versus-16 bin configs must differ."""
    n = {z: _ref(oracle, wc.lattice_distinct(), _zone_cfg(z)).shape[0] for z in ZONES}
    assert n[(64, 7, 15, 256, -200.0)] == 0 < n[(64, 8, 15, 256, -200.0)] < n[(64, 8, 16, 256, -200.0)]
    assert n[(1, 512, 1, 256, -200.0)] > 600 and n[(64, 512, 1024, 256, -200.0)] > 40000
    return n


@pytest.mark.parametrize("z", ZONES, ids=[f"fan{z[0]}-t{z[1]}-f{z[2]}" for z in ZONES])
def test_targets_at_the_zone_edges(gpu_ctx, oracle, zone_counts, z):
    o = _check(gpu_ctx, oracle, wc.lattice_distinct(), _zone_cfg(z), z)
    assert o.shape[0] == zone_counts[z]
    if z[1] <= 8 and o.shape[0]:
        assert ((o[:, 0] & 0x3FFF) == 8).all()               # every pair sits exactly on the zone's last frame


@pytest.fixture(scope="module")
def floor_dbs(oracle):
    """+30 dB (no anchor), -200 dB (every anchor), and a float32 dB whose floor power falls between two adjacent peak
    powers near the median of lattice_distinct: derived in float64 from their midpoint."""
    x = wc.lattice_distinct()
    db = wc.mid_floor_db(oracle)
    dbs = {"+30": 30.0, "mid": db, "-200": -200.0}
    n = {k: _ref(oracle, x, dict(WIDE256, min_anchor_mag_db=v)).shape[0] for k, v in dbs.items()}
    assert n["+30"] == 0 < n["mid"] < n["-200"], n
    return dbs


@pytest.mark.parametrize("which", ["+30", "mid", "-200"])
def test_anchor_floor(gpu_ctx, oracle, floor_dbs, which):
    _check(gpu_ctx, oracle, wc.lattice_distinct(), dict(WIDE256, min_anchor_mag_db=floor_dbs[which]), which)


# ---------------------------------------------------------------- non-finite and out-of-range samples

@pytest.mark.parametrize("cfg", [DEFAULT, NOFLOOR256], ids=["default", "nofloor256"])
@pytest.mark.parametrize("where", wc.NONFINITE_WHERE)
@pytest.mark.parametrize("kind", list(wc.NONFINITE_KINDS))
def test_nonfinite_samples(gpu_ctx, oracle, kind, where, cfg):
    """A NaN or Inf sample makes 8 all-NaN rows.  A NaN cell is never a peak and never blocks one: the peaks of the
    rows beside such a run (whose 7 earlier or 7 later rows are all NaN) stand as the oracle says."""
    o = _check(gpu_ctx, oracle, wc.nonfinite(kind, where), cfg, (kind, where))
    assert o.shape[0] > 400


@pytest.mark.parametrize("a", wc.SCALES)
def test_scaled_samples(gpu_ctx, oracle, a):
    """Denormal powers (kept, not flushed), powers that underflow to 0 (never a peak), rows of +Inf (all ties: one
    peak, no hash) -- with the floor at 0, so that a denormal peak is an anchor."""
    o = _check(gpu_ctx, oracle, wc.scaled(a), NOFLOOR256, a)
    assert (o.shape[0] == 0) == (a >= 1e19)
    _check(gpu_ctx, oracle, wc.scaled(a), DEFAULT, a)


@pytest.mark.parametrize("kind", list(wc.NONFINITE_KINDS))
def test_nonfinite_samples_in_a_resampled_clip(gpu_ctx, oracle, kind):
    """The same through the kernel that resamples while it cuts the frames: the clip read as 16 kHz audio (A1 spreads a
    bad sample over its two neighbours at 8 kHz), between two clean clips."""
    from ucfp_amd import audio
    clips = [wc.noise3(), wc.nonfinite(kind, "pair9"), wc.noise3()]
    refs = [oracle.wang(oracle.resample_linear(c, 16000, 8000), _ocfg(oracle, NOFLOOR256)) for c in clips]
    P = oracle.stft_power(oracle.resample_linear(clips[1], 16000, 8000), wc.N_FFT, wc.HOP)
    assert 8 <= np.isnan(P).all(axis=1).sum() < 24 and refs[1].shape[0] > 1000
    got = audio.wang_hashes_batch(clips, 16000, audio.WangConfig(**NOFLOOR256), ctx=gpu_ctx)
    for i, (g, o) in enumerate(zip(got, refs)):
        _same(g, o, (kind, i))


# ---------------------------------------------------------------- ragged batch

@pytest.mark.parametrize("cfg", [DEFAULT, NOFLOOR256], ids=["default", "nofloor256"])
def test_ragged_batch_of_dense_and_poisoned_clips(gpu_ctx, oracle, cfg):
    """One call: a dense or poisoned clip must not leak into its neighbour's per-second candidate lists."""
    from ucfp_amd import audio
    clips = [wc.lattice_tied(), wc.short_noise(), wc.lattice_distinct(), np.zeros(0, np.float32),
             wc.nonfinite("nan", "mid"), wc.am_tones()]
    got = audio.wang_hashes_batch(clips, 8000, audio.WangConfig(**cfg), ctx=gpu_ctx)
    assert len(got) == len(clips)
    for i, (g, x) in enumerate(zip(got, clips)):
        _same(g, _ref(oracle, x, cfg), i)
    assert got[3].shape[0] == 0 and got[4].shape[0] > 400


# ---------------------------------------------------------------- truncation, guards, rejections

class _Call:
    pass


def _prepare(torch, ctx, clips, cfg, cap, guard=64):
    """Uploads the batch; d_out holds cap + guard hashes of FILL, d_out_offsets is prefilled with -1."""
    from ucfp_amd import audio
    offs = np.zeros(len(clips) + 1, np.uint64)
    np.cumsum([c.size for c in clips], out=offs[1:])
    k = _Call()
    k.ctx, k.n, k.total, k.cap, k.cfg = ctx, len(clips), int(offs[-1]), cap, audio.WangConfig(**cfg)._c()
    k.pcm = torch.from_numpy(np.concatenate(clips)).cuda()
    k.off = torch.from_numpy(offs.view(np.int64)).cuda()
    k.out = torch.full((cap + guard, 2), FILL, dtype=torch.int32, device="cuda")
    k.oo = torch.full((k.n + 1,), -1, dtype=torch.int64, device="cuda")
    return k


def _enqueue(torch, k, out_shift=0) -> int:
    """ucfp_audio_wang_batch_dev with d_out moved by out_shift bytes -> its status."""
    from ucfp_amd import _lib
    rc = _lib.load().ucfp_audio_wang_batch_dev(k.ctx.handle, k.pcm.data_ptr(), k.off.data_ptr(), k.total, k.n, 8000,
                                               C.byref(k.cfg), k.out.data_ptr() + out_shift, k.cap, k.oo.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream or None)
    torch.cuda.synchronize()
    return rc


def _untouched(k):
    return bool((k.out.cpu().numpy().view(np.uint32) == FILL).all()) and bool((k.oo.cpu().numpy() == -1).all())


@pytest.fixture(scope="module")
def pair_of_clips(oracle):
    clips = [wc.lattice_distinct(), wc.noise3()]
    refs = [_ref(oracle, c, WIDE256) for c in clips]
    assert refs[0].shape[0] > 40000 and refs[1].shape[0] > 5000
    return clips, refs


@pytest.mark.parametrize("cap", ["1", "half", "total-1", "total"])
def test_truncation_at_cap_hashes(gpu_ctx, torch_cuda, pair_of_clips, cap):
    clips, refs = pair_of_clips
    want = np.concatenate(refs)
    total = want.shape[0]
    cap = {"1": 1, "half": total // 2, "total-1": total - 1, "total": total}[cap]
    assert refs[0].shape[0] > total // 2 or cap != total // 2          # (the cut falls inside the first clip)
    k = _prepare(torch_cuda, gpu_ctx, clips, WIDE256, cap)
    assert _enqueue(torch_cuda, k) == 0
    out = k.out.cpu().numpy().view(np.uint32)
    assert np.array_equal(out[:cap], want[:cap])                        # the oracle's prefix
    assert (out[cap:] == FILL).all()                                    # nothing behind cap is touched
    assert k.oo.cpu().numpy().tolist() == [0, refs[0].shape[0], total]  # the offsets stay those of the whole result


BAD_FIELDS = [("fan_out", 0), ("fan_out", 65), ("target_zone_t", 0), ("target_zone_t", 513), ("target_zone_f", 0),
              ("target_zone_f", 1025), ("peaks_per_sec", 0), ("peaks_per_sec", 257)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_config_outside_its_ranges_is_rejected(gpu_ctx, torch_cuda, field, value):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import ModalityError
    torch = torch_cuda
    clips = [wc.short_noise(), wc.short_noise()]
    cfg = dict(DEFAULT, **{field: value})
    k = _prepare(torch, gpu_ctx, clips, cfg, 4096)
    assert _enqueue(torch, k) == UCFP_E_MODALITY and _untouched(k)
    lib = _lib.load()
    d_n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    rc = lib.ucfp_audio_wang_dev(gpu_ctx.handle, k.pcm.data_ptr(), clips[0].size, 8000, C.byref(k.cfg), k.out.data_ptr(),
                                 k.cap, d_n.data_ptr(), torch.cuda.current_stream().cuda_stream or None)
    torch.cuda.synchronize()
    assert rc == UCFP_E_MODALITY and _untouched(k) and int(d_n.item()) == -1
    host = np.full((4096, 2), FILL, np.uint32)
    n = C.c_size_t(0)
    rc = lib.ucfp_audio_wang(gpu_ctx.handle, clips[0].ctypes.data, clips[0].size, 8000, C.byref(k.cfg), host.ctypes.data,
                             4096, C.byref(n))
    assert rc == UCFP_E_MODALITY and n.value == 0 and (host == FILL).all()
    with pytest.raises(ModalityError, match="ranges"):
        audio.wang_hashes_batch(clips, 8000, audio.WangConfig(**cfg), ctx=gpu_ctx)
    with pytest.raises(ModalityError, match="ranges"):
        audio.WangStreams(1, audio.WangConfig(**cfg), ctx=gpu_ctx)


def test_range_ends_are_accepted_and_a_misaligned_buffer_is_rejected(gpu_ctx, oracle, torch_cuda):
    from ucfp_amd import _lib
    from ucfp_amd.errors import InvalidArgument
    clips = [wc.short_noise(), wc.short_noise()]
    for cfg in (dict(fan_out=1, target_zone_t=1, target_zone_f=1, peaks_per_sec=1, min_anchor_mag_db=-50.0),
                dict(fan_out=64, target_zone_t=512, target_zone_f=1024, peaks_per_sec=256, min_anchor_mag_db=-50.0)):
        o = _ref(oracle, clips[0], cfg)
        k = _prepare(torch_cuda, gpu_ctx, clips, cfg, 2 * o.shape[0] + 1)
        assert _enqueue(torch_cuda, k) == 0
        assert k.oo.cpu().numpy().tolist() == [0, o.shape[0], 2 * o.shape[0]]
        assert np.array_equal(k.out.cpu().numpy().view(np.uint32)[:o.shape[0]], o)
    k = _prepare(torch_cuda, gpu_ctx, clips, DEFAULT, 4096)
    assert k.out.data_ptr() % 8 == 0
    rc = _enqueue(torch_cuda, k, out_shift=4)
    assert rc == UCFP_E_INVALID and _untouched(k)
    with pytest.raises(InvalidArgument, match="8-byte"):
        _lib.check(rc)


# ---------------------------------------------------------------- the shared front end: streams, Panako

def _run(ws, slot, x, chunk):
    got, n = [], 0
    while n < x.size:
        got.append(ws.push({slot: x[n:n + chunk]})[slot])
        n += chunk
    got.append(ws.push({slot: x[:0]}, final={slot})[slot])
    return np.concatenate(got)


@pytest.mark.parametrize("chunk", [128, 1000, wc.N3])
@pytest.mark.parametrize("pps", [30, 256])
@pytest.mark.parametrize("name", ["lattice_tied", "lattice_distinct"])
def test_streams_carry_a_full_second_of_candidates(gpu_ctx, oracle, name, pps, chunk):
    """A stream cut into 128-sample, 1000-sample or one chunk emits the offline hashes: the open second's carried
    candidates come close to their capacity (256 of 320) and tie."""
    from ucfp_amd import audio
    x = wc.LATTICES[name]()
    cfg = dict(WIDE, peaks_per_sec=pps)
    ws = audio.WangStreams(1, audio.WangConfig(**cfg), ctx=gpu_ctx)
    _same(_run(ws, ws.open(), x, chunk), _ref(oracle, x, cfg), (name, pps, chunk))


@pytest.mark.parametrize("name", ["lattice_tied", "lattice_distinct"])
def test_panako_over_dense_peaks(gpu_ctx, oracle, name):
    from ucfp_amd import audio
    x = wc.LATTICES[name]()
    c = pr.Cfg(peaks_per_sec=256)
    o = pr.panako_ref(oracle, x, c)
    g = audio.panako_hashes(x, 8000, audio.PanakoConfig(*c.astuple()), ctx=gpu_ctx)
    assert o.shape[0] > 2000 and g.shape == o.shape and g.tobytes() == o.tobytes()
