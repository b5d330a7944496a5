"""Live Wang windows on the device: a WangStreams created with window_frames = W keeps, per stream, its
emitted hashes with t_anchor >= max(0, F(n) - W), hands them out rebased in the query shape of the landmark index, and
GpuIndex.identify_live chains that into the index without leaving the device."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr
from test_panako_streams_gpu import DENSE, _chunking, _signal

pytestmark = pytest.mark.gpu

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4


def _cfg(**kw):
    from ucfp_amd import audio
    return audio.WangConfig(**kw)


def _window_ref(full, F, W):
    """The live window by its definition: the offline hashes with max(0, F - W) <= t_anchor < F, rebased."""
    w0 = max(0, F - W)
    ta = full[:, 1].astype(np.int64)
    w = full[(ta >= w0) & (ta < F)].copy()
    w[:, 1] -= np.uint32(w0)
    return w, w0


@pytest.fixture(scope="module")
def long_signal(gpu_ctx):
    """31 s of chirps and its offline hashes under the two configs of the window test, computed once."""
    from ucfp_amd import audio
    x = _signal(np.random.default_rng(61), 31.0, "chirps")
    return x, {k: audio.wang_hashes(x, 8000, _cfg(**dict(k)), ctx=gpu_ctx) for k in ((), tuple(DENSE.items()))}


@pytest.mark.parametrize("W", [1, 63, 625, 8192])
@pytest.mark.parametrize("cfg", [dict(), DENSE])
def test_windows_follow_the_stream(gpu_ctx, long_signal, cfg, W):
    from ucfp_amd import audio
    x, fulls = long_signal
    full = fulls[tuple(cfg.items())]
    assert np.all(np.diff(full[:, 1].astype(np.int64)) >= 0)
    ws = audio.WangStreams(2, _cfg(**cfg), ctx=gpu_ctx, window_frames=W)
    other = ws.open()                              # slot 0 stays open and untouched: its window stays empty
    slot = ws.open()
    assert ws.window_frames == W
    assert ws.window_cap == (-(-2 * W // 125) + 1) * ws._cfg.peaks_per_sec * ws._cfg.fan_out
    w, origin = ws.windows([slot])[slot]
    assert w.shape == (0, 2) and origin == 0           # empty before the first push
    rng = np.random.default_rng(W)
    n, emitted = 0, 0
    for c in _chunking(rng, x.size):
        emitted += ws.push({slot: x[n:n + c]})[slot].shape[0]
        n += c
        got = ws.windows([other, slot])
        want, w0 = _window_ref(full, ws.frontier(n), W)
        assert got[slot][1] == w0 and np.array_equal(got[slot][0], want), (n, w0)
        assert got[other][0].shape == (0, 2) and got[other][1] == 0
        assert want.shape[0] <= ws.window_cap
    if W in (1, 63) and not cfg:
        # the ring went round many times: the oracle gives 5612 hashes for this signal under the defaults, against
        # rings of 600 and 900 (under the dense config the chirps' 9268 hashes stay below a ring of 32768)
        assert emitted > 4 * ws.window_cap
    ws.push({slot: x[:0]}, final={slot})
    again = ws.open()                                  # the slot of the finished stream: a fresh, empty window
    assert again == slot
    w, origin = ws.windows([again])[again]
    assert w.shape == (0, 2) and origin == 0


def test_window_of_a_push_that_emits_more_than_the_ring_holds(gpu_ctx):
    """W = 1, fan_out = 1: window_cap = 60 hashes.  The signal is loud between frames 94 and 228 only, so the strongest
    peaks of seconds 1 and 3 lie next to second 2, and with target_zone_t = 96 the push that moves F from 92 to 217
    emits more than 60 (77 by the oracle)."""
    from ucfp_amd import audio
    rng = np.random.default_rng(0)
    n0, n1 = 1024 + 128 * 206, 1024 + 128 * 206 + 16000
    x = 0.003 * rng.standard_normal(n1)
    a, b = 128 * 94 + 512, 128 * 228 + 512
    x[a:b] = 0.3 * rng.standard_normal(b - a)
    x = x.astype(np.float32)
    ws = audio.WangStreams(1, _cfg(fan_out=1, target_zone_t=96, target_zone_f=96), ctx=gpu_ctx, window_frames=1)
    assert ws.window_cap == 60 and ws.frontier(n0) == 92 and ws.frontier(n1) == 217
    slot = ws.open()
    first = ws.push({slot: x[:n0]})[slot]
    got = ws.push({slot: x[n0:]})[slot]
    assert got.shape[0] > ws.window_cap
    full = np.concatenate([first, got])
    want, w0 = _window_ref(full, 217, 1)
    w, origin = ws.windows([slot])[slot]
    assert origin == w0 == 216 and want.shape[0] > 0 and np.array_equal(w, want)


def test_windows_of_many_slots_and_errors(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import InvalidArgument, UcfpError
    torch = torch_cuda
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ucfp_wang_streams_create_ex(gpu_ctx.handle, 16000, None, 4, 63, C.byref(h)) == UCFP_E_MODALITY
    bad = _lib.WangConfig(10, 513, 64, 30, -50.0)
    assert lib.ucfp_wang_streams_create_ex(gpu_ctx.handle, 8000, C.byref(bad), 4, 8193, C.byref(h)) == UCFP_E_MODALITY
    assert lib.ucfp_wang_streams_create_ex(gpu_ctx.handle, 8000, None, 4, 8193, C.byref(h)) == UCFP_E_INVALID
    assert b"window_frames" in lib.ucfp_last_error() and not h.value
    rng = np.random.default_rng(77)
    W, S = 63, 9
    ws = audio.WangStreams(S, ctx=gpu_ctx, window_frames=W)
    slots = [ws.open() for _ in range(S)]
    sig = {s: _signal(rng, 6.0, ["chirps", "noise", "bursts"][s % 3]) for s in slots}
    full = dict(zip(slots, audio.wang_hashes_batch([sig[s] for s in slots], 8000, ctx=gpu_ctx)))
    pos = {s: 0 for s in slots}
    for r in range(5):                                 # the last round leaves slots 0-2 out
        pick = [s for s in slots if r < 4 or s > 2]
        chunks = {}
        for s in pick:
            c = int(rng.integers(2000, 12000))
            chunks[s] = sig[s][pos[s]:pos[s] + c]
            pos[s] += chunks[s].size
        ws.push(chunks)
    order = [int(s) for s in rng.permutation(slots)]
    got = ws.windows(order)
    assert list(got) == order
    some = 0
    for s in slots:
        want, w0 = _window_ref(full[s], ws.frontier(pos[s]), W)
        assert got[s][1] == w0 and np.array_equal(got[s][0], want), s
        some += want.shape[0] > 0
    assert some >= 3
    # byte offsets, as the landmark index takes them
    d_lm = torch.zeros((S * ws.window_cap, 2), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    ws.windows_dev(order, d_lm, d_off)                 # origins may be left out
    off = d_off.cpu().numpy()
    assert off[0] == 0 and np.all(off % 8 == 0) and np.all(np.diff(off) >= 0)
    assert np.array_equal(np.diff(off), [8 * got[s][0].shape[0] for s in order])
    with pytest.raises(InvalidArgument):
        ws.windows_dev(order, d_lm, d_off, cap_landmarks=S * ws.window_cap - 1)
    assert b"cap_landmarks" in lib.ucfp_last_error()
    sl = np.array(order, np.uint32)
    st = lib.ucfp_wang_streams_windows_dev(ws.handle, sl.ctypes.data, S, d_lm.data_ptr() + 4, S * ws.window_cap - 1,
                                           d_off.data_ptr(), None, None)                    # misaligned
    assert st == UCFP_E_INVALID and b"aligned" in lib.ucfp_last_error()
    with pytest.raises(InvalidArgument):
        ws.windows([slots[0], slots[1], slots[0]])     # a slot twice
    ws.close(slots[4])
    with pytest.raises(InvalidArgument):
        ws.windows([slots[3], slots[4]])               # a closed slot
    with pytest.raises(InvalidArgument):
        ws.windows([S])                                # out of range
    after = ws.windows([s for s in order if s != slots[4]][:3])
    for s in after:                                    # a failed call changed no state
        assert after[s][1] == got[s][1] and np.array_equal(after[s][0], got[s][0])
    assert ws.windows([]) == {}
    again = ws.open()                                  # reopened after close: nothing pushed yet, so an empty window
    assert again == slots[4]
    w, origin = ws.windows([again])[again]
    assert w.shape == (0, 2) and origin == 0
    plain = audio.WangStreams(1, ctx=gpu_ctx)          # W = 0: the set keeps no windows
    s = plain.open()
    assert plain.window_cap == 0 and plain.window_frames == 0
    with pytest.raises(UcfpError):
        plain.windows([s])
    assert b"window_frames" in lib.ucfp_last_error()


def test_window_of_an_old_stream(gpu_ctx, torch_cuda):
    """37.3 h of silence (2^23 frames is the limit of one offline clip, not of a stream), then 20 s of audio: the origin
    lies past 2^23, every rebased t below W, and the landmark index takes the window as a query."""
    from ucfp_amd import audio, index
    torch = torch_cuda
    W = 625
    ws = audio.WangStreams(1, ctx=gpu_ctx, window_frames=W)
    slot = ws.open()
    zeros = torch.zeros(107_520_000, dtype=torch.float32, device="cuda")
    cap = ws.max_hashes([slot], [zeros.numel()]) + 1000
    out = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    oo = torch.zeros(2, dtype=torch.int64, device="cuda")
    for _ in range(10):
        ws.push_dev([slot], [zeros.numel()], zeros, out, oo)
    assert oo.cpu().tolist() == [0, 0]              # silence has no peaks
    del zeros, out
    x = _signal(np.random.default_rng(8), 20.0, "chirps")
    ws.push({slot: x[:77777]})
    ws.push({slot: x[77777:]})
    win, origin = ws.windows([slot])[slot]
    base = 1_075_200_000 // 128
    assert base == 8_400_000 and base > 1 << 23
    ref = audio.wang_hashes(x, 8000, ctx=gpu_ctx)
    ref = ref[ref[:, 1] >= 63].copy()                # the first second's peaks see the silence in front of them
    shifted = ref.copy()
    shifted[:, 1] += np.uint32(base)
    F = ws.frontier(1_075_200_000 + x.size)
    assert F - W >= base + 63
    want, w0 = _window_ref(shifted, F, W)
    assert origin == w0 == F - W and origin > 1 << 23
    assert want.shape[0] > 100 and int(win[:, 1].max()) < W
    assert np.array_equal(win, want)
    ix = index.LandmarkIndex(ctx=gpu_ctx)
    ix.upsert(0, [5], [ref])
    ids, votes, offs, _, counts = ix.query(0, [win], 1)
    assert counts[0] == 1 and ids[0, 0] == 5 and offs[0, 0] == w0 - base
    assert votes[0, 0] == np.unique(want, axis=0).shape[0]      # duplicate (hash, t) pairs count once


def test_no_window_is_the_set_as_it_was(gpu_ctx):
    from ucfp_amd import _lib, audio
    lib = _lib.load()
    for c in (None, _lib.WangConfig(64, 512, 1024, 256, -50.0)):
        p = C.byref(c) if c is not None else None
        assert lib.ucfp_wang_streams_state_bytes(p) == lib.ucfp_wang_streams_state_bytes_ex(p, 0) > 0
    x = _signal(np.random.default_rng(5), 9.0, "chirps")
    ref = audio.wang_hashes(x, 8000, ctx=gpu_ctx)
    assert ref.shape[0] > 300
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.ucfp_wang_streams_create(gpu_ctx.handle, 8000, None, 2, C.byref(a)) == 0
    assert lib.ucfp_wang_streams_create_ex(gpu_ctx.handle, 8000, None, 2, 0, C.byref(b)) == 0
    try:
        for h in (a, b):
            slot = C.c_uint32(9)
            assert lib.ucfp_wang_streams_open(h, C.byref(slot)) == 0 and slot.value == 0
            got, n = [], 0
            for c in _chunking(np.random.default_rng(6), x.size) + [0]:
                fin = 1 if n == x.size else 0
                chunk = np.ascontiguousarray(x[n:n + c])
                out = np.zeros((8000, 2), np.uint32)           # above any push's bound: 11 s * 30 * 10
                m = C.c_size_t(0)
                assert lib.ucfp_wang_streams_push(h, 0, chunk.ctypes.data if c else None, c, fin, out.ctypes.data,
                                                  out.shape[0], C.byref(m)) == 0
                got.append(out[:m.value])
                n += c
            assert fin and np.concatenate(got).tobytes() == ref.tobytes()
    finally:
        lib.ucfp_wang_streams_destroy(a)
        lib.ucfp_wang_streams_destroy(b)
    plain = audio.WangStreams(1, ctx=gpu_ctx)
    assert plain.window_cap == 0 and plain.window_frames == 0


def test_live_windows_identify_on_the_device(gpu_ctx, torch_cuda):
    """8 recordings in a LandmarkIndex, 8 live streams playing 12 s of them from second 4 on: the windows go from the set
    to the index without leaving the device, and every stream's top hit is its recording at the right place."""
    from ucfp_amd import audio, index
    torch = torch_cuda
    W, k = 625, 3
    ix = index.LandmarkIndex(ctx=gpu_ctx)
    recs = [pr.recording(i) for i in range(pr.N_RECORDINGS)]
    ix.upsert(0, [100 + i for i in range(len(recs))], audio.wang_hashes_batch(recs, 8000, ctx=gpu_ctx))
    ix.flush()
    ws = audio.WangStreams(len(recs), ctx=gpu_ctx, window_frames=W)
    slots = [ws.open() for _ in recs]
    for sec in range(12):
        ws.push({s: pr.excerpt(recs[i], 4 + sec, 1.0) for i, s in enumerate(slots)})
    nq = len(slots)
    d_lm = torch.zeros((nq * ws.window_cap, 2), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    d_org = torch.zeros(nq, dtype=torch.int32, device="cuda")
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_v = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_o = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ws.windows_dev(slots, d_lm, d_off, d_org, stream=st)
    ix.query_dev(0, d_lm.data_ptr(), d_off.data_ptr(), nq, k, 2, o_ids.data_ptr(), o_v.data_ptr(), o_o.data_ptr(),
                 o_s.data_ptr(), o_n.data_ptr(), st)
    torch.cuda.synchronize()
    host = ws.windows(slots)
    F = ws.frontier(12 * 8000)
    w0 = max(0, F - W)
    assert d_org.cpu().tolist() == [w0] * nq == [host[s][1] for s in slots]
    h = ix.query(0, [host[s][0] for s in slots], k, 2)
    ids = o_ids.cpu().numpy().view(np.uint64)
    assert ids[:, 0].tolist() == [100 + i for i in range(nq)]
    assert np.all(o_v.cpu().numpy()[:, 0] >= 20)
    # frame w0 of the stream = frame 4 s * 62.5 + w0 of the recording
    assert np.all(np.abs(o_o.cpu().numpy()[:, 0] - (250 + w0)) <= 2)
    assert np.array_equal(ids, h[0])
    assert np.array_equal(o_v.cpu().numpy().view(np.uint32), h[1])
    assert np.array_equal(o_o.cpu().numpy(), h[2])
    assert np.array_equal(o_s.cpu().numpy().view(np.uint32), h[3].view(np.uint32))
    assert np.array_equal(o_n.cpu().numpy().view(np.uint32), h[4])


@pytest.mark.parametrize("kind", ["wang", "panako"])
def test_identify_live(gpu_ctx, kind):
    """GpuIndex.identify_live = identify / identify_stretched on the host copies of the same windows."""
    from ucfp_amd import audio, index
    from ucfp_amd.errors import InvalidArgument
    W, k, tenant = 625, 3, 4
    recs = [pr.recording(i) for i in range(4)]
    gx = index.GpuIndex(ctx=gpu_ctx)
    if kind == "wang":
        make, fp = (lambda **kw: audio.WangStreams(6, ctx=gpu_ctx, **kw)), audio.fingerprint_wang
    else:
        make, fp = (lambda **kw: audio.PanakoStreams(6, ctx=gpu_ctx, **kw)), audio.fingerprint_panako
    live = make(window_frames=W)
    slots = [live.open() for _ in range(5)]            # the fifth stays untouched: an empty window
    assert live.open() == 5
    live.close(5)
    empty = gx.identify_live(tenant, live, slots, k)   # nothing indexed, nothing pushed
    assert empty == {s: ([], 0) for s in slots}
    gx.upsert([fp(x, 8000, tenant, 100 + i) for i, x in enumerate(recs)])
    for sec in range(12):
        live.push({s: pr.excerpt(recs[i], 4 + sec, 1.0) for i, s in enumerate(slots[:4])})
    order = [slots[2], slots[4], slots[0], slots[3], slots[1]]
    match = dict(window=12) if kind == "panako" else {}
    got = gx.identify_live(tenant, live, order, k, 2, **match)
    host = live.windows(order)
    assert list(got) == order
    for i, s in enumerate(slots):
        hits, origin = got[s]
        assert origin == host[s][1]
        if kind == "wang":
            want = gx.identify(tenant, host[s][0], k, 2)
        else:
            want = gx.identify_stretched(tenant, host[s][0], k, 2, **match)
        assert hits == want, s
        if i < 4:
            assert hits and hits[0].record_id == 100 + i and origin == max(0, live.frontier(12 * 8000) - W)
        else:
            assert hits == [] and origin == 0 and host[s][0].shape[0] == 0
    assert gx.identify_live(tenant, live, [], k) == {}
    assert gx.identify_live(tenant + 1, live, order, k) == {s: ([], host[s][1]) for s in order}   # an unknown tenant
    with pytest.raises(InvalidArgument):
        gx.identify_live(tenant, live, [5], k)          # a closed slot
    with pytest.raises(InvalidArgument):
        gx.identify_live(tenant, live, order, k, bogus=1)
    plain = make()
    s = plain.open()
    with pytest.raises(InvalidArgument):
        gx.identify_live(tenant, plain, [s], k)         # a set without windows
    with pytest.raises(InvalidArgument):
        gx.identify_live(tenant, audio.HaitsmaStreams(1, 8000, ctx=gpu_ctx), [0], k)
