"""Streaming Panako on the device: whatever the chunking, a stream's records are the offline records of
the whole signal byte for byte, each emitted exactly when t_a < F(n); many streams advance in one push; every stream
keeps its latest window in the shape the Panako index takes as a query."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr

pytestmark = pytest.mark.gpu

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4
CHUNKS = (0, 1, 127, 128, 1023, 1024, 7999, 8000, 16000)
DENSE = dict(fan_out=64, peaks_per_sec=256)


def _signal(rng, seconds, kind):
    n = int(seconds * 8000)
    t = np.arange(n) / 8000.0
    if kind == "sine440":
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t)
    elif kind == "chirps":
        x = np.zeros(n)
        for i in range(8):
            f0 = 100.0 * (1.5 ** i)
            x += 0.06 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f0 / 4) * t * t / max(seconds, 1e-3)))
        x += 0.0158 * rng.standard_normal(n)
    elif kind == "noise":
        x = 0.2 * rng.standard_normal(n)
    elif kind == "clicks":
        x = np.zeros(n)
        x[::8000 // 7] = 0.9
    else:                    # noise bursts between silence gaps
        x = np.zeros(n)
        a = 0
        while a < n:
            b = a + int(rng.integers(1, 24000))
            if rng.random() < 0.5:
                x[a:b] = 0.3 * rng.standard_normal(len(x[a:b]))
            a = b
    return np.clip(x, -0.9, 0.9).astype(np.float32)


def _chunking(rng, n):
    out, a = [], 0
    while a < n:
        c = int(rng.choice(CHUNKS)) if rng.random() < 0.8 else int(rng.integers(0, 40000))
        out.append(min(c, n - a))
        a += out[-1]
    return out


def _cfg(**kw):
    from ucfp_amd import audio
    return audio.PanakoConfig(**kw)


def _run(ps, slot, x, chunks, full=None):
    """Pushes x through `slot` in `chunks` (then a final empty push); with `full`, checks the exact frontier after every
    non-final push.  -> the concatenated records."""
    got, n, held = [], 0, 0
    for c in chunks:
        got.append(ps.push({slot: x[n:n + c]})[slot])
        n += c
        held += got[-1].shape[0]
        if full is not None:
            F = ps.frontier(n)
            want = int(np.searchsorted(full[:, 1], F, "left"))      # t_a is sorted: full[:want] = full[t_a < F]
            assert held == want and np.array_equal(got[-1], full[want - got[-1].shape[0]:want]), (n, F)
    got.append(ps.push({slot: x[n:n]}, final={slot})[slot])
    return np.concatenate(got)


def _window_ref(full, F, W):
    """The live window by its definition: the offline records with max(0, F - W) <= t_a < F, rebased."""
    w0 = max(0, F - W)
    ta = full[:, 1].astype(np.int64)
    w = full[(ta >= w0) & (ta < F)].copy()
    w[:, 1:] -= np.uint32(w0)
    return w, w0


@pytest.mark.parametrize("cfg", [dict(), dict(target_zone_t=1), dict(target_zone_t=512), dict(peaks_per_sec=1),
                                 dict(peaks_per_sec=256), dict(fan_out=1), dict(target_zone_f=1),
                                 dict(fan_out=64, peaks_per_sec=256, target_zone_f=1024)])
def test_chunking_invariance_and_exact_frontier(gpu_ctx, oracle, cfg):
    from ucfp_amd import audio
    c = _cfg(**cfg)
    ps = audio.PanakoStreams(2, c, ctx=gpu_ctx)
    rng = np.random.default_rng(len(str(cfg)))
    kinds = ["sine440", "chirps", "noise", "clicks", "bursts"]
    for case, sec in enumerate([0.0, 0.1, 1.3, 7.9, 31.0]):
        x = _signal(rng, sec, kinds[case % len(kinds)])
        full = audio.panako_hashes(x, 8000, c, ctx=gpu_ctx)
        assert np.all(np.diff(full[:, 1].astype(np.int64)) >= 0)
        if case == 3:
            ref = pr.panako_ref(oracle, x, pr.Cfg(c.fan_out, c.target_zone_t, c.target_zone_f, c.peaks_per_sec,
                                                  c.min_anchor_mag_db))
            assert np.array_equal(full, ref)
        slot = ps.open()
        got = _run(ps, slot, x, _chunking(rng, x.size), full)
        assert np.array_equal(got, full), (case, sec, got.shape, full.shape)
    if c.target_zone_t >= 96 and c.target_zone_f >= 96 and c.peaks_per_sec >= 30:
        assert full.shape[0] > 300           # the 31 s signal under the roomier configs


def test_one_sample_chunks(gpu_ctx):
    from ucfp_amd import audio
    rng = np.random.default_rng(3)
    x = _signal(rng, 0.4, "chirps")
    ps = audio.PanakoStreams(1, ctx=gpu_ctx)
    slot = ps.open()
    chunks = [1] * 1500 + [x.size - 1500]
    full = audio.panako_hashes(x, 8000, ctx=gpu_ctx)
    assert full.shape[0] > 0
    assert np.array_equal(_run(ps, slot, x, chunks), full)


def test_many_streams_per_push(gpu_ctx):
    """512 slots: rounds in which a random subset pushes random sizes, some final; closed slots are reopened."""
    from ucfp_amd import audio
    rng = np.random.default_rng(21)
    S = 512
    ps = audio.PanakoStreams(S, window_frames=63, ctx=gpu_ctx)
    sig, pos, got, done = {}, {}, {}, []
    for _ in range(S):
        s = ps.open()
        sig[s] = _signal(rng, 1 + 14 * rng.random(), ["chirps", "noise", "bursts", "sine440"][s % 4])
        pos[s], got[s] = 0, []
    for r in range(24):
        live = list(sig)
        pick = [s for s in live if rng.random() < 0.6]
        chunks, final = {}, set()
        for s in pick:
            c = int(rng.choice(CHUNKS + (4000, 12000, 30000)))
            x = sig[s]
            chunks[s] = x[pos[s]:pos[s] + c]
            pos[s] += chunks[s].size
            if pos[s] >= x.size and rng.random() < 0.5:
                final.add(s)
        out = ps.push(chunks, final)
        for s in pick:
            got[s].append(out[s])
        for s in final:
            done.append((sig.pop(s), np.concatenate(got.pop(s))))
        for s in final:
            n = ps.open()                      # reopen: a fresh stream in the slot
            sig[n] = _signal(rng, 0.5 + 5 * rng.random(), "chirps")
            pos[n], got[n] = 0, []
    # the windows of all 512 slots in one call, whatever each one's last push was
    win = ps.windows(list(sig))
    for s in sig:
        cum = np.concatenate(got[s]) if got[s] else np.zeros((0, 4), np.uint32)
        w, w0 = _window_ref(cum, ps.frontier(pos[s]), 63)       # everything below F has been emitted
        assert win[s][1] == w0 and np.array_equal(win[s][0], w), s
    out = ps.push({s: sig[s][pos[s]:] for s in sig}, final=set(sig))
    for s in sig:
        got[s].append(out[s])
        done.append((sig[s], np.concatenate(got[s])))
    assert len(done) > S
    ref = audio.panako_hashes_batch([x for x, _ in done], 8000, ctx=gpu_ctx)
    for (x, g), r in zip(done, ref):
        assert np.array_equal(g, r)
    alone = audio.PanakoStreams(1, ctx=gpu_ctx)          # and the same streams pushed alone
    for x, g in done[:6]:
        slot = alone.open()
        assert np.array_equal(_run(alone, slot, x, _chunking(rng, x.size)), g)


def test_past_37_hours(gpu_ctx, torch_cuda):
    """2^23 frames is the limit of one offline clip, not of a stream: 37.3 h of silence, then 20 s of audio.  The times
    of the records are absolute; those of the window are counted from its origin F - W."""
    from ucfp_amd import audio
    torch = torch_cuda
    W = 625
    ps = audio.PanakoStreams(1, window_frames=W, ctx=gpu_ctx)
    slot = ps.open()
    zeros = torch.zeros(107_520_000, dtype=torch.float32, device="cuda")
    assert zeros.numel() <= 1 << 29
    cap = ps.max_hashes([slot], [zeros.numel()]) + 1000
    out = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    oo = torch.zeros(2, dtype=torch.int64, device="cuda")
    for _ in range(10):
        ps.push_dev([slot], [zeros.numel()], zeros, out, oo)
        assert oo.cpu().tolist() == [0, 0]          # silence has no peaks
    del zeros
    rng = np.random.default_rng(8)
    x = _signal(rng, 20.0, "chirps")
    got = [ps.push({slot: x[:77777]})[slot], ps.push({slot: x[77777:]})[slot]]
    win, origin = ps.windows([slot])[slot]
    got = np.concatenate(got + [ps.push({slot: x[:0]}, {slot})[slot]])
    base = 1_075_200_000 // 128
    assert base == 8_400_000 and base > 1 << 23
    ref = audio.panako_hashes(x, 8000, ctx=gpu_ctx)
    ref = ref[ref[:, 1] >= 63].copy()                # the first second's peaks see the silence in front of them
    ref[:, 1:] += np.uint32(base)
    assert ref.shape[0] > 100
    assert np.array_equal(got[got[:, 1] >= base + 63], ref)
    F = ps.frontier(1_075_200_000 + x.size)
    assert F - W >= base + 63
    w, w0 = _window_ref(ref, F, W)
    assert origin == w0 == F - W and w.shape[0] > 100 and int(w[:, 3].max()) < W + 96 + 1
    assert np.array_equal(win, w)


def test_capacity_and_errors(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import UcfpError
    torch = torch_cuda
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ucfp_panako_streams_create(gpu_ctx.handle, 16000, None, 4, 0, C.byref(h)) == UCFP_E_MODALITY
    bad = _lib.PanakoConfig(5, 513, 96, 30, -50.0)
    assert lib.ucfp_panako_streams_create(gpu_ctx.handle, 8000, C.byref(bad), 4, 0, C.byref(h)) == UCFP_E_MODALITY
    assert lib.ucfp_panako_streams_create(gpu_ctx.handle, 8000, None, 4, 8193, C.byref(h)) == UCFP_E_INVALID
    assert not h.value
    rng = np.random.default_rng(4)
    x = _signal(rng, 6.0, "chirps")
    a, b = audio.PanakoStreams(4, ctx=gpu_ctx), audio.PanakoStreams(4, ctx=gpu_ctx)
    sa, sb = a.open(), b.open()
    s2 = a.open()
    d_x = torch.from_numpy(x).cuda()
    oo = torch.zeros(2, dtype=torch.int64, device="cuda")
    ref = [b.push({sb: x[:30000]})[sb], b.push({sb: x[30000:]}, {sb})[sb]]
    assert ref[0].shape[0] and ref[1].shape[0]
    for part, (lo, hi, fin) in enumerate([(0, 30000, ()), (30000, x.size, (sa,))]):
        bound = a.max_hashes([sa], [hi - lo], fin)
        assert bound > 0
        out = torch.zeros((bound + 1, 4), dtype=torch.int32, device="cuda")
        args = (a.handle, np.array([sa], np.uint32).ctypes.data, np.array([hi - lo], np.uint64).ctypes.data,
                np.array([1 if fin else 0], np.uint8).ctypes.data, 1, d_x[lo:].data_ptr())
        st = lib.ucfp_panako_streams_push_dev(*args, out.data_ptr(), bound - 1, oo.data_ptr(), None)
        assert st == UCFP_E_INVALID and b"cap_hashes" in lib.ucfp_last_error()
        st = lib.ucfp_panako_streams_push_dev(*args, out.data_ptr() + 8, bound, oo.data_ptr(), None)   # misaligned
        assert st == UCFP_E_INVALID and b"aligned" in lib.ucfp_last_error()
        a.push_dev([sa], [hi - lo], d_x[lo:hi], out, oo, fin, bound)     # the retry: exactly what it would have given
        o = oo.cpu().numpy()
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[o[0]:o[1]], ref[part])
    with pytest.raises(UcfpError):
        a.push({sa: x[:10]})               # closed by its final push
    with pytest.raises(UcfpError):
        a.push({7: x[:10]})                # out of range
    with pytest.raises(UcfpError):
        a.push_dev([s2, s2], [5, 5], d_x[:10], torch.zeros((8, 4), dtype=torch.int32, device="cuda"),
                   torch.zeros(3, dtype=torch.int64, device="cuda"))       # twice in one push
    big = np.array([(1 << 29) + 1], np.uint64)         # a chunk above 2^29 samples: refused from its size alone
    assert a.max_hashes([s2], big) == 0 and b"2^29" in lib.ucfp_last_error()
    st = lib.ucfp_panako_streams_push_dev(a.handle, np.array([s2], np.uint32).ctypes.data, big.ctypes.data, None, 1,
                                          d_x.data_ptr(), None, 0, oo.data_ptr(), None)
    assert st == UCFP_E_INVALID and b"2^29" in lib.ucfp_last_error()
    a.close(s2)
    with pytest.raises(UcfpError):
        a.close(s2)
    with pytest.raises(UcfpError):
        a.push({s2: x[:10]})
    s3 = a.open()                          # fresh after close: t starts at 0 again
    assert np.array_equal(_run(a, s3, x, [40000, x.size - 40000]), audio.panako_hashes(x, 8000, ctx=gpu_ctx))


@pytest.fixture(scope="module")
def long_signal(gpu_ctx):
    """31 s of chirps and its offline records under the two configs of the window tests, computed once."""
    from ucfp_amd import audio
    x = _signal(np.random.default_rng(61), 31.0, "chirps")
    return x, {k: audio.panako_hashes(x, 8000, _cfg(**dict(k)), ctx=gpu_ctx) for k in ((), tuple(DENSE.items()))}


@pytest.mark.parametrize("W", [1, 63, 625, 8192])
@pytest.mark.parametrize("cfg", [dict(), DENSE])
def test_windows_follow_the_stream(gpu_ctx, long_signal, cfg, W):
    from ucfp_amd import audio
    x, fulls = long_signal
    full = fulls[tuple(cfg.items())]
    ps = audio.PanakoStreams(2, _cfg(**cfg), window_frames=W, ctx=gpu_ctx)
    other = ps.open()                              # slot 0 stays open and untouched: its window stays empty
    slot = ps.open()
    assert ps.window_cap == (-(-2 * W // 125) + 1) * ps._cfg.peaks_per_sec * ps._cfg.fan_out
    w, origin = ps.windows([slot])[slot]
    assert w.shape == (0, 4) and origin == 0           # empty before the first emission
    rng = np.random.default_rng(W)
    n, emitted, wraps = 0, 0, 0
    for c in _chunking(rng, x.size):
        emitted += ps.push({slot: x[n:n + c]})[slot].shape[0]
        n += c
        got = ps.windows([other, slot])
        want, w0 = _window_ref(full, ps.frontier(n), W)
        assert got[slot][1] == w0 and np.array_equal(got[slot][0], want), (n, w0)
        assert got[other][0].shape == (0, 4) and got[other][1] == 0
        assert want.shape[0] <= ps.window_cap
    if W == 63 and not cfg:
        assert emitted > 4 * ps.window_cap             # the ring went round many times (the chirps have too few peaks
                                                       # for that under the dense config: it wraps at W = 1 only)
    ps.push({slot: x[:0]}, final={slot})
    again = ps.open()                                  # the slot of the finished stream: a fresh, empty window
    assert again == slot
    w, origin = ps.windows([again])[again]
    assert w.shape == (0, 4) and origin == 0


def test_window_of_a_push_that_emits_more_than_the_ring_holds(gpu_ctx):
    """W = 1, fan_out = 1: window_cap = 60 records.  The signal is loud between frames 94 and 228 only, so the strongest
    peaks of seconds 1 and 3 lie next to second 2 and the push that moves F from 92 to 217 emits more than 60."""
    from ucfp_amd import audio
    rng = np.random.default_rng(0)
    n0, n1 = 1024 + 128 * 206, 1024 + 128 * 206 + 16000
    x = 0.003 * rng.standard_normal(n1)
    a, b = 128 * 94 + 512, 128 * 228 + 512
    x[a:b] = 0.3 * rng.standard_normal(b - a)
    x = x.astype(np.float32)
    c = _cfg(fan_out=1)
    ps = audio.PanakoStreams(1, c, window_frames=1, ctx=gpu_ctx)
    assert ps.window_cap == 60 and ps.frontier(n0) == 92 and ps.frontier(n1) == 217
    slot = ps.open()
    first = ps.push({slot: x[:n0]})[slot]
    got = ps.push({slot: x[n0:]})[slot]
    assert got.shape[0] > ps.window_cap
    full = np.concatenate([first, got])
    want, w0 = _window_ref(full, 217, 1)
    w, origin = ps.windows([slot])[slot]
    assert origin == w0 == 216 and want.shape[0] > 0 and np.array_equal(w, want)


def test_windows_of_many_slots_and_errors(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import UcfpError
    torch = torch_cuda
    lib = _lib.load()
    rng = np.random.default_rng(77)
    W, S = 63, 9
    ps = audio.PanakoStreams(S, window_frames=W, ctx=gpu_ctx)
    slots = [ps.open() for _ in range(S)]
    sig = {s: _signal(rng, 6.0, ["chirps", "noise", "bursts"][s % 3]) for s in slots}
    full = dict(zip(slots, audio.panako_hashes_batch([sig[s] for s in slots], 8000, ctx=gpu_ctx)))
    pos = {s: 0 for s in slots}
    for r in range(5):                                 # the last round leaves slots 0-2 out
        pick = [s for s in slots if r < 4 or s > 2]
        chunks = {}
        for s in pick:
            c = int(rng.integers(2000, 12000))
            chunks[s] = sig[s][pos[s]:pos[s] + c]
            pos[s] += chunks[s].size
        ps.push(chunks)
    order = [int(s) for s in rng.permutation(slots)]
    got = ps.windows(order)
    assert list(got) == order
    some = 0
    for s in slots:
        want, w0 = _window_ref(full[s], ps.frontier(pos[s]), W)
        assert got[s][1] == w0 and np.array_equal(got[s][0], want), s
        some += want.shape[0] > 0
    assert some >= 3
    # byte offsets, as the Panako index takes them
    d_rec = torch.zeros((S * ps.window_cap, 4), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    ps.windows_dev(order, d_rec, d_off)                # origins may be left out
    off = d_off.cpu().numpy()
    assert off[0] == 0 and np.all(off % 16 == 0) and off[-1] == 16 * sum(got[s][0].shape[0] for s in slots)
    with pytest.raises(UcfpError):
        ps.windows_dev(order, d_rec, d_off, cap_records=S * ps.window_cap - 1)
    assert b"cap_records" in lib.ucfp_last_error()
    with pytest.raises(UcfpError):
        ps.windows([slots[0], slots[1], slots[0]])     # a slot twice
    ps.close(slots[4])
    with pytest.raises(UcfpError):
        ps.windows([slots[3], slots[4]])               # a closed slot
    with pytest.raises(UcfpError):
        ps.windows([S])                                # out of range
    assert ps.windows([]) == {}
    again = ps.open()                                  # reopened after close: nothing pushed yet, so an empty window
    assert again == slots[4]
    w, origin = ps.windows([again])[again]
    assert w.shape == (0, 4) and origin == 0
    plain = audio.PanakoStreams(1, ctx=gpu_ctx)        # W = 0: the set keeps no windows
    s = plain.open()
    assert plain.window_cap == 0
    with pytest.raises(UcfpError):
        plain.windows([s])
    assert b"window_frames" in lib.ucfp_last_error()


def test_live_windows_identify_on_the_device(gpu_ctx, torch_cuda):
    """8 recordings in a PanakoIndex, 8 live streams playing 12 s of them: the windows go from the set to the index
    without leaving the device, and every stream's top hit is its recording."""
    from ucfp_amd import audio, index
    torch = torch_cuda
    W, k = 625, 3
    ix = index.PanakoIndex(ctx=gpu_ctx)
    recs = [pr.recording(i) for i in range(pr.N_RECORDINGS)]
    ix.upsert(0, [100 + i for i in range(len(recs))], audio.panako_hashes_batch(recs, 8000, ctx=gpu_ctx))
    ix.flush()
    ps = audio.PanakoStreams(len(recs), window_frames=W, ctx=gpu_ctx)
    slots = [ps.open() for _ in recs]
    for sec in range(12):
        ps.push({s: pr.excerpt(recs[i], 4 + sec, 1.0) for i, s in enumerate(slots)})
    nq = len(slots)
    d_rec = torch.zeros((nq * ps.window_cap, 4), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    d_org = torch.zeros(nq, dtype=torch.int32, device="cuda")
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_v = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_o = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_c = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ps.windows_dev(slots, d_rec, d_off, d_org, stream=st)
    ix.query_dev(0, d_rec.data_ptr(), d_off.data_ptr(), nq, k, 2, o_ids.data_ptr(), o_v.data_ptr(), o_o.data_ptr(),
                 o_c.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)
    torch.cuda.synchronize()
    host = ps.windows(slots)
    F = ps.frontier(12 * 8000)
    w0 = max(0, F - W)
    assert d_org.cpu().tolist() == [w0] * nq == [host[s][1] for s in slots]
    h = ix.query(0, [host[s][0] for s in slots], k, 2)
    ids = o_ids.cpu().numpy().view(np.uint64)
    assert ids[:, 0].tolist() == [100 + i for i in range(nq)]
    assert np.all(o_v.cpu().numpy()[:, 0] >= 20)
    # frame w0 of the stream = frame 4 s * 62.5 + w0 of the recording.  Checked on the noise recordings (the odd ones):
    # slow linear chirps look alike under a small shift in time, so their best (scale, offset) bin is not unique
    assert np.all(np.abs(o_o.cpu().numpy()[1::2, 0] - (250 + w0)) <= 2)
    assert np.array_equal(ids, h[0])
    assert np.array_equal(o_v.cpu().numpy().view(np.uint32), h[1])
    assert np.array_equal(o_o.cpu().numpy(), h[2])
    assert np.array_equal(o_c.cpu().numpy().view(np.uint32), h[3])
    assert np.array_equal(o_s.cpu().numpy().view(np.uint32), h[4].view(np.uint32))
    assert np.array_equal(o_n.cpu().numpy().view(np.uint32), h[5])


def test_streaming_session_random_chunkings(gpu_ctx):
    from ucfp_amd import audio
    from ucfp_amd.errors import ModalityError
    rng = np.random.default_rng(17)
    s = audio.StreamingPanakoSession(8000, 3, 9)
    kinds = ["chirps", "noise", "bursts", "sine440", "clicks"]
    records = 0
    for case in range(10):
        x = _signal(rng, 1 + 9 * rng.random(), kinds[case % len(kinds)])
        rec = audio.fingerprint_panako(x, 8000, 3, 9)
        n = 0
        for c in _chunking(rng, x.size):
            assert s.push(x[n:n + c]) == []
            n += c
        out = s.finalize()
        if not rec.fingerprint:              # no records, no record
            assert out == []
            continue
        assert len(out) == 1 and out[0].fingerprint == rec.fingerprint and out[0].record_id == 9
        assert out[0].algorithm == "audiofp-panako-v1"
        records += 1
    assert records >= 4 and s.finalize() == []
    with pytest.raises(ModalityError):
        audio.StreamingPanakoSession(16000, 3, 9)
