"""Streaming Wang on the device: whatever the chunking, a stream's hashes are the offline hashes of the
whole signal byte for byte, each emitted exactly when t_anchor < F(n); many streams advance in one push."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4
CHUNKS = (0, 1, 127, 128, 1023, 1024, 7999, 8000, 16000)


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
    return audio.WangConfig(**kw)


def _run(ws, slot, x, chunks, full=None):
    """Pushes x through `slot` in `chunks` (then a final empty push); with `full`, checks the exact frontier after every
    non-final push.  -> the concatenated hashes."""
    got, n = [], 0
    for c in chunks:
        got.append(ws.push({slot: x[n:n + c]})[slot])
        n += c
        if full is not None:
            cum = np.concatenate(got)
            F = ws.frontier(n)
            assert np.array_equal(cum, full[full[:, 1] < F]), (n, F)   # nothing late, nothing early
    got.append(ws.push({slot: x[n:n]}, final={slot})[slot])
    return np.concatenate(got)


@pytest.mark.parametrize("cfg", [dict(), dict(target_zone_t=1), dict(target_zone_t=512), dict(peaks_per_sec=1),
                                 dict(peaks_per_sec=256), dict(fan_out=64), dict(target_zone_f=1)])
def test_chunking_invariance_and_exact_frontier(gpu_ctx, oracle, cfg):
    from ucfp_amd import audio
    c = _cfg(**cfg)
    ws = audio.WangStreams(2, c, ctx=gpu_ctx)
    rng = np.random.default_rng(len(str(cfg)))
    kinds = ["sine440", "chirps", "noise", "clicks", "bursts"]
    for case, sec in enumerate([0.0, 0.1, 1.3, 7.9, 31.0] + ([180.0] if not cfg else [])):
        x = _signal(rng, sec, kinds[case % len(kinds)])
        full = audio.wang_hashes(x, 8000, c, ctx=gpu_ctx)
        if case == 3:
            oc = oracle.WangCfg(c.fan_out, c.target_zone_t, c.target_zone_f, c.peaks_per_sec, c.min_anchor_mag_db)
            assert np.array_equal(full, oracle.wang(x, oc))
        slot = ws.open()
        got = _run(ws, slot, x, _chunking(rng, x.size), full if sec < 40 else None)
        assert np.array_equal(got, full), (case, sec, got.shape, full.shape)


def test_one_sample_chunks(gpu_ctx):
    from ucfp_amd import audio
    rng = np.random.default_rng(3)
    x = _signal(rng, 0.4, "chirps")
    ws = audio.WangStreams(1, ctx=gpu_ctx)
    slot = ws.open()
    chunks = [1] * 1500 + [x.size - 1500]
    assert np.array_equal(_run(ws, slot, x, chunks), audio.wang_hashes(x, 8000, ctx=gpu_ctx))


def test_many_streams_per_push(gpu_ctx):
    """512 slots: rounds in which a random subset pushes random sizes, some final; closed slots are reopened."""
    from ucfp_amd import audio
    rng = np.random.default_rng(21)
    S = 512
    ws = audio.WangStreams(S, ctx=gpu_ctx)
    sig, pos, got, done = {}, {}, {}, []
    for _ in range(S):
        s = ws.open()
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
        out = ws.push(chunks, final)
        for s in pick:
            got[s].append(out[s])
        for s in final:
            done.append((sig.pop(s), np.concatenate(got.pop(s))))
        for s in final:
            n = ws.open()                      # reopen: a fresh stream in the slot
            sig[n] = _signal(rng, 0.5 + 5 * rng.random(), "chirps")
            pos[n], got[n] = 0, []
    out = ws.push({s: sig[s][pos[s]:] for s in sig}, final=set(sig))
    for s in sig:
        got[s].append(out[s])
        done.append((sig[s], np.concatenate(got[s])))
    assert len(done) > S
    ref = audio.wang_hashes_batch([x for x, _ in done], 8000, ctx=gpu_ctx)
    for (x, g), r in zip(done, ref):
        assert np.array_equal(g, r)
    alone = audio.WangStreams(1, ctx=gpu_ctx)          # and the same streams pushed alone
    for x, g in done[:6]:
        slot = alone.open()
        assert np.array_equal(_run(alone, slot, x, _chunking(rng, x.size)), g)


def test_past_37_hours(gpu_ctx, torch_cuda):
    """2^23 frames is the limit of one offline clip, not of a stream: 37.3 h of silence, then 20 s of audio."""
    from ucfp_amd import audio
    torch = torch_cuda
    ws = audio.WangStreams(1, ctx=gpu_ctx)
    slot = ws.open()
    zeros = torch.zeros(107_520_000, dtype=torch.float32, device="cuda")
    cap = ws.max_hashes([slot], [zeros.numel()]) + 1000
    out = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    oo = torch.zeros(2, dtype=torch.int64, device="cuda")
    for _ in range(10):
        ws.push_dev([slot], [zeros.numel()], zeros, out, oo)
        assert oo.cpu().tolist() == [0, 0]          # silence has no peaks
    del zeros
    rng = np.random.default_rng(8)
    x = _signal(rng, 20.0, "chirps")
    got = [ws.push({slot: x[:77777]})[slot], ws.push({slot: x[77777:]})[slot], ws.push({slot: x[:0]}, {slot})[slot]]
    got = np.concatenate(got)
    base = 1_075_200_000 // 128
    assert base == 8_400_000 and base > 1 << 23
    ref = audio.wang_hashes(x, 8000, ctx=gpu_ctx)
    ref = ref[ref[:, 1] >= 63].copy()
    ref[:, 1] += base
    assert ref.shape[0] > 100
    assert np.array_equal(got[got[:, 1] >= base + 63], ref)


def test_capacity_and_errors(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib, audio
    from ucfp_amd.errors import UcfpError
    torch = torch_cuda
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ucfp_wang_streams_create(gpu_ctx.handle, 16000, None, 4, C.byref(h)) == UCFP_E_MODALITY
    bad = _lib.WangConfig(10, 513, 64, 30, -50.0)
    assert lib.ucfp_wang_streams_create(gpu_ctx.handle, 8000, C.byref(bad), 4, C.byref(h)) == UCFP_E_MODALITY
    rng = np.random.default_rng(4)
    x = _signal(rng, 6.0, "chirps")
    a, b = audio.WangStreams(4, ctx=gpu_ctx), audio.WangStreams(4, ctx=gpu_ctx)
    sa, sb = a.open(), b.open()
    s2 = a.open()
    d_x = torch.from_numpy(x).cuda()
    oo = torch.zeros(2, dtype=torch.int64, device="cuda")
    ref = [b.push({sb: x[:30000]})[sb], b.push({sb: x[30000:]}, {sb})[sb]]
    for part, (lo, hi, fin) in enumerate([(0, 30000, ()), (30000, x.size, (sa,))]):
        bound = a.max_hashes([sa], [hi - lo], fin)
        assert bound > 0
        out = torch.zeros((bound, 2), dtype=torch.int32, device="cuda")
        st = lib.ucfp_wang_streams_push_dev(a.handle, np.array([sa], np.uint32).ctypes.data,
                                            np.array([hi - lo], np.uint64).ctypes.data,
                                            np.array([1 if fin else 0], np.uint8).ctypes.data, 1, d_x[lo:].data_ptr(),
                                            out.data_ptr(), bound - 1, oo.data_ptr(), None)
        assert st == UCFP_E_INVALID and b"cap_hashes" in lib.ucfp_last_error()
        a.push_dev([sa], [hi - lo], d_x[lo:hi], out, oo, fin)        # the retry: exactly what it would have given
        o = oo.cpu().numpy()
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[o[0]:o[1]], ref[part])
    with pytest.raises(UcfpError):
        a.push({sa: x[:10]})               # closed by its final push
    with pytest.raises(UcfpError):
        a.push({7: x[:10]})                # out of range
    with pytest.raises(UcfpError):
        a.push_dev([s2, s2], [5, 5], d_x[:10], torch.zeros((8, 2), dtype=torch.int32, device="cuda"),
                   torch.zeros(3, dtype=torch.int64, device="cuda"))       # twice in one push
    a.close(s2)
    with pytest.raises(UcfpError):
        a.close(s2)
    with pytest.raises(UcfpError):
        a.push({s2: x[:10]})
    s3 = a.open()                          # fresh after close: t starts at 0 again
    assert np.array_equal(_run(a, s3, x, [40000, x.size - 40000]), audio.wang_hashes(x, 8000, ctx=gpu_ctx))


def test_streaming_session_random_chunkings(gpu_ctx):
    from ucfp_amd import audio
    rng = np.random.default_rng(17)
    s = audio.StreamingWangSession(8000, 3, 9)
    for case in range(4):
        x = _signal(rng, 1 + 9 * rng.random(), ["chirps", "noise", "bursts", "sine440"][case])
        rec = audio.fingerprint_wang(x, 8000, 3, 9)
        n = 0
        for c in _chunking(rng, x.size):
            assert s.push(x[n:n + c]) == []
            n += c
        out = s.finalize()
        if not rec.fingerprint:              # silence: no hashes, no record
            assert out == []
            continue
        assert len(out) == 1 and out[0].fingerprint == rec.fingerprint and out[0].record_id == 9
    assert s.finalize() == []
