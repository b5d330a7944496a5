"""Streaming Haitsma on the device: whatever the cutting, the concatenation of what a stream's pushes
emit is the offline record of the whole signal byte for byte, frame f leaving with the push that completes it; many
streams advance in one push; the live blocks feed the sub-fingerprint index."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SECONDS = 2.2            # 11 000 samples at 5 kHz: 140 frames, more than one workgroup's 8 waves of them


def _noise(seed, n):
    return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


_CASES = {}


def _case(gpu_ctx, sr, seconds=SECONDS, cfg=None):
    """(signal, offline record), computed once per rate and left unchanged."""
    from ucfp_amd import audio
    key = (sr, seconds, None if cfg is None else (cfg.fmin, cfg.fmax))
    if key not in _CASES:
        x = _noise(sr + 7, int(seconds * sr))
        full = audio.haitsma_frames(x, sr, cfg, ctx=gpu_ctx)
        x.setflags(write=False)
        full.setflags(write=False)
        _CASES[key] = (x, full)
    return _CASES[key]


def _run(hs, slot, x, chunks, final_carries=False):
    """x through `slot` in `chunks`; the final push carries the last chunk or is empty.  Every push must emit exactly the
    frames [Fr(before), Fr(after)).  -> the concatenated frames."""
    got, a = [], 0
    for k, c in enumerate(chunks):
        last = final_carries and k == len(chunks) - 1
        out = hs.push({slot: x[a:a + c]}, final={slot} if last else ())[slot]
        assert out.size == hs.emitted(a + c, last) - hs.emitted(a), (a, c, last)
        got.append(out)
        a += c
    assert a == len(x)
    if not (final_carries and chunks):
        got.append(hs.push({slot: x[:0]}, final={slot})[slot])
    return np.concatenate(got)


def _equal_chunks(n, c):
    return [c] * (n // c) + ([n % c] if n % c else [])


def _random_chunks(rng, n, hi=3000):
    out, a = [], 0
    while a < n:
        c = 0 if rng.random() < 0.15 else int(rng.integers(0, hi + 1))
        out.append(min(c, n - a))
        a += out[-1]
    return out


def _first_n_with(hs, frames):
    """The smallest sample count at which the stream has emitted `frames` frames."""
    lo, hi = 0, 1 << 32
    while lo < hi:
        mid = (lo + hi) // 2
        if hs.emitted(mid) >= frames:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _ones_around(n, at, run=40):
    """Chunks that reach `at` with `run` one-sample pushes around it."""
    a = max(0, at - run // 2)
    return [a] + [1] * run + [n - a - run]


@pytest.mark.parametrize("sr", [5000, 8000, 44100, 4000])
def test_cut_invariance(gpu_ctx, sr):
    from ucfp_amd import audio
    x, full = _case(gpu_ctx, sr)
    n = len(x)
    assert full.size >= 140
    hs = audio.HaitsmaStreams(2, sr, ctx=gpu_ctx)
    rng = np.random.default_rng(sr)
    patterns = [
        ([n], True), ([n], False),                                      # one push
        (_equal_chunks(n, sr), False), (_equal_chunks(n, sr), True),    # one second each; the final push carries the rest
        (_random_chunks(rng, n), False), (_random_chunks(rng, n), True),
        (_ones_around(n, _first_n_with(hs, 1)), False),                 # frame 0 completes inside a run of one-sample pushes
        (_ones_around(n, _first_n_with(hs, 58)), False),                # ... and frame 57
        ([0, 0, n - 1, 0, 1], False), ([1, 2, n - 3], True),
    ]
    for chunks, final_carries in patterns:
        slot = hs.open()
        got = _run(hs, slot, x, chunks, final_carries)
        assert np.array_equal(got, full), (sr, chunks[:4], final_carries)
    hs.destroy()


@pytest.mark.parametrize("sr", [384000, 1000])
def test_extreme_rates(gpu_ctx, sr):
    """384 kHz: up to 77 input samples are carried for the next output; 1 kHz: five outputs hang on one future input."""
    from ucfp_amd import audio
    x, full = _case(gpu_ctx, sr, 0.6)
    n = len(x)
    assert full.size >= 14
    hs = audio.HaitsmaStreams(1, sr, ctx=gpu_ctx)
    rng = np.random.default_rng(sr)
    step = max(1, sr // 5000)
    at = _first_n_with(hs, 3)
    patterns = [(_random_chunks(rng, n, hi=max(40, n // 30)), False),
                (_ones_around(n, at, run=2 * step + 6), True),          # every phase between two outputs, twice over
                ([at - 1, 1, n - at], False), ([n - 1, 1], True), ([n], True)]
    for chunks, final_carries in patterns:
        slot = hs.open()
        got = _run(hs, slot, x, chunks, final_carries)
        assert np.array_equal(got, full), (sr, chunks[:4], final_carries)
    hs.destroy()


def test_history_is_carried_across_pushes(gpu_ctx):
    from ucfp_amd import audio
    sr = 5000
    x, full = _case(gpu_ctx, sr)
    hs = audio.HaitsmaStreams(1, sr, ctx=gpu_ctx)
    for f in (0, 30):                        # frame f is the last of one push, f + 1 the first of the next
        cut = 2048 + 64 * f
        slot = hs.open()
        a = hs.push({slot: x[:cut]})[slot]
        b = hs.push({slot: x[cut:cut + 64]})[slot]        # emits nothing but frame f + 1
        mid = hs.push({slot: x[:0]})[slot]                # a push that emits nothing keeps the history
        c = hs.push({slot: x[cut + 64:]}, final={slot})[slot]
        assert a.size == f + 1 and b.size == 1 and mid.size == 0
        assert np.array_equal(np.concatenate([a, b, c]), full)
        no_history = audio.haitsma_frames(x[64 * (f + 1):64 * (f + 1) + 2048], sr, ctx=gpu_ctx)
        assert no_history.size == 1 and no_history[0] != full[f + 1]      # so the case does test the carry
        no_history = audio.haitsma_frames(x[64 * (f + 2):64 * (f + 2) + 2048], sr, ctx=gpu_ctx)
        assert no_history[0] != full[f + 2]
    hs.destroy()


def test_many_streams_in_one_push(gpu_ctx):
    from ucfp_amd import audio
    sr, n_streams = 8000, 65
    rng = np.random.default_rng(65)
    xs = [_noise(100 + i, 9000 + 613 * i) for i in range(n_streams)]
    xs[2] = xs[2][:5000]                                 # finalised by the first push: 3125 samples at 5 kHz
    fulls = audio.haitsma_frames_batch(xs, sr, ctx=gpu_ctx)
    hs = audio.HaitsmaStreams(n_streams, sr, ctx=gpu_ctx)
    slots = [hs.open() for _ in range(n_streams)]
    assert slots == list(range(n_streams))
    first = [3300 + 531 * i + int(rng.integers(0, 64)) for i in range(n_streams)]    # different lengths and phases
    first[0], first[1], first[2] = 0, 100, len(xs[2])    # an empty chunk, one that emits nothing, one that finalises
    order = [int(v) for v in rng.permutation(n_streams)]
    got = hs.push({s: xs[s][:first[s]] for s in order}, final={2})
    assert got[0].size == 0 and got[1].size == 0 and np.array_equal(got[2], fulls[2])
    assert sum(g.size for g in got.values()) > 8 * 3                        # more than one workgroup's waves of frames
    rest = [s for s in order[::-1] if s != 2]
    mid = [first[s] + (len(xs[s]) - first[s]) // 2 for s in range(n_streams)]
    got2 = hs.push({s: xs[s][first[s]:mid[s]] for s in rest})
    got3 = hs.push({s: xs[s][mid[s]:] for s in rest}, final=set(rest))
    for s in rest:
        assert np.array_equal(np.concatenate([got[s], got2[s], got3[s]]), fulls[s]), s
    hs.destroy()


def test_push_spanning_chunks_of_frames(gpu_ctx):
    """More than 2 x 131 072 frames in one push: the band energies are produced in chunks of 131 072 frames.  One chunk
    starts at a stream's first frame of the push (history from the state), the next in mid-stream (history recomputed)."""
    from ucfp_amd import audio
    sr, chunk = 5000, 131072

    def samples(frames):
        return 2048 + 64 * (frames - 1)

    xa, xb, xc = _noise(1, samples(chunk - 200) + 40), _noise(2, samples(300)), _noise(3, samples(chunk + 150) + 7)
    hs = audio.HaitsmaStreams(3, sr, ctx=gpu_ctx)
    a, b, c = hs.open(), hs.open(), hs.open()
    head = hs.push({b: xb[:samples(100)], c: xc[:samples(50) + 9]})       # b and c have a history when the big push comes
    assert head[b].size == 100 and head[c].size == 50
    # frames of the push: b [0, 200), a [200, 131 072), c [131 072, 262 172)
    got = hs.push({b: xb[samples(100):], a: xa, c: xc[samples(50) + 9:]}, final={a, b, c})
    assert got[b].size == 200 and got[a].size == chunk - 200 and got[c].size == chunk + 100
    assert np.array_equal(got[a], audio.haitsma_frames(xa, sr, ctx=gpu_ctx))
    assert np.array_equal(np.concatenate([head[b], got[b]]), audio.haitsma_frames(xb, sr, ctx=gpu_ctx))
    assert np.array_equal(np.concatenate([head[c], got[c]]), audio.haitsma_frames(xc, sr, ctx=gpu_ctx))
    hs.destroy()


def test_slot_reuse_starts_from_nothing(gpu_ctx):
    from ucfp_amd import audio
    sr = 8000
    x, full = _case(gpu_ctx, sr)
    y = _noise(99, 7000)
    full_y = audio.haitsma_frames(y, sr, ctx=gpu_ctx)
    hs = audio.HaitsmaStreams(1, sr, block_frames=8, ctx=gpu_ctx)
    slot = hs.open()
    assert np.array_equal(_run(hs, slot, x, [5000, len(x) - 5000]), full)
    with pytest.raises(Exception):
        hs.push({slot: y[:10]})                                           # the final push closed the slot
    assert hs.open() == slot                                              # ... and `open` hands it out again
    cut = _first_n_with(hs, 3)
    head = hs.push({slot: y[:cut]})[slot]
    assert head.size == 3 and np.array_equal(hs.blocks([slot])[slot], full_y[:3])      # no stale ring
    tail = hs.push({slot: y[cut:]}, final={slot})[slot]
    assert np.array_equal(np.concatenate([head, tail]), full_y)           # zero history, no stale tail
    hs.destroy()


def test_failed_calls_change_nothing(gpu_ctx, torch_cuda):
    from ucfp_amd import audio
    from ucfp_amd.errors import InvalidArgument
    torch = torch_cuda
    sr = 8000
    x, full = _case(gpu_ctx, sr)
    hs = audio.HaitsmaStreams(3, sr, ctx=gpu_ctx)
    slot = hs.open()
    cuts = [0, 4000, 9000, 13000, len(x)]
    d_out = torch.zeros(4096, dtype=torch.int32, device="cuda")
    d_oo = torch.zeros(4, dtype=torch.int64, device="cuda")
    got = []
    for k in range(4):
        chunk = x[cuts[k]:cuts[k + 1]]
        d_pcm = torch.from_numpy(np.concatenate([chunk, chunk])).cuda()
        if k == 1:
            with pytest.raises(InvalidArgument, match="twice"):
                hs.push_dev([slot, slot], [chunk.size, chunk.size], d_pcm, d_out, d_oo)
            assert hs.max_frames([slot, slot], [chunk.size, chunk.size]) == 0
        if k == 2:
            with pytest.raises(InvalidArgument, match="not open"):
                hs.push_dev([slot, 1], [chunk.size, chunk.size], d_pcm, d_out, d_oo)
            with pytest.raises(InvalidArgument, match="out of range"):
                hs.push_dev([slot, 3], [chunk.size, chunk.size], d_pcm, d_out, d_oo)
        if k == 3:
            need = hs.max_frames([slot], [chunk.size])
            assert need > 1
            with pytest.raises(InvalidArgument, match="cap_frames"):
                hs.push_dev([slot], [chunk.size], d_pcm, d_out, d_oo, cap_frames=need - 1)
        got.append(hs.push({slot: chunk})[slot])
    got.append(hs.push({slot: x[:0]}, final={slot})[slot])
    assert np.array_equal(np.concatenate(got), full)
    hs.destroy()


def test_push_size_limits(gpu_ctx, torch_cuda):
    """The limits are judged from the counts alone, before any sample is read."""
    from ucfp_amd import audio
    from ucfp_amd.errors import InvalidArgument
    torch = torch_cuda
    d_pcm = torch.zeros(16, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(16, dtype=torch.int32, device="cuda")
    d_oo = torch.zeros(2, dtype=torch.int64, device="cuda")
    hs = audio.HaitsmaStreams(1, 1000, ctx=gpu_ctx)                    # one input sample is five at 5 kHz
    slot = hs.open()
    with pytest.raises(InvalidArgument, match="2\\^29"):
        hs.push_dev([slot], [(1 << 29) + 1], d_pcm, d_out, d_oo)
    with pytest.raises(InvalidArgument, match="2\\^31"):
        hs.push_dev([slot], [1 << 29], d_pcm, d_out, d_oo)             # 5 x 2^29 samples at 5 kHz
    most = (1 << 31) // 5 + 1                                          # S = 5 (n - 1) = 2^31 - 3
    assert hs.max_frames([slot], [1 << 29]) == 0 and hs.max_frames([slot], [most + 1]) == 0
    assert hs.max_frames([slot], [most]) == (5 * (most - 1) - 2048) // 64 + 1
    x = _noise(5, 600)
    assert np.array_equal(hs.push({slot: x}, final={slot})[slot], audio.haitsma_frames(x, 1000, ctx=gpu_ctx))
    hs.destroy()


def test_band_edges_travel_with_the_set(gpu_ctx):
    from ucfp_amd import audio
    cfg = audio.HaitsmaConfig(fmin=150.0, fmax=2400.0)
    sr = 8000
    x, full = _case(gpu_ctx, sr, cfg=cfg)
    assert not np.array_equal(full, _case(gpu_ctx, sr)[1])
    hs = audio.HaitsmaStreams(1, sr, cfg, ctx=gpu_ctx)
    assert np.array_equal(_run(hs, hs.open(), x, _equal_chunks(len(x), 3001)), full)
    hs.destroy()


@pytest.mark.parametrize("block", [1, 256])
def test_blocks_feed_the_index(gpu_ctx, torch_cuda, block):
    from ucfp_amd import audio
    from ucfp_amd.index import HaitsmaIndex
    torch = torch_cuda
    sr = 5000
    x, full = _case(gpu_ctx, sr, 6.0)                     # 437 frames: the ring of 256 wraps
    hs = audio.HaitsmaStreams(2, sr, block_frames=block, ctx=gpu_ctx)
    slot, idle = hs.open(), hs.open()
    ix = HaitsmaIndex(ctx=gpu_ctx)
    others = [np.random.default_rng(s).integers(0, 2 ** 32, 400, dtype=np.uint64).astype(np.uint32) for s in (1, 2)]
    ix.upsert(0, np.array([11, 22, 33], np.uint64), [others[0], full, others[1]])
    assert hs.blocks([slot, idle])[slot].size == 0        # before any frame exists the item is empty
    d_fr = torch.zeros(block, dtype=torch.int32, device="cuda")
    d_oo = torch.zeros(2, dtype=torch.int64, device="cuda")
    o_ids = torch.zeros((1, 1), dtype=torch.int64, device="cuda")
    o_d = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    o_o = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((1, 1), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    n = 0
    for c in (2047, 1, 640, 5000, 0, 9000, 3, len(x) - 16691):
        hs.push({slot: x[n:n + c]})
        n += c
        emitted = hs.emitted(n)
        m = min(block, emitted)
        got = hs.blocks([idle, slot])
        assert got[idle].size == 0 and np.array_equal(got[slot], full[emitted - m:emitted]), (n, emitted)
        if m == 0:
            continue
        # push -> blocks -> query without a host round trip of frames
        hs.blocks_dev([slot], d_fr, d_oo, stream=st)
        ix.query_dev(0, d_fr.data_ptr(), d_oo.data_ptr(), 1, 1, 2, 350_000, o_ids.data_ptr(), o_d.data_ptr(),
                     o_o.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)
        torch.cuda.synchronize()
        assert o_n.cpu().tolist() == [1] and d_oo.cpu().tolist() == [0, m]
        assert (int(o_ids[0, 0]), int(o_d[0, 0]), int(o_o[0, 0])) == (22, 0, emitted - m), (n, emitted)
    assert n == len(x) and hs.emitted(n) == full.size
    ix.close()
    hs.destroy()


def test_session(gpu_ctx):
    from ucfp_amd import audio
    sr = 44100
    x, _ = _case(gpu_ctx, sr)
    want = audio.fingerprint_haitsma(x, sr, 3, 9)
    s = audio.StreamingHaitsmaSession(sr, 3, 9)
    for use in range(2):                                  # the session is reusable after finalize
        for a in range(0, len(x), 30000):
            assert s.push(x[a:a + 30000]) == []
        recs = s.finalize()
        assert len(recs) == 1 and recs[0].algorithm == "audiofp-haitsma-v1" == want.algorithm
        assert recs[0].fingerprint == want.fingerprint and recs[0] == want
    s.push(x[:sr // 4])                                   # too short for a frame
    assert s.finalize() == []
    cfg = audio.HaitsmaConfig(fmin=150.0, fmax=2400.0)
    s = audio.StreamingHaitsmaSession(8000, 1, 2, cfg)
    y, _ = _case(gpu_ctx, 8000)
    s.push(y[:5000])
    s.push(y[5000:])
    assert s.finalize()[0] == audio.fingerprint_haitsma_with(y, 8000, cfg, 1, 2)
