"""The cases of the resampling stream sets, written once for the two kinds: tests/test_wang_streams_sr_gpu.py
and tests/test_panako_streams_sr_gpu.py run them with their `Kind`.  Whatever the cutting, a stream at `sr` emits the
record of the offline batch entry at that rate byte for byte, each row exactly when its anchor time < F(S(n))."""

import numpy as np
import pytest

import panako_ref as pr

UCFP_E_MODALITY, UCFP_E_INVALID = -1, -4
GPU_RATES = (44100, 48000, 11025, 7999, 8001, 1000, 384000)
DENSE = dict(fan_out=64, peaks_per_sec=256)
WIDE = dict(fan_out=1, target_zone_t=125, target_zone_f=1024)


class Kind:
    """What differs between the Wang and the Panako set."""

    def __init__(self, name):
        from ucfp_amd import audio
        self.name = name
        self.width = 2 if name == "wang" else 4
        self.Config = audio.WangConfig if name == "wang" else audio.PanakoConfig
        self.Streams = audio.WangStreams if name == "wang" else audio.PanakoStreams
        self.Session = audio.StreamingWangSession if name == "wang" else audio.StreamingPanakoSession
        self.batch = audio.wang_hashes_batch if name == "wang" else audio.panako_hashes_batch
        self.algorithm = audio.ALGORITHM_WANG if name == "wang" else audio.ALGORITHM_PANAKO

    def cfg(self, **kw):
        return self.Config(**kw)

    def make(self, ctx, slots, sr, cfg=None, W=0, resample=True):
        return self.Streams(slots, cfg, sample_rate=sr, ctx=ctx, window_frames=W, resample=resample)

    def empty(self):
        return np.zeros((0, self.width), np.uint32)


def feed(sr, seconds, seed):
    """Noise, three drifting tones and a silent gap: peaks in every second, at any rate."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    x = 0.08 * rng.standard_normal(n)
    for f in (230.0 + 13 * (seed % 7), 880.0, 1900.0 + 40 * (seed % 5)):
        if f < 0.45 * sr:
            x += 0.15 * np.sin(2 * np.pi * f * t * (1 + 0.05 * t))
    a = int(0.37 * n)
    x[a:a + n // 17] = 0.0
    return np.clip(x, -0.9, 0.9).astype(np.float32)


def cycle_chunks(n, sizes):
    """`sizes` over and over until n samples are cut."""
    out, a, i = [], 0, 0
    while a < n:
        out.append(min(sizes[i % len(sizes)], n - a))
        a += out[-1]
        i += 1
    return out


def run(ss, slot, x, chunks, full=None, final_carries=False):
    """Pushes x through `slot` in `chunks`; the final push is empty or carries the last chunk.  Every push stays within
    max_hashes; with `full`, the rows so far are exactly full[t < F(n)] after every non-final push."""
    got, n, held = [], 0, 0
    for i, c in enumerate(chunks):
        last = final_carries and i == len(chunks) - 1
        bound = ss.max_hashes([slot], [c], [slot] if last else ())
        got.append(ss.push({slot: x[n:n + c]}, final={slot} if last else ())[slot])
        n += c
        held += got[-1].shape[0]
        assert got[-1].shape[0] <= bound, (n, bound)
        if full is not None and not last:
            want = int(np.searchsorted(full[:, 1], ss.frontier(n), "left"))     # anchor times are sorted
            assert held == want and np.array_equal(got[-1], full[want - got[-1].shape[0]:want]), (n, c)
    assert n == x.size
    if not (final_carries and chunks):
        bound = ss.max_hashes([slot], [0], [slot])
        got.append(ss.push({slot: x[:0]}, final={slot})[slot])
        assert got[-1].shape[0] <= bound
    return np.concatenate(got)


def window_ref(full, F, W):
    """The live window by its definition: the offline rows with max(0, F - W) <= anchor time < F, rebased."""
    w0 = max(0, F - W)
    ta = full[:, 1].astype(np.int64)
    w = full[(ta >= w0) & (ta < F)].copy()
    w[:, 1:] -= np.uint32(w0)
    return w, w0


def first_n_with(ss, s8):
    """The least n with S(n) >= s8."""
    lo, hi = 0, (s8 + 2) * ss.sample_rate // 8000 + 4
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ss.final_samples(mid) >= s8 else (mid + 1, hi)
    return lo


# ---- the cases ---------------------------------------------------------------------------------------------------

def cut_invariance(kind, ctx, sr, cfg_kw):
    c = kind.cfg(**cfg_kw)
    x = feed(sr, 4.6, sr % 1000 + len(cfg_kw))
    full = kind.batch([x], sr, c, ctx=ctx)[0]
    assert np.all(np.diff(full[:, 1].astype(np.int64)) >= 0) and full.shape[0] > 20
    ss = kind.make(ctx, 2, sr, c)
    assert ss.frontier(x.size) > 0                       # rows leave before the final push
    k = -(-sr // 8000)
    cuttings = [
        (cycle_chunks(x.size, [0, 1, 997, k - 1, k + 1, k, sr, 0, 1, 1, sr // 2 + 3]), False),
        (cycle_chunks(x.size, [sr]), True),             # whole seconds; the final push carries the last chunk
        (cycle_chunks(x.size, [sr + 1, 2 * sr - 1]), False),
        ([x.size], True),                               # a single push
        ([x.size], False),                              # ... and the final push without samples
        ([], False),                                    # only the final push: nothing
    ]
    for chunks, final_carries in cuttings:
        xs = x if chunks else x[:0]
        slot = ss.open()
        got = run(ss, slot, xs, chunks, full if chunks else None, final_carries)
        assert np.array_equal(got, full if chunks else kind.empty()), (sr, cfg_kw, len(chunks), final_carries)


def one_sample_pushes_at_44100(kind, ctx):
    """64 one-sample pushes across the completion of frame 0 and of the frame that closes second 0 (frame 69: J = 63,
    and with target_zone_t = 20 the frontier leaves 0 there)."""
    sr = 44100
    x = feed(sr, 3.4, 5)
    c = kind.cfg(target_zone_t=20)
    full = kind.batch([x], sr, c, ctx=ctx)[0]
    ss = kind.make(ctx, 1, sr, c)
    b0, b1 = first_n_with(ss, 1024), first_n_with(ss, 1024 + 128 * 69)
    assert ss.frontier(b1 - 1) == 0 < ss.frontier(b1)
    chunks = [b0 - 32] + [1] * 64 + [b1 - 32 - (b0 + 32)] + [1] * 64
    chunks += [x.size - sum(chunks)]
    stalls = sum(ss.final_samples(n) == ss.final_samples(n + 1) for n in range(b0 - 32, b0 + 32))
    assert stalls >= 40                                  # most of those pushes release no 8 kHz sample
    slot = ss.open()
    assert np.array_equal(run(ss, slot, x, chunks, full), full)


def pushes_that_release_nothing(kind, ctx):
    """At 384 kHz an 8 kHz sample takes 48 inputs: a run of 40 one-sample pushes releases none, in the middle of a feed."""
    sr = 384000
    x = feed(sr, 3.3, 9)
    full = kind.batch([x], sr, ctx=ctx)[0]
    ss = kind.make(ctx, 1, sr)
    a = 2 * sr + 48 * 5 + 2
    assert ss.final_samples(a) == ss.final_samples(a + 40)
    chunks = [a] + [1] * 40 + [0, 0] + [7] * 3
    chunks += [x.size - sum(chunks)]
    slot = ss.open()
    assert np.array_equal(run(ss, slot, x, chunks, full), full)


def same_as_old_entry_at_8000(kind, ctx):
    x = feed(8000, 5.0, 3)
    old = kind.make(ctx, 2, 8000, W=63, resample=False)
    new = kind.make(ctx, 2, 8000, W=63, resample=True)
    so, sn = old.open(), new.open()
    n = 0
    chunks = cycle_chunks(x.size, [0, 1, 127, 1023, 8000, 4001])
    for i, c in enumerate(chunks):
        fin = {so} if i == len(chunks) - 1 else ()
        assert old.max_hashes([so], [c], fin) == new.max_hashes([sn], [c], fin)
        a, b = old.push({so: x[n:n + c]}, fin)[so], new.push({sn: x[n:n + c]}, fin)[sn]
        assert np.array_equal(a, b), (i, c)
        n += c
        assert old.frontier(n) == new.frontier(n)
        if not fin:
            wa, wb = old.windows([so])[so], new.windows([sn])[sn]
            assert wa[1] == wb[1] and np.array_equal(wa[0], wb[0])
    lib = new._lib
    abi = f"ucfp_{kind.name}_streams_state_bytes"
    old_bytes = getattr(lib, abi + "_ex")(None, 63) if kind.name == "wang" else getattr(lib, abi)(None, 63)
    assert getattr(lib, abi + "_sr")(None, 63, 8000) == old_bytes


def many_streams_at_different_phases(kind, ctx):
    """65 streams in one push, each pre-advanced by a different count; then a push in which some entries are fresh, some
    carry state and some are final.  Every push gives each stream what it gives the stream pushed alone."""
    sr, S = 44100, 65
    many, alone = kind.make(ctx, S + 8, sr), kind.make(ctx, 1, sr)
    sig = [feed(sr, 2.4 + 0.01 * (i % 5), 100 + i) for i in range(S)]
    pre = [0 if i % 13 == 0 else 1 + 37 * i + (i % 7) * 5513 for i in range(S)]
    step = [sr + 11 * i for i in range(S)]
    slots = [many.open() for _ in range(S)]
    outs = {s: [] for s in slots}
    for i, s in enumerate(slots):                        # different phases of S, different ages
        if pre[i]:
            outs[s].append(many.push({s: sig[i][:pre[i]]})[s])
    phases = {(pre[i] * 8000) % sr for i in range(S)}
    assert len(phases) > 40
    got = many.push({s: sig[i][pre[i]:pre[i] + step[i]] for i, s in enumerate(slots)})       # 65 entries, one push
    for s in slots:
        outs[s].append(got[s])
    # some final (with and without samples), some carrying state, some fresh
    fresh = [many.open() for _ in range(5)]
    fsig = [feed(sr, 1.5, 300 + i) for i in range(5)]
    chunks, final = {}, set()
    for i, s in enumerate(slots):
        lo = pre[i] + step[i]
        chunks[s] = (sig[i][lo:], sig[i][lo:lo + 20000 + i], sig[i][:0])[i % 3]
        if i % 3 != 1:
            final.add(s)
    for i, s in enumerate(fresh):
        chunks[s] = fsig[i][:30000 + 7 * i]
    bound = many.max_hashes(list(chunks), [v.size for v in chunks.values()], final)
    got = many.push(chunks, final)
    assert sum(v.shape[0] for v in got.values()) <= bound
    for s in chunks:
        outs.setdefault(s, []).append(got[s])
    emitted = 0
    for i, s in enumerate(slots):                        # the same pushes, alone
        a = alone.open()
        want = []
        if pre[i]:
            want.append(alone.push({a: sig[i][:pre[i]]})[a])
        want.append(alone.push({a: sig[i][pre[i]:pre[i] + step[i]]})[a])
        want.append(alone.push({a: chunks[s]}, {a} if s in final else ())[a])
        if s not in final:
            alone.close(a)
        assert len(want) == len(outs[s])
        for g, w in zip(outs[s], want):
            assert np.array_equal(g, w), (i, s)
        emitted += sum(w.shape[0] for w in want)
    assert emitted > 1000
    done = [i for i in range(S) if i % 3 == 0]           # whole feeds: the offline record
    ref = kind.batch([sig[i] for i in done], sr, ctx=ctx)
    for i, r in zip(done, ref):
        assert np.array_equal(np.concatenate(outs[slots[i]]), r), i
    for i, s in enumerate(fresh):                        # the fresh ones go on to their offline record too
        rest = many.push({s: fsig[i][30000 + 7 * i:]}, {s})[s]
        assert np.array_equal(np.concatenate([outs[s][0], rest]), kind.batch([fsig[i]], sr, ctx=ctx)[0])


def slot_reuse(kind, ctx):
    """A stream closed, or ended by a final push, in mid-phase leaves no carried input behind."""
    sr = 44100
    x, y = feed(sr, 3.3, 41), feed(sr, 3.3, 42)
    full = kind.batch([x], sr, ctx=ctx)[0]
    ss = kind.make(ctx, 1, sr)
    chunks = cycle_chunks(x.size, [12347, 1, 30001])
    for how in ("close", "final", "final with samples"):
        slot = ss.open()
        assert slot == 0
        ss.push({slot: y[:20003]})                       # S = 3628 and a fraction: inputs are carried
        ss.push({slot: y[20003:20005]})
        assert (20005 * 8000) % sr != 0
        if how == "close":
            ss.close(slot)
        else:
            ss.push({slot: y[20005:20005 + (3 if "samples" in how else 0)]}, final={slot})
        slot = ss.open()
        assert slot == 0
        assert np.array_equal(run(ss, slot, x, chunks, full), full), how


def failed_calls_change_nothing(kind, ctx, torch):
    from ucfp_amd.errors import UcfpError
    sr = 44100
    x = feed(sr, 4.4, 77)
    full = kind.batch([x], sr, ctx=ctx)[0]
    ss = kind.make(ctx, 4, sr)
    lib = ss._lib
    push_dev = getattr(lib, f"ucfp_{kind.name}_streams_push_dev")
    s0, s1 = ss.open(), ss.open()
    ss.close(s1)
    d_x = torch.from_numpy(x).cuda()
    oo = torch.zeros(3, dtype=torch.int64, device="cuda")
    cuts = [0, 110251, 158762, x.size]               # 2.5 s and 3.6 s: the frontier has moved at both
    got = []
    for part in range(3):
        lo, hi = cuts[part], cuts[part + 1]
        fin = (s0,) if part == 2 else ()
        with pytest.raises(UcfpError):                   # a slot twice
            ss.push_dev([s0, s0], [5, 5], d_x[:10], torch.zeros((8, kind.width), dtype=torch.int32, device="cuda"), oo)
        assert b"twice" in lib.ucfp_last_error()
        with pytest.raises(UcfpError):                   # a closed slot beside an open one
            ss.push({s0: x[lo:hi], s1: x[:10]})
        assert b"not open" in lib.ucfp_last_error()
        bound = ss.max_hashes([s0], [hi - lo], fin)
        assert bound > 0
        out = torch.zeros((bound + 1, kind.width), dtype=torch.int32, device="cuda")
        st = push_dev(ss.handle, np.array([s0], np.uint32).ctypes.data, np.array([hi - lo], np.uint64).ctypes.data,
                      np.array([1 if fin else 0], np.uint8).ctypes.data, 1, d_x[lo:].data_ptr(), out.data_ptr(), bound - 1,
                      oo.data_ptr(), None)
        assert st == UCFP_E_INVALID and b"cap_hashes" in lib.ucfp_last_error()
        big = np.array([(1 << 29) + 1], np.uint64)       # a chunk above 2^29 input samples
        assert ss.max_hashes([s0], big) == 0 and b"2^29" in lib.ucfp_last_error()
        ss.push_dev([s0], [hi - lo], d_x[lo:hi], out, oo, fin, bound)        # the push that follows
        o = oo.cpu().numpy()
        got.append(out.cpu().numpy().view(np.uint32)[o[0]:o[1]])
        if part < 2:
            want = int(np.searchsorted(full[:, 1], ss.frontier(hi), "left"))
            assert sum(g.shape[0] for g in got) == want
    assert np.array_equal(np.concatenate(got), full)
    with pytest.raises(UcfpError):
        ss.push({s0: x[:10]})                            # closed by its final push


def upsampled_chunk_limit(kind, ctx):
    """A chunk may release at most 2^29 samples at 8 kHz: at 1 kHz that is reached from 2^26 inputs on."""
    ss = kind.make(ctx, 1, 1000)
    s = ss.open()
    ok, big = np.array([1 << 26], np.uint64), np.array([(1 << 26) + 2], np.uint64)
    assert ss.final_samples(int(ok[0])) <= 1 << 29 < ss.final_samples(int(big[0]))
    assert ss.max_hashes([s], big) == 0 and b"2^29" in ss._lib.ucfp_last_error()
    assert ss.max_hashes([s], ok) > 0


def windows_follow_the_stream(kind, ctx, W):
    sr = 44100
    x = feed(sr, 5.6, 61)
    full = kind.batch([x], sr, ctx=ctx)[0]
    ss = kind.make(ctx, 2, sr, W=W)
    other, slot = ss.open(), ss.open()
    w, origin = ss.windows([slot])[slot]
    assert w.shape == (0, kind.width) and origin == 0
    n, some = 0, 0
    for c in cycle_chunks(x.size, [1, sr // 3, 0, sr, 997, sr // 2]):
        ss.push({slot: x[n:n + c]})
        n += c
        got = ss.windows([other, slot])
        want, w0 = window_ref(full, ss.frontier(n), W)
        assert got[slot][1] == w0 and np.array_equal(got[slot][0], want), (n, w0)
        assert got[other][0].shape == (0, kind.width) and got[other][1] == 0
        assert want.shape[0] <= ss.window_cap
        some += want.shape[0] > 0
    assert some >= 5
    ss.push({slot: x[:0]}, final={slot})
    again = ss.open()
    assert again == slot
    w, origin = ss.windows([again])[again]
    assert w.shape == (0, kind.width) and origin == 0


def identify_live(kind, ctx, sr):
    """Four recordings ingested at `sr` through the batch entry, four live feeds at `sr` playing 12 s of them."""
    from ucfp_amd import audio, index
    W, k, tenant = 625, 3, 4
    recs = [pr.signal("chirps" if i % 2 == 0 else "noise", pr.RECORDING_S, seed=7100 + i, sr=sr) for i in range(4)]
    gx = index.GpuIndex(ctx=ctx)
    rows = kind.batch(recs, sr, ctx=ctx)
    gx.upsert([audio._record(kind.algorithm, r.tobytes(), tenant, 100 + i) for i, r in enumerate(rows)])
    live = kind.make(ctx, 6, sr, W=W)
    slots = [live.open() for _ in range(5)]              # the fifth stays untouched: an empty window
    for sec in range(12):
        live.push({s: recs[i][(4 + sec) * sr:(5 + sec) * sr] for i, s in enumerate(slots[:4])})
    order = [slots[2], slots[4], slots[0], slots[3], slots[1]]
    match = dict(window=12) if kind.name == "panako" else {}
    got = gx.identify_live(tenant, live, order, k, 2, **match)
    host = live.windows(order)
    assert list(got) == order
    for i, s in enumerate(slots):
        hits, origin = got[s]
        assert origin == host[s][1]
        if kind.name == "wang":
            want = gx.identify(tenant, host[s][0], k, 2)
        else:
            want = gx.identify_stretched(tenant, host[s][0], k, 2, **match)
        assert hits == want, s
        if i < 4:
            assert hits and hits[0].record_id == 100 + i and origin == max(0, live.frontier(12 * sr) - W)
        else:
            assert hits == [] and origin == 0 and host[s][0].shape[0] == 0


def sessions(kind, ctx):
    from ucfp_amd import audio
    from ucfp_amd.errors import ModalityError
    sr = 44100
    with pytest.raises(ModalityError):
        kind.Session(sr, 3, 9)
    with pytest.raises(ModalityError):
        kind.Session(sr, 3, 9, resample=False)
    s = kind.Session(sr, 3, 9, resample=True)
    for case in range(2):
        x = feed(sr, 3.1 + case, 17 + case)
        rows = kind.batch([x], sr)[0]
        assert rows.shape[0] > 0
        n = 0
        for c in cycle_chunks(x.size, [0, 1, 4410, sr, 997]):
            assert s.push(x[n:n + c]) == []
            n += c
        out = s.finalize()
        assert len(out) == 1 and out[0].fingerprint == rows.tobytes() and out[0].record_id == 9
        assert out[0].algorithm == kind.algorithm
    assert s.finalize() == []
    s8 = kind.Session(8000, 3, 9, resample=True)        # at 8 kHz the keyword changes nothing
    x = feed(8000, 3.0, 5)
    s8.push(x)
    rec = (audio.fingerprint_wang if kind.name == "wang" else audio.fingerprint_panako)(x, 8000, 3, 9)
    assert s8.finalize()[0].fingerprint == rec.fingerprint
