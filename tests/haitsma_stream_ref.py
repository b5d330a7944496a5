"""Streaming Haitsma restated on the CPU over the oracle: the emission rule in integers and a stateful
stream that resamples by the absolute output index, keeps the 5 kHz tail from one frame before the next frame to emit,
runs the oracle's 5 kHz core over it and drops that first frame (it only supplies the history)."""
import numpy as np

SR5, N, HOP = 5000, 2048, 64


def final_samples(n: int, sr: int, final: bool = False) -> int:
    """S(n): the 5 kHz samples of a stream that are final after n input samples."""
    if sr == SR5:
        return n
    if final or n == 0:
        return n * SR5 // sr
    return min(-(-(n - 1) * SR5 // sr), n * SR5 // sr)


def frames(s5: int) -> int:
    return 0 if s5 < N else (s5 - N) // HOP + 1


def stream_frames(n: int, sr: int, final: bool = False) -> int:
    """Fr: sub-fingerprints emitted after n input samples."""
    return frames(final_samples(n, sr, final))


def resample_range(x, base: int, n_total: int, sr: int, lo: int, hi: int, clamp: bool) -> np.ndarray:
    """Outputs [lo, hi) of the linear resampler sr -> 5 kHz; x holds the input samples from absolute index `base` on.
    The operations of oracle.resample_linear at the ABSOLUTE output index; only `clamp` (the stream's end) clamps idx + 1."""
    i = np.arange(lo, hi, dtype=np.uint64)
    num = i * np.uint64(sr)
    idx = (num // np.uint64(SR5)).astype(np.int64)
    frac = ((num % np.uint64(SR5)).astype(np.float64) / float(SR5)).astype(np.float32)
    nxt = idx + 1
    if clamp:
        nxt = np.minimum(nxt, n_total - 1)
    assert i.size == 0 or (idx[0] >= base and nxt.max() < n_total)
    x = np.asarray(x, np.float32)
    x0, x1 = x[idx - base], x[nxt - base]
    return (x0 + (x1 - x0) * frac).astype(np.float32)


class HaitsmaStreamRef:
    def __init__(self, oracle, sr: int, fmin: float = 300.0, fmax: float = 2000.0):
        self.oracle, self.sr, self.fmin, self.fmax = oracle, sr, fmin, fmax
        self.n = 0                                   # input samples so far
        self.base = 0                                # absolute index of self.inputs[0]
        self.inputs = np.zeros(0, np.float32)        # the input samples the next output still needs
        self.tail0 = 0                               # absolute 5 kHz index of self.tail[0]
        self.tail = np.zeros(0, np.float32)

    def push(self, chunk, final: bool = False) -> np.ndarray:
        chunk = np.asarray(chunk, np.float32).reshape(-1)
        s0 = final_samples(self.n, self.sr)
        f0 = frames(s0)
        x = np.concatenate([self.inputs, chunk])
        self.n += chunk.size
        s1 = final_samples(self.n, self.sr, final)
        f1 = frames(s1)
        if self.sr == SR5:
            new = x[s0 - self.base: s1 - self.base]
        else:
            new = resample_range(x, self.base, self.n, self.sr, s0, s1, final)
        run = np.concatenate([self.tail, new])       # 5 kHz samples [tail0, s1)
        out = np.zeros(0, np.uint32)
        if f1 > f0:
            out = self.oracle.haitsma(run, SR5, self.fmin, self.fmax)
            drop = 1 if f0 > 0 else 0                # run starts at frame f0 - 1 then: its bits had no history
            assert out.size == f1 - f0 + drop
            out = out[drop:]
        keep = HOP * (f1 - 1) if f1 > 0 else 0       # one frame before the next frame to emit
        self.tail, self.tail0 = run[keep - self.tail0:], keep
        c = s1 * self.sr // SR5                      # the input sample output s1 starts from
        self.inputs, self.base = x[c - self.base:], c
        assert self.tail.size <= N + HOP - 1 and self.inputs.size <= -(-self.sr // SR5) + 1
        return out


def run_stream(oracle, x, sr: int, chunks, final_carries: bool = False, **kw) -> np.ndarray:
    """x through a fresh stream in `chunks`; the final push carries the last chunk or is empty."""
    ref = HaitsmaStreamRef(oracle, sr, **kw)
    got, a = [], 0
    for k, c in enumerate(chunks):
        last = final_carries and k == len(chunks) - 1
        got.append(ref.push(x[a:a + c], final=last))
        a += c
    assert a == len(x)
    if not (final_carries and chunks):
        got.append(ref.push(x[:0], final=True))
    return np.concatenate(got) if got else np.zeros(0, np.uint32)
