"""Wang / Panako streams at any sample rate restated on the CPU: the rule S(n) in integers and a stateful
stream that resamples by the absolute 8 kHz index and keeps, between chunks, only the inputs the next output still
needs -- at most ceil(sr / 8000) + 1 of them."""
import numpy as np

SR8 = 8000
RATES = (1000, 4000, 7999, 8000, 8001, 11025, 16000, 22050, 44100, 48000, 384000)


def final_samples(n: int, sr: int, final: bool = False) -> int:
    """S(n): the 8 kHz samples of a stream that are final after n input samples."""
    if sr == SR8:
        return n
    if final or n == 0:
        return n * SR8 // sr
    return min(-(-(n - 1) * SR8 // sr), n * SR8 // sr)


def carry_cap(sr: int) -> int:
    return 0 if sr == SR8 else -(-sr // SR8) + 1


def frames(s8: int) -> int:
    return 0 if s8 < 1024 else (s8 - 1024) // 128 + 1


def resample_range(x, base: int, n_total: int, sr: int, lo: int, hi: int, clamp: bool) -> np.ndarray:
    """Outputs [lo, hi) of the linear resampler sr -> 8 kHz; x holds the input samples from absolute index `base` on.
    The operations of oracle.resample_linear at the ABSOLUTE output index; only `clamp` (the stream's end) clamps idx + 1."""
    i = np.arange(lo, hi, dtype=np.uint64)
    num = i * np.uint64(sr)
    idx = (num // np.uint64(SR8)).astype(np.int64)
    frac = ((num % np.uint64(SR8)).astype(np.float64) / float(SR8)).astype(np.float32)
    nxt = idx + 1
    if clamp:
        nxt = np.minimum(nxt, n_total - 1)
    assert i.size == 0 or (idx[0] >= base and nxt.max() < n_total)
    x = np.asarray(x, np.float32)
    x0, x1 = x[idx - base], x[nxt - base]
    return (x0 + (x1 - x0) * frac).astype(np.float32)


class WangStreamSrRef:
    """The assemble step alone: push(chunk) -> the 8 kHz samples that became final."""

    def __init__(self, sr: int):
        self.sr = sr
        self.n = 0                                   # input samples so far
        self.base = 0                                # absolute index of self.inputs[0]
        self.inputs = np.zeros(0, np.float32)        # the input samples the next output still needs

    def push(self, chunk, final: bool = False) -> np.ndarray:
        chunk = np.asarray(chunk, np.float32).reshape(-1)
        s0 = final_samples(self.n, self.sr)
        x = np.concatenate([self.inputs, chunk])
        self.n += chunk.size
        s1 = final_samples(self.n, self.sr, final)
        assert s1 >= s0
        if self.sr == SR8:
            new, self.base = x, self.n
            self.inputs = x[:0]
            return new
        new = resample_range(x, self.base, self.n, self.sr, s0, s1, final)
        c = self.n if final else s1 * self.sr // SR8    # the input sample output s1 starts from
        self.inputs, self.base = x[c - self.base:], c
        assert self.inputs.size <= carry_cap(self.sr)
        return new


def run_stream(x, sr: int, chunks, final_carries: bool = False) -> np.ndarray:
    """x through a fresh stream in `chunks`; the final push carries the last chunk or is empty."""
    ref = WangStreamSrRef(sr)
    got, a = [np.zeros(0, np.float32)], 0
    for k, c in enumerate(chunks):
        last = final_carries and k == len(chunks) - 1
        got.append(ref.push(x[a:a + c], final=last))
        a += c
    assert a == len(x)
    if not (final_carries and chunks):
        got.append(ref.push(x[:0], final=True))
    return np.concatenate(got)
