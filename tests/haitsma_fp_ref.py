"""float64 restatement of the Haitsma sub-fingerprint arithmetic (steps A7 and A8 of audio.hip), numpy only.

It shares no code with the C oracle or the HIP kernels: frames and window from the definitions, numpy's rfft, band sums over
slices of the spectrum.  The bits of a float32 implementation may differ from sign(dd) only where |dd| is small against the
energies it is the difference of; `haitsma_bits64` returns that scale next to dd so that a test can leave such bits out."""
import numpy as np

N, HOP, SR, BANDS = 2048, 64, 5000, 33


def edges64(fmin, fmax) -> np.ndarray:
    """int64 [34]: min(ceil(f32(fmin) * (f32(fmax) / f32(fmin)) ** (b / 33) * 2048 / 5000), 1024), b = 0 .. 33."""
    lo, hi = float(np.float32(fmin)), float(np.float32(fmax))
    f = lo * np.power(hi / lo, np.arange(BANDS + 1, dtype=np.float64) / BANDS)
    return np.minimum(np.ceil(f * N / SR), N // 2).astype(np.int64)


def band_energies64(x5k, fmin, fmax) -> np.ndarray:
    """float64 [T, 33]: E[t, b] = the sum of |rfft(hann * frame t)|^2 over the bins [edge[b], edge[b + 1])."""
    x = np.asarray(x5k, dtype=np.float64).reshape(-1)
    T = 1 + (x.size - N) // HOP if x.size >= N else 0
    e = edges64(fmin, fmax)
    E = np.zeros((T, BANDS), np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)          # periodic Hann
    for t0 in range(0, T, 4096):
        t1 = min(T, t0 + 4096)
        idx = (np.arange(t0, t1) * HOP)[:, None] + np.arange(N)[None, :]
        P = np.abs(np.fft.rfft(x[idx] * win[None, :], axis=1)) ** 2
        for b in range(BANDS):
            E[t0:t1, b] = P[:, e[b]:e[b + 1]].sum(axis=1)              # an empty band sums to 0
    return E


def haitsma_bits64(x5k, fmin=300.0, fmax=2000.0):
    """-> (dd, scale), float64 [T, 32] each: dd[t, b] = (E[t, b] - E[t, b+1]) - (E[t-1, b] - E[t-1, b+1]) with a zero row
    before frame 0; scale[t, b] = the sum of those four energies.  Bit b of frame t is dd[t, b] > 0."""
    E = band_energies64(x5k, fmin, fmax)
    Ep = np.concatenate([np.zeros((1, BANDS)), E[:-1]], axis=0) if E.shape[0] else E
    dd = (E[:, :-1] - E[:, 1:]) - (Ep[:, :-1] - Ep[:, 1:])
    scale = E[:, :-1] + E[:, 1:] + Ep[:, :-1] + Ep[:, 1:]
    return dd, scale


def unpack_bits(frames) -> np.ndarray:
    """uint32 [T] -> bool [T, 32], column b = bit b."""
    f = np.asarray(frames, dtype=np.uint32).reshape(-1)
    return ((f[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)).astype(bool)
