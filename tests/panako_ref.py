"""CPU restatement of the Panako triplet spec, shared by the Panako tests.

The front end is the oracle's (`oracle.stft_power(x, 1024, 128)`, `oracle.wang_peaks(P, peaks_per_sec)`); everything
after the peaks is restated here in numpy / plain Python, twice: `triplets` walks the peaks the way the device does
(P3 + P4), `triplets_literal` reads the definition literally (all targets of the zone, all pairs b < c, sorted by
(c, b), the first fan_out).  `wang_pairs` is the walk with P4 switched off: it must reproduce `oracle.wang`.

Records are uint32 [n, 4] arrays of (hash, t_a, t_b, t_c)."""
from dataclasses import dataclass

import numpy as np

SR, N_FFT, HOP = 8000, 1024, 128


@dataclass
class Cfg:
    fan_out: int = 5
    target_zone_t: int = 96
    target_zone_f: int = 96
    peaks_per_sec: int = 30
    min_anchor_mag_db: float = -50.0

    def astuple(self):
        return (self.fan_out, self.target_zone_t, self.target_zone_f, self.peaks_per_sec, self.min_anchor_mag_db)


def floor_power(db: float) -> np.float32:
    """P2: (float)(65536 * 10^(dB / 10)), evaluated in double from the float32 config field."""
    return np.float32(65536.0 * 10.0 ** (float(np.float32(db)) / 10.0))


def max_hashes(n_samples: int, cfg: Cfg) -> int:
    """P6: seconds * peaks_per_sec * fan_out, the formula of ucfp_audio_wang_max_hashes."""
    if n_samples < N_FFT:
        return 0
    frames = 1 + (n_samples - N_FFT) // HOP
    return (((frames - 1) * HOP) // SR + 1) * cfg.peaks_per_sec * cfg.fan_out


def peaks(oracle, x, peaks_per_sec: int):
    """P1: the clip's peaks ordered by (t, k): int64 t, int64 k, float32 p."""
    P = oracle.stft_power(np.ascontiguousarray(x, np.float32), N_FFT, HOP)
    t, k, p = oracle.wang_peaks(P, peaks_per_sec)
    order = np.lexsort((k, t))
    return t[order].astype(np.int64), k[order].astype(np.int64), p[order]


def _walk(t, k, i, zone_t, zone_f):
    """P3: the qualifying peaks of anchor i, in walk order (a generator, so that a caller can stop early)."""
    for j in range(i + 1, t.size):
        dt = int(t[j] - t[i])
        if dt <= 0:
            continue
        if dt > zone_t:
            break
        if abs(int(k[j] - k[i])) > zone_f:
            continue
        yield j


def _record(t, k, i, b, c):
    r = min(31, (32 * int(t[b] - t[i])) // int(t[c] - t[i]))
    return ((int(k[i]) << 23) | (int(k[b]) << 14) | (int(k[c]) << 5) | r, int(t[i]), int(t[b]), int(t[c]))


def triplets(t, k, p, cfg: Cfg, per_anchor=None) -> np.ndarray:
    """P2-P5 by the walk.  `per_anchor`, if a list, receives the number of triplets of every peak."""
    fl = floor_power(cfg.min_anchor_mag_db)
    out = []
    for i in range(t.size):
        n = 0
        if p[i] >= fl:
            q = []
            for j in _walk(t, k, i, cfg.target_zone_t, cfg.target_zone_f):
                for b in q:
                    if n >= cfg.fan_out:
                        break
                    out.append(_record(t, k, i, b, j))
                    n += 1
                q.append(j)
                if n >= cfg.fan_out:
                    break
        if per_anchor is not None:
            per_anchor.append(n)
    return np.array(out, np.uint64).astype(np.uint32).reshape(-1, 4)


def triplets_literal(t, k, p, cfg: Cfg) -> np.ndarray:
    """The definition read literally: every target of the zone, every pair b < c, sorted by (c, b), the first fan_out."""
    fl = floor_power(cfg.min_anchor_mag_db)
    out = []
    for i in range(t.size):
        if not p[i] >= fl:
            continue
        zone = [j for j in range(i + 1, t.size)
                if 0 < t[j] - t[i] <= cfg.target_zone_t and abs(int(k[j] - k[i])) <= cfg.target_zone_f]
        pairs = sorted((c, b) for b in zone for c in zone if b < c)
        out.extend(_record(t, k, i, b, c) for c, b in pairs[: cfg.fan_out])
    return np.array(out, np.uint64).astype(np.uint32).reshape(-1, 4)


def wang_pairs(t, k, p, cfg: Cfg) -> np.ndarray:
    """The same walk with P4 switched off: one Wang landmark per target, fan_out targets per anchor (A6)."""
    fl = floor_power(cfg.min_anchor_mag_db)
    out = []
    for i in range(t.size):
        if not p[i] >= fl:
            continue
        n = 0
        for j in _walk(t, k, i, cfg.target_zone_t, cfg.target_zone_f):
            out.append(((int(k[i]) << 23) | (int(k[j]) << 14) | (int(t[j] - t[i]) & 0x3FFF), int(t[i])))
            n += 1
            if n >= cfg.fan_out:
                break
    return np.array(out, np.uint64).astype(np.uint32).reshape(-1, 2)


def panako_ref(oracle, x, cfg: Cfg = None, per_anchor=None) -> np.ndarray:
    """8 kHz mono f32 -> the Panako records of the clip, uint32 [n, 4]."""
    cfg = cfg or Cfg()
    t, k, p = peaks(oracle, x, cfg.peaks_per_sec)
    return triplets(t, k, p, cfg, per_anchor)


def landmarks(rec) -> np.ndarray:
    """P7: the (hash, t_anchor) projection of a record."""
    return np.ascontiguousarray(np.asarray(rec, np.uint32).reshape(-1, 4)[:, :2])


# ---- signals shared by the tests ---------------------------------------------------------------------------------

def signal(kind: str, seconds: float, seed: int = 0, sr: int = SR) -> np.ndarray:
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    if kind == "noise":
        return (0.2 * rng.standard_normal(n)).astype(np.float32)
    if kind == "quiet":          # 1e-4 noise: no peak passes the default anchor floor
        return (1e-4 * rng.standard_normal(n)).astype(np.float32)
    if kind == "sine440":
        return (0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    if kind == "chirps":         # eight log-spaced chirps of seeded start and rate, plus noise at -30 dB
        x = np.zeros(n)
        for i in range(8):
            f0 = 100.0 * (1.5 ** i) * rng.uniform(0.9, 1.1)
            rate = rng.uniform(0.05, 0.4) * f0
            x += 0.06 * np.sin(2 * np.pi * (f0 * t + 0.5 * rate * t * t / max(seconds, 1e-3)) + rng.uniform(0, 6.28))
        x += 0.0316 * 0.5 * rng.standard_normal(n)
        return np.clip(x, -0.5, 0.5).astype(np.float32)
    raise ValueError(kind)


# identification (P7): 8 recordings of 20 s, alternating chirps and noise; excerpts that start on a multiple of 2 s
# (125 frames and a whole number of seconds, so the frame grid and the per-second peak cap both line up)
N_RECORDINGS, RECORDING_S = 8, 20
EXCERPTS = ((2, 3.0), (4, 4.5), (10, 6.0))      # (start s, length s)
FRAMES_PER_S = 62.5


def recording(i: int) -> np.ndarray:
    return signal("chirps" if i % 2 == 0 else "noise", RECORDING_S, seed=7100 + i)


def excerpt(x: np.ndarray, start_s: int, length_s: float) -> np.ndarray:
    return x[start_s * SR: start_s * SR + int(length_s * SR)]
