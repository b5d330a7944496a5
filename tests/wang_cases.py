"""Clips that drive the Wang front end to the limits its kernels are built around, shared by
tests/test_wang_peaks_spec.py (the oracle against a numpy restatement, and each clip's reason to exist) and
tests/test_wang_edges_gpu.py (the kernels against the oracle).

Every clip is 8 kHz mono float32 and at most 3 s long.  A clip is built once per process and handed out read-only."""
import functools

import numpy as np

SR, N_FFT, HOP, BINS = 8000, 1024, 128, 512
N3 = 3 * SR                                   # 180 frames: seconds of 63, 62 and 55 frames
BAD = 12000                                   # a sample in the middle of N3: frames 86 .. 93 hold it

PERIODS = (896, 1024, 1152)
COMB_PERIODS = (1024, 896)
NONFINITE_KINDS = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}
NONFINITE_WHERE = ("first", "last", "mid", "pair15", "pair9")
SCALES = (1e-22, 1e-19, 1e17, 1e19, 1e35)


def frames_of(n: int) -> int:
    return 1 + (n - N_FFT) // HOP if n >= N_FFT else 0


def samples_for(frames: int) -> int:
    return N_FFT + HOP * (frames - 1) if frames else 0


def _ro(x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def _lattice64() -> np.ndarray:
    """An impulse every 64 samples (so every 16th bin of every frame carries the same power) under a 1024-sample
    cosine envelope: 32 row-local candidates in every frame, a peak row every 8 frames."""
    i = np.arange(N3)
    x = np.zeros(N3)
    x[::64] = 0.5
    return x * (1.0 + 0.5 * np.cos(2 * np.pi * i / 1024))


@functools.lru_cache(maxsize=None)
def lattice_tied() -> np.ndarray:
    """704 peaks, 32 in a row, 256 in a second, all of exactly the same power."""
    return _ro(_lattice64())


@functools.lru_cache(maxsize=None)
def lattice_distinct() -> np.ndarray:
    """The same lattice with every power of a second different."""
    return _ro(_lattice64() + 1e-3 * np.random.default_rng(101).standard_normal(N3))


@functools.lru_cache(maxsize=None)
def lattice_partial() -> np.ndarray:
    """The same lattice where noise at float32's resolution splits the powers into a few dozen levels: ranks are decided
    by the power for some peaks and by (t, k) for others, inside one second."""
    return _ro(_lattice64() + 1e-6 * np.random.default_rng(102).standard_normal(N3))


@functools.lru_cache(maxsize=None)
def am_tones() -> np.ndarray:
    """32 tones on bin centres 8 + 16 j, each under its own 1024-sample envelope: about as many peaks per second as the
    lattice, but a few per frame -- many frames (waves) add to one second's list instead of one frame adding 32."""
    rng = np.random.default_rng(103)
    i = np.arange(N3)
    x = np.zeros(N3)
    for j in range(32):
        f = (8 + 16 * j) * SR / N_FFT
        env = 1.0 + 0.8 * np.cos(2 * np.pi * i / 1024 + rng.uniform(0, 2 * np.pi))
        x += 0.02 * np.sin(2 * np.pi * f * i / SR + rng.uniform(0, 2 * np.pi)) * env
    return _ro(x)


LATTICES = {"lattice_tied": lattice_tied, "lattice_distinct": lattice_distinct, "lattice_partial": lattice_partial,
            "am_tones": am_tones}


@functools.lru_cache(maxsize=None)
def period(p: int) -> np.ndarray:
    """float32 noise of period p over 120 frames: frames t and t + p / 128 are bit-identical, so every cell ties with the
    cells 7 (inside the window), 8 or 9 (outside it) frames away."""
    assert p % HOP == 0
    n = samples_for(120)
    pat = (0.2 * np.random.default_rng(p).standard_normal(p)).astype(np.float32)
    return _ro(np.tile(pat, n // p + 1)[:n])


@functools.lru_cache(maxsize=None)
def comb(p: int, frames: int = 0) -> np.ndarray:
    """An impulse every 64 samples with a random height per tooth, repeating after p samples: ties 16 bins apart are
    broken by the teeth, ties p / 128 frames apart are exact.  `frames` cuts the clip (default: 3 s)."""
    assert p % 64 == 0
    n = samples_for(frames) if frames else N3
    pat = np.zeros(p)
    pat[::64] = 0.5 * (1.0 + 0.3 * np.random.default_rng(7).uniform(size=p // 64))
    return _ro(np.tile(pat.astype(np.float32), n // p + 1)[:n])


@functools.lru_cache(maxsize=None)
def noise3() -> np.ndarray:
    return _ro(0.2 * np.random.default_rng(104).standard_normal(N3))


def nonfinite_at(where: str):
    """The poisoned sample indices of a `nonfinite` clip."""
    last = samples_for(frames_of(N3)) - 1
    return {"first": (0,), "last": (last,), "mid": (BAD,), "pair15": (BAD, BAD + 15 * HOP),
            "pair9": (BAD, BAD + 9 * HOP)}[where]


@functools.lru_cache(maxsize=None)
def nonfinite(kind: str, where: str) -> np.ndarray:
    """3 s of noise with one sample (pair*: two) replaced by NaN, +Inf or -Inf.  A bad sample turns the 8 frames that
    hold it into all-NaN rows.  pair15: two runs with 7 finite frames between them (the first of those has only NaN
    rows before it, the last only NaN rows after it); pair9: ONE finite frame with nothing but NaN rows on both sides."""
    x = noise3().copy()
    for i in nonfinite_at(where):
        x[i] = NONFINITE_KINDS[kind]
    return _ro(x)


@functools.lru_cache(maxsize=None)
def scaled(a: float) -> np.ndarray:
    """The noise clip times a: denormal and zero powers at the small end, powers that overflow to +Inf at the large."""
    return _ro((noise3().astype(np.float64) * a).astype(np.float32))


@functools.lru_cache(maxsize=None)
def short_noise() -> np.ndarray:
    return _ro(0.2 * np.random.default_rng(105).standard_normal(int(0.3 * SR)))


# (fan_out, target_zone_t, target_zone_f, peaks_per_sec, dB): the lattice's peaks are 8 frames and 16 bins apart, so
# dt == target_zone_t and |df| == target_zone_f decide
ZONES = ((64, 8, 16, 256, -200.0), (64, 7, 15, 256, -200.0), (64, 8, 15, 256, -200.0), (1, 512, 1, 256, -200.0),
         (64, 512, 1024, 256, -200.0))


def mid_floor_db(oracle) -> float:
    """A float32 dB whose floor power 65536 * 10^(dB / 10) falls strictly between two adjacent peak powers near the
    median of lattice_distinct: derived in float64 from the midpoint of the widest gap among the middle 5 %."""
    _, _, p = oracle.wang_peaks(oracle.stft_power(lattice_distinct(), N_FFT, HOP), 256)
    u = np.unique(p).astype(np.float64)
    lo = u.size // 2 - u.size // 40
    i = lo + int(np.argmax(np.diff(u[lo:lo + u.size // 20 + 1])))
    db = float(np.float32(10.0 * np.log10(0.5 * (u[i] + u[i + 1]) / 65536.0)))
    floor = float(np.float32(65536.0 * 10.0 ** (db / 10.0)))
    assert u[i] < floor < u[i + 1], (u[i], floor, u[i + 1])
    assert 0.4 * p.size < (p >= np.float32(floor)).sum() < 0.6 * p.size
    return db


def all_cases():
    """(name, clip) of every generator above, for the spec test."""
    for name, f in LATTICES.items():
        yield name, f()
    for p in PERIODS:
        yield f"period{p}", period(p)
    for p in COMB_PERIODS:
        yield f"comb{p}", comb(p)
    for kind in NONFINITE_KINDS:
        for where in NONFINITE_WHERE:
            yield f"nonfinite-{kind}-{where}", nonfinite(kind, where)
    for a in SCALES:
        yield f"scaled{a:g}", scaled(a)
