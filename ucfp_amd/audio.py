"""Audio fingerprinting -- host-side mirror of src/modality/audio.rs.

    fingerprint_wang(samples, sample_rate, tenant_id, record_id)              audio.rs:46-60
    fingerprint_wang_with(samples, sample_rate, cfg, tenant_id, record_id)    audio.rs:64-98
    fingerprint_panako / fingerprint_panako_with                              audio.rs:106-156
    fingerprint_haitsma / fingerprint_haitsma_with                            audio.rs:164-224
    StreamingWangSession(sample_rate, tenant_id, record_id).push/.finalize    audio.rs:414-480
    HaitsmaStreams / StreamingHaitsmaSession                                  DESIGN.md A18 (no reference counterpart)
    PanakoStreams / StreamingPanakoSession                                    DESIGN.md A19 (no reference counterpart)

All DSP runs in the HIP library through the C ABI (ucfp_audio_*); this module validates arguments
the way the reference does and wraps bytes into `Record`s.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib
from ._streams import AudioStreamSet
from .core import Modality, Record
from .errors import ModalityError

ALGORITHM_WANG = "audiofp-wang-v1"
ALGORITHM_PANAKO = "audiofp-panako-v1"
ALGORITHM_HAITSMA = "audiofp-haitsma-v1"
WANG_SR, HAITSMA_SR = 8000, 5000


@dataclass
class WangConfig:
    """audiofp::classical::WangConfig; defaults src/server/algorithms_manifest.rs:553-592."""
    fan_out: int = 10
    target_zone_t: int = 63
    target_zone_f: int = 64
    peaks_per_sec: int = 30
    min_anchor_mag_db: float = -50.0

    def _c(self):
        return _lib.WangConfig(self.fan_out, self.target_zone_t, self.target_zone_f, self.peaks_per_sec,
                               self.min_anchor_mag_db)


@dataclass
class PanakoConfig:
    """audiofp::classical::PanakoConfig; defaults and ranges src/server/algorithms_manifest.rs:601-650."""
    fan_out: int = 5
    target_zone_t: int = 96
    target_zone_f: int = 96
    peaks_per_sec: int = 30
    min_anchor_mag_db: float = -50.0

    def _c(self):
        return _lib.PanakoConfig(self.fan_out, self.target_zone_t, self.target_zone_f, self.peaks_per_sec,
                                 self.min_anchor_mag_db)


@dataclass
class HaitsmaConfig:
    """audiofp::classical::HaitsmaConfig; defaults manifest :655-672."""
    fmin: float = 300.0
    fmax: float = 2000.0

    def _c(self):
        return _lib.HaitsmaConfig(self.fmin, self.fmax)


def _check_rate(sample_rate: int):
    if not (0 < int(sample_rate) <= 384_000):
        raise ModalityError(f"invalid sample rate {sample_rate}")   # audio.rs:74-75


def wang_hashes(samples, sample_rate: int, cfg: Optional[WangConfig] = None, ctx=None) -> np.ndarray:
    """-> uint32 [n, 2]: (packed hash, t_anchor) -- the byte image of audiofp's [WangHash]."""
    ctx = ctx or _lib.current_context()
    _check_rate(sample_rate)
    x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    c = (cfg or WangConfig())._c()
    lib = _lib.load()
    cap = max(1, int(lib.ucfp_audio_wang_max_hashes(x.size, C.byref(c))))
    out = np.zeros((cap, 2), np.uint32)
    n = C.c_size_t(0)
    _lib.check(lib.ucfp_audio_wang(ctx.handle, x.ctypes.data, x.size, sample_rate, C.byref(c), out.ctypes.data,
                                   cap, C.byref(n)))
    return out[: n.value].copy()


def wang_hashes_batch_dev(pcm_ptr: int, offsets_ptr: int, n_total: int, n_clips: int, sample_rate: int, out_ptr: int,
                          cap_hashes: int, out_offsets_ptr: int, cfg: Optional[WangConfig] = None, stream: int = 0,
                          ctx=None) -> None:
    """Ragged batch of clips, device pointers, no sync (ucfp_audio_wang_batch_dev): clip i = pcm[offsets[i] ..
    offsets[i+1]) at `sample_rate` (resampled to 8 kHz in the kernel unless it is 8000)."""
    ctx = ctx or _lib.current_context()
    c = (cfg or WangConfig())._c()
    _lib.check(_lib.load().ucfp_audio_wang_batch_dev(ctx.handle, pcm_ptr or None, offsets_ptr or None, n_total, n_clips,
                                                     sample_rate, C.byref(c), out_ptr or None, cap_hashes,
                                                     out_offsets_ptr, stream or None))


def wang_hashes_batch(clips, sample_rate: int, cfg: Optional[WangConfig] = None, ctx=None) -> List[np.ndarray]:
    """Host convenience over the batch entry: a list of mono f32 clips (all at `sample_rate`) -> one uint32 [n_i, 2]
    array per clip.  One launch sequence for the whole batch."""
    import torch
    ctx = ctx or _lib.current_context()
    _check_rate(sample_rate)
    arrs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
    if not arrs:
        return []
    offs = np.zeros(len(arrs) + 1, np.uint64)
    np.cumsum([a.size for a in arrs], out=offs[1:])
    blob = np.concatenate(arrs) if offs[-1] else np.zeros(1, np.float32)
    c = (cfg or WangConfig())._c()
    cap = max(1, int(_lib.load().ucfp_audio_wang_batch_max_hashes(int(offs[-1]), len(arrs), sample_rate, C.byref(c))))
    dev = f"cuda:{ctx.device}"
    d_pcm = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_out = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    d_oo = torch.zeros(len(arrs) + 1, dtype=torch.int64, device=dev)
    wang_hashes_batch_dev(d_pcm.data_ptr(), d_off.data_ptr(), int(offs[-1]), len(arrs), sample_rate, d_out.data_ptr(), cap,
                          d_oo.data_ptr(), cfg, torch.cuda.current_stream().cuda_stream, ctx)
    oo = d_oo.cpu().numpy()
    out = d_out.cpu().numpy().view(np.uint32)
    if oo[-1] > cap:
        raise ModalityError(f"Wang batch produced {oo[-1]} hashes, buffer holds {cap}")
    return [out[oo[i]:oo[i + 1]].copy() for i in range(len(arrs))]


class WangBatcher:
    """Host micro-batcher for clips (handlers.rs:704-918 fingerprints one clip per request): concurrent
    `submit` calls become one ucfp_audio_wang_batch_dev launch sequence.  All clips at `sample_rate`."""

    def __init__(self, sample_rate: int = WANG_SR, cfg: Optional[WangConfig] = None, *, max_batch: int = 1024,
                 max_samples: int = 64 << 20, max_delay_us: int = 500, ctx=None):
        _check_rate(sample_rate)
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.sample_rate = sample_rate
        self._cfg = (cfg or WangConfig())._c()
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_audio_batcher_create(self.ctx.handle, sample_rate, C.byref(self._cfg), max_batch,
                                                       max_samples, max_delay_us, C.byref(h)))
        self.handle = h

    def submit(self, samples) -> np.ndarray:
        """-> uint32 [n, 2] hashes of this clip.  Blocks until they are ready."""
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        cap = max(1, int(self._lib.ucfp_audio_wang_batch_max_hashes(x.size, 1, self.sample_rate, C.byref(self._cfg))))
        out = np.zeros((cap, 2), np.uint32)
        n = C.c_size_t(0)
        _lib.check(self._lib.ucfp_audio_batcher_submit(self.handle, x.ctypes.data, x.size, out.ctypes.data, cap,
                                                       C.byref(n)))
        return out[: n.value].copy()

    def stats(self):
        b, i = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.ucfp_audio_batcher_stats(self.handle, C.byref(b), C.byref(i)))
        return int(b.value), int(i.value)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_audio_batcher_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _aligned_records(cap: int) -> np.ndarray:
    """uint32 [cap, 4] whose data is 16-byte aligned (the Panako entries require it)."""
    raw = np.zeros(cap * 16 + 16, np.uint8)
    skip = -raw.ctypes.data % 16
    return raw[skip: skip + cap * 16].view(np.uint32).reshape(cap, 4)


def panako_hashes(samples, sample_rate: int, cfg: Optional[PanakoConfig] = None, ctx=None) -> np.ndarray:
    """-> uint32 [n, 4]: (hash, t_anchor, t_b, t_c) -- the byte image of audiofp's [PanakoHash] (DESIGN A13)."""
    ctx = ctx or _lib.current_context()
    _check_rate(sample_rate)
    x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    c = (cfg or PanakoConfig())._c()
    lib = _lib.load()
    cap = max(1, int(lib.ucfp_audio_panako_max_hashes(x.size, C.byref(c))))
    out = _aligned_records(cap)
    n = C.c_size_t(0)
    _lib.check(lib.ucfp_audio_panako(ctx.handle, x.ctypes.data, x.size, sample_rate, C.byref(c), out.ctypes.data,
                                     cap, C.byref(n)))
    return out[: n.value].copy()


def panako_hashes_batch_dev(pcm_ptr: int, offsets_ptr: int, n_total: int, n_clips: int, sample_rate: int, out_ptr: int,
                            cap_hashes: int, out_offsets_ptr: int, cfg: Optional[PanakoConfig] = None, stream: int = 0,
                            ctx=None) -> None:
    """Ragged batch of clips, device pointers, no sync (ucfp_audio_panako_batch_dev): clip i = pcm[offsets[i] ..
    offsets[i+1]) at `sample_rate` (resampled to 8 kHz in the kernel unless it is 8000); `out_ptr` 16-byte aligned."""
    ctx = ctx or _lib.current_context()
    c = (cfg or PanakoConfig())._c()
    _lib.check(_lib.load().ucfp_audio_panako_batch_dev(ctx.handle, pcm_ptr or None, offsets_ptr or None, n_total, n_clips,
                                                       sample_rate, C.byref(c), out_ptr or None, cap_hashes,
                                                       out_offsets_ptr, stream or None))


def panako_hashes_batch(clips, sample_rate: int, cfg: Optional[PanakoConfig] = None, ctx=None) -> List[np.ndarray]:
    """Host convenience over the batch entry: a list of mono f32 clips (all at `sample_rate`) -> one uint32 [n_i, 4]
    array per clip.  One launch sequence for the whole batch."""
    import torch
    ctx = ctx or _lib.current_context()
    _check_rate(sample_rate)
    arrs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
    if not arrs:
        return []
    offs = np.zeros(len(arrs) + 1, np.uint64)
    np.cumsum([a.size for a in arrs], out=offs[1:])
    blob = np.concatenate(arrs) if offs[-1] else np.zeros(1, np.float32)
    c = (cfg or PanakoConfig())._c()
    cap = max(1, int(_lib.load().ucfp_audio_panako_batch_max_hashes(int(offs[-1]), len(arrs), sample_rate, C.byref(c))))
    dev = f"cuda:{ctx.device}"
    d_pcm = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_out = torch.zeros((cap, 4), dtype=torch.int32, device=dev)
    d_oo = torch.zeros(len(arrs) + 1, dtype=torch.int64, device=dev)
    panako_hashes_batch_dev(d_pcm.data_ptr(), d_off.data_ptr(), int(offs[-1]), len(arrs), sample_rate, d_out.data_ptr(),
                            cap, d_oo.data_ptr(), cfg, torch.cuda.current_stream().cuda_stream, ctx)
    oo = d_oo.cpu().numpy()
    out = d_out.cpu().numpy().view(np.uint32)
    if oo[-1] > cap:
        raise ModalityError(f"Panako batch produced {oo[-1]} hashes, buffer holds {cap}")
    return [out[oo[i]:oo[i + 1]].copy() for i in range(len(arrs))]


def panako_landmarks(record_bytes) -> np.ndarray:
    """The identification projection of a Panako record (DESIGN A13, P7): its (hash, t_anchor) pairs, 8 bytes out of
    each 16, as uint32 [n, 2] -- what a LandmarkIndex stores and is queried with."""
    if isinstance(record_bytes, (bytes, bytearray, memoryview)):
        if len(record_bytes) % 16:
            raise ModalityError("a Panako record is a multiple of 16 bytes (u32 hash, t_anchor, t_b, t_c)")
        rec = np.frombuffer(bytes(record_bytes), "<u4")
    else:
        rec = np.ascontiguousarray(record_bytes, dtype=np.uint32)
    return np.ascontiguousarray(rec.reshape(-1, 4)[:, :2])


def haitsma_frames(samples, sample_rate: int, cfg: Optional[HaitsmaConfig] = None, ctx=None) -> np.ndarray:
    ctx = ctx or _lib.current_context()
    _check_rate(sample_rate)
    x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    c = (cfg or HaitsmaConfig())._c()
    lib = _lib.load()
    cap = max(1, int(lib.ucfp_audio_haitsma_frames(x.size, sample_rate)))
    out = np.zeros(cap, np.uint32)
    n = C.c_size_t(0)
    _lib.check(lib.ucfp_audio_haitsma(ctx.handle, x.ctypes.data, x.size, sample_rate, C.byref(c), out.ctypes.data,
                                      cap, C.byref(n)))
    return out[: n.value].copy()


def haitsma_frames_batch(clips, sample_rate: int, cfg: Optional[HaitsmaConfig] = None, ctx=None) -> List[np.ndarray]:
    """A list of mono f32 clips (all at `sample_rate`) -> one uint32 [frames_i] array per clip, one launch sequence for
    the whole batch (ucfp_audio_haitsma_batch_dev)."""
    import torch
    ctx = ctx or _lib.current_context()
    _check_rate(sample_rate)
    arrs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
    if not arrs:
        return []
    offs = np.zeros(len(arrs) + 1, np.uint64)
    np.cumsum([a.size for a in arrs], out=offs[1:])
    blob = np.concatenate(arrs) if offs[-1] else np.zeros(1, np.float32)
    c = (cfg or HaitsmaConfig())._c()
    lib = _lib.load()
    cap = max(1, int(lib.ucfp_audio_haitsma_batch_max_frames(int(offs[-1]), len(arrs), sample_rate)))
    dev = f"cuda:{ctx.device}"
    d_pcm = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_out = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_oo = torch.zeros(len(arrs) + 1, dtype=torch.int64, device=dev)
    _lib.check(lib.ucfp_audio_haitsma_batch_dev(ctx.handle, d_pcm.data_ptr(), d_off.data_ptr(), int(offs[-1]), len(arrs),
                                                sample_rate, C.byref(c), d_out.data_ptr(), cap, d_oo.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream or None))
    oo = d_oo.cpu().numpy()
    out = d_out.cpu().numpy().view(np.uint32)
    return [out[oo[i]:oo[i + 1]].copy() for i in range(len(arrs))]


def _record(algo: str, payload: bytes, tenant_id: int, record_id: int) -> Record:
    # format_version 1, config_hash 0: audio.rs:89-91
    return Record(tenant_id=tenant_id, record_id=record_id, modality=Modality.Audio, format_version=1,
                  algorithm=algo, config_hash=0, fingerprint=payload, embedding=None, model_id=None, metadata=b"",
                  text=None)


def fingerprint_wang(samples, sample_rate: int, tenant_id: int, record_id: int) -> Record:
    return fingerprint_wang_with(samples, sample_rate, WangConfig(), tenant_id, record_id)


def fingerprint_wang_with(samples, sample_rate: int, cfg: WangConfig, tenant_id: int, record_id: int) -> Record:
    return _record(ALGORITHM_WANG, wang_hashes(samples, sample_rate, cfg).tobytes(), tenant_id, record_id)


def fingerprint_panako(samples, sample_rate: int, tenant_id: int, record_id: int) -> Record:
    return fingerprint_panako_with(samples, sample_rate, PanakoConfig(), tenant_id, record_id)


def fingerprint_panako_with(samples, sample_rate: int, cfg: PanakoConfig, tenant_id: int, record_id: int) -> Record:
    # tag, format_version 1, config_hash 0: audio.rs:141-155
    return _record(ALGORITHM_PANAKO, panako_hashes(samples, sample_rate, cfg).tobytes(), tenant_id, record_id)


def fingerprint_haitsma(samples, sample_rate: int, tenant_id: int, record_id: int) -> Record:
    return fingerprint_haitsma_with(samples, sample_rate, HaitsmaConfig(), tenant_id, record_id)


def fingerprint_haitsma_with(samples, sample_rate: int, cfg: HaitsmaConfig, tenant_id: int, record_id: int) -> Record:
    return _record(ALGORITHM_HAITSMA, haitsma_frames(samples, sample_rate, cfg).tobytes(), tenant_id, record_id)


class WangStreams(AudioStreamSet):
    """A set of live Wang streams on the device (ucfp_wang_streams_*): `push` advances any subset of them
    by one chunk each with one launch sequence and returns the hashes each one emits now -- exactly the offline hashes
    with t_anchor < frontier(n) so far, the rest on the final push (t_anchor = frames since `open`).  With
    `window_frames` = W > 0, `windows` hands out each stream's latest W frames of hashes, rebased to the
    window's origin, in the ragged shape `LandmarkIndex.query_dev` / ucfp_landmark_index_query_dev take.  With
    `resample=True` the set takes its feed at any `sample_rate` from 1 to 384 kHz and resamples it on
    the device: counts are input samples, the pushes add up to `wang_hashes_batch` of the feed at that rate, and times
    and windows stay in 8 kHz frames."""
    _abi, _cap_entry, _row = "ucfp_wang_streams", "max_hashes", (2,)

    def __init__(self, max_streams: int, cfg: Optional[WangConfig] = None, sample_rate: int = WANG_SR, ctx=None, *,
                 window_frames: int = 0, resample: bool = False):
        self._cfg = (cfg or WangConfig())._c()
        self._create(ctx, "create_sr" if resample else "create_ex", sample_rate, C.byref(self._cfg), max_streams,
                     window_frames)
        self.max_streams, self.window_frames = max_streams, window_frames
        self.sample_rate = sample_rate
        self.window_cap = int(self._lib.ucfp_wang_streams_window_cap(C.byref(self._cfg), window_frames))

    def final_samples(self, n_samples: int, final: bool = False) -> int:
        """S(n): the 8 kHz samples of a stream that are final once it has received n samples at the set's rate."""
        return int(self._lib.ucfp_wang_stream_samples(n_samples, self.sample_rate, 1 if final else 0))

    def frontier(self, n_samples: int) -> int:
        """F(n), n in samples at the set's rate: after a non-final push, every hash with t_anchor < F(n) has been
        emitted, and no other."""
        return int(self._lib.ucfp_wang_stream_frontier(self.final_samples(n_samples), C.byref(self._cfg)))

    max_hashes = AudioStreamSet._max_rows

    def push_dev(self, slots, counts, pcm, out, out_offsets, final=(), cap_hashes: Optional[int] = None,
                 stream: int = 0) -> None:
        """Device variant (no sync): `pcm` the chunks of `slots` concatenated (float32 tensor), `out` an int32 [cap, 2]
        tensor, `out_offsets` an int64 [len(slots) + 1] tensor; hashes of slots[i] = out[out_offsets[i]:out_offsets[i+1]]."""
        self._push_dev(slots, counts, pcm, out, out_offsets, final, cap_hashes, stream)

    def push(self, chunks: dict, final=()) -> dict:
        """{slot: samples} -> {slot: uint32 [n, 2]} of the hashes emitted now; slots in `final` end (and close)."""
        return self._push(chunks, final)

    def windows_dev(self, slots, landmarks, offsets, origins=None, cap_landmarks: Optional[int] = None,
                    stream: int = 0) -> None:
        """Device variant (no sync): the live window of slots[i] -> the bytes landmarks[offsets[i]:offsets[i+1]]
        (`landmarks` an int32 [cap, 2] tensor of at least len(slots) * window_cap hashes, `offsets` an int64
        [len(slots) + 1] tensor of BYTE offsets, `origins` an optional int32 [len(slots)] tensor of the windows' first
        frames)."""
        self._windows_dev(slots, landmarks, offsets, origins, cap_landmarks, stream)

    def windows(self, slots) -> dict:
        """{slot: (uint32 [m, 2] hashes rebased to the window's origin, origin)}, oldest hash first."""
        return self._windows(slots)


class _StreamingSession:
    """push / finalize on a one-slot audio set through its staged single-stream entry: each `push` moves its PCM to the
    device and advances the stream there; only the rows emitted so far are held on the host."""
    _algorithm = ""

    def _start(self, stream_set, tenant_id: int, record_id: int) -> None:
        self.tenant_id, self.record_id = tenant_id, record_id
        self._set = stream_set
        self._slot = self._set.open()
        self._n = 0                   # samples since the stream began
        self._rows: List[np.ndarray] = []

    def _cap(self, n_new: int, final: bool) -> int:
        return self._set._max_rows([self._slot], [n_new], [self._slot] if final else ())

    def _buffer(self, rows: int) -> np.ndarray:
        return np.zeros((rows, *self._set._row), np.uint32)

    def _push(self, samples, final: bool):
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        cap = self._cap(x.size, final)
        out = self._buffer(max(cap, 1))
        n = C.c_size_t(0)
        _lib.check(self._set._fn("push")(self._set.handle, self._slot, x.ctypes.data if x.size else None, x.size,
                                         1 if final else 0, out.ctypes.data, cap, C.byref(n)))
        self._n += x.size
        if n.value:
            self._rows.append(out[: n.value].copy())

    def push(self, samples) -> List[Record]:
        self._push(samples, False)
        return []

    def finalize(self) -> List[Record]:
        self._push(np.zeros(0, np.float32), True)
        self._slot = self._set.open()           # the session may be reused
        self._n = 0
        rows, self._rows = self._rows, []
        if not rows:
            return []
        return [_record(self._algorithm, np.concatenate(rows).tobytes(), self.tenant_id, self.record_id)]


class StreamingWangSession(_StreamingSession):
    """Push/finalize wrapper (audio.rs:414-480) on a one-slot WangStreams: each `push` moves its PCM to the device and
    advances the stream there; only the hashes emitted so far are held on the host, so memory stays bounded however
    long the stream runs.  `push` returns no records -- allowed by the reference contract ("typically zero or one");
    `finalize` returns one record with every hash (the offline hashes of the whole stream, byte for byte)."""
    _algorithm = ALGORITHM_WANG

    def __init__(self, sample_rate: int, tenant_id: int, record_id: int, *, resample: bool = False):
        """`resample=True` (A21): any rate from 1 to 384 kHz, resampled on the device; `finalize` then returns the
        record of `wang_hashes_batch` at that rate."""
        if sample_rate != WANG_SR and not resample:
            raise ModalityError(f"Wang requires 8 kHz mono input (got {sample_rate} Hz); resample upstream")
        self._start(WangStreams(1, sample_rate=sample_rate, resample=resample), tenant_id, record_id)


class HaitsmaStreams(AudioStreamSet):
    """A set of live Haitsma streams on the device (ucfp_haitsma_streams_*): `push` advances any subset of
    them by one chunk each with one launch sequence and returns the sub-fingerprints each one emits now -- frames
    [Fr(before), Fr(after)) of its offline record, the rest on the final push.  `blocks` hands out each stream's latest
    `block_frames` sub-fingerprints in the ragged shape `HaitsmaIndex.identify_frames` / ucfp_haitsma_index_query_dev take."""
    _abi, _cap_entry, _row = "ucfp_haitsma_streams", "max_frames", ()

    def __init__(self, max_streams: int, sample_rate: int, cfg: Optional[HaitsmaConfig] = None, block_frames: int = 256,
                 ctx=None):
        self._cfg = (cfg or HaitsmaConfig())._c()
        # as ucfp_haitsma_streams_create: the rate and the band edges are judged before a device is asked for
        if not (1000 <= int(sample_rate) <= 384_000):
            raise ModalityError(f"invalid sample rate {sample_rate} (1 000 .. 384 000 Hz)")
        if not (1.0 <= self._cfg.fmin < self._cfg.fmax <= 2500.0):
            raise ModalityError("Haitsma band edges must satisfy 1 <= fmin < fmax <= 2500 Hz")
        self._create(ctx, "create", sample_rate, C.byref(self._cfg), max_streams, block_frames)
        self.max_streams, self.sample_rate, self.block_frames = max_streams, sample_rate, block_frames

    def emitted(self, n_samples: int, final: bool = False) -> int:
        """Fr(n): the frames a stream has emitted once it has received n samples (all of them after a final push)."""
        return int(self._lib.ucfp_haitsma_stream_frames(n_samples, self.sample_rate, 1 if final else 0))

    max_frames = AudioStreamSet._max_rows

    def push_dev(self, slots, counts, pcm, out, out_offsets, final=(), cap_frames: Optional[int] = None,
                 stream: int = 0) -> None:
        """Device variant (no sync): `pcm` the chunks of `slots` concatenated (float32 tensor), `out` an int32 [cap]
        tensor, `out_offsets` an int64 [len(slots) + 1] tensor; frames of slots[i] = out[out_offsets[i]:out_offsets[i+1]]."""
        self._push_dev(slots, counts, pcm, out, out_offsets, final, cap_frames, stream)

    def push(self, chunks: dict, final=()) -> dict:
        """{slot: samples} -> {slot: uint32 [n]} of the sub-fingerprints emitted now; slots in `final` end (and close)."""
        return self._push(chunks, final)

    def blocks_dev(self, slots, out, out_offsets, cap_frames: Optional[int] = None, stream: int = 0) -> None:
        """Device variant (no sync): the live block of slots[i] -> out[out_offsets[i]:out_offsets[i+1]] (`out` an int32
        tensor of at least len(slots) * block_frames, `out_offsets` an int64 [len(slots) + 1] tensor)."""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        cap = out.shape[0] if cap_frames is None else cap_frames
        _lib.check(self._lib.ucfp_haitsma_streams_blocks_dev(self.handle, sl.ctypes.data, sl.size,
                                                             out.data_ptr() if cap else None, cap, out_offsets.data_ptr(),
                                                             stream or None))

    def blocks(self, slots) -> dict:
        """{slot: uint32 [m]}: each stream's latest m = min(block_frames, frames emitted) sub-fingerprints, oldest first."""
        slots = list(slots)
        rows = self._ragged(len(slots), len(slots) * self.block_frames, (),
                            lambda out, oo, cap, st: self.blocks_dev(slots, out, oo, cap, st))
        return dict(zip(slots, rows))


class StreamingHaitsmaSession(_StreamingSession):
    """Push/finalize wrapper on a one-slot HaitsmaStreams, the shape of StreamingWangSession: each `push` moves its PCM to
    the device and advances the stream there; only the sub-fingerprints emitted so far are held on the host.  `push`
    returns no records; `finalize` returns one record equal to `fingerprint_haitsma_with` of the whole stream byte for
    byte, or none when the stream is too short for a frame."""
    _algorithm = ALGORITHM_HAITSMA

    def __init__(self, sample_rate: int, tenant_id: int, record_id: int, cfg: Optional[HaitsmaConfig] = None):
        self._start(HaitsmaStreams(1, sample_rate, cfg, block_frames=0), tenant_id, record_id)

    def _cap(self, n_new: int, final: bool) -> int:      # from the closed form, without a call into the set
        return self._set.emitted(self._n + n_new, final) - self._set.emitted(self._n)


class PanakoStreams(AudioStreamSet):
    """A set of live Panako streams on the device (ucfp_panako_streams_*): `push` advances any subset of
    them by one chunk each with one launch sequence and returns the records each one emits now -- exactly the offline
    records with t_a < frontier(n) so far, the rest on the final push (times = frames since `open`).  With
    `window_frames` = W > 0, `windows` hands out each stream's latest W frames of records, rebased to the window's
    origin, in the ragged shape `PanakoIndex.query_dev` / ucfp_panako_index_query_dev take.  With `resample=True`
     the set takes its feed at any `sample_rate` from 1 to 384 kHz and resamples it on the device: counts
    are input samples, the pushes add up to `panako_hashes_batch` of the feed at that rate, and times and windows stay
    in 8 kHz frames."""
    _abi, _cap_entry, _row = "ucfp_panako_streams", "max_hashes", (4,)

    def __init__(self, max_streams: int, cfg: Optional[PanakoConfig] = None, window_frames: int = 0,
                 sample_rate: int = WANG_SR, ctx=None, *, resample: bool = False):
        self._cfg = (cfg or PanakoConfig())._c()
        self._create(ctx, "create_sr" if resample else "create", sample_rate, C.byref(self._cfg), max_streams,
                     window_frames)
        self.max_streams, self.window_frames = max_streams, window_frames
        self.sample_rate = sample_rate
        self.window_cap = int(self._lib.ucfp_panako_streams_window_cap(C.byref(self._cfg), window_frames))

    def close(self, slot: int) -> None:
        """Discards the stream and its window; emits nothing."""
        super().close(slot)

    def final_samples(self, n_samples: int, final: bool = False) -> int:
        """S(n): the 8 kHz samples of a stream that are final once it has received n samples at the set's rate."""
        return int(self._lib.ucfp_wang_stream_samples(n_samples, self.sample_rate, 1 if final else 0))

    def frontier(self, n_samples: int) -> int:
        """F(n), n in samples at the set's rate: after a non-final push, every record with t_a < F(n) has been emitted,
        and no other."""
        return int(self._lib.ucfp_panako_stream_frontier(self.final_samples(n_samples), C.byref(self._cfg)))

    max_hashes = AudioStreamSet._max_rows

    def push_dev(self, slots, counts, pcm, out, out_offsets, final=(), cap_hashes: Optional[int] = None,
                 stream: int = 0) -> None:
        """Device variant (no sync): `pcm` the chunks of `slots` concatenated (float32 tensor), `out` an int32 [cap, 4]
        tensor (16-byte aligned), `out_offsets` an int64 [len(slots) + 1] tensor; records of slots[i] =
        out[out_offsets[i]:out_offsets[i+1]]."""
        self._push_dev(slots, counts, pcm, out, out_offsets, final, cap_hashes, stream)

    def push(self, chunks: dict, final=()) -> dict:
        """{slot: samples} -> {slot: uint32 [n, 4]} of the records emitted now; slots in `final` end (and close)."""
        return self._push(chunks, final)

    def windows_dev(self, slots, records, offsets, origins=None, cap_records: Optional[int] = None,
                    stream: int = 0) -> None:
        """Device variant (no sync): the live window of slots[i] -> the bytes records[offsets[i]:offsets[i+1]] (`records`
        an int32 [cap, 4] tensor of at least len(slots) * window_cap records, `offsets` an int64 [len(slots) + 1] tensor
        of BYTE offsets, `origins` an optional int32 [len(slots)] tensor of the windows' first frames)."""
        self._windows_dev(slots, records, offsets, origins, cap_records, stream)

    def windows(self, slots) -> dict:
        """{slot: (uint32 [m, 4] records rebased to the window's origin, origin)}, oldest record first."""
        return self._windows(slots)


class StreamingPanakoSession(_StreamingSession):
    """Push/finalize wrapper on a one-slot PanakoStreams, the shape of StreamingWangSession: each `push` moves its PCM
    to the device and advances the stream there; only the records emitted so far are held on the host.  `push` returns
    no records; `finalize` returns one record equal to `fingerprint_panako_with` of the whole stream byte for byte."""
    _algorithm = ALGORITHM_PANAKO

    def __init__(self, sample_rate: int, tenant_id: int, record_id: int, cfg: Optional[PanakoConfig] = None, *,
                 resample: bool = False):
        """`resample=True` (A21): any rate from 1 to 384 kHz, resampled on the device; `finalize` then returns the
        record of `panako_hashes_batch` at that rate."""
        if sample_rate != WANG_SR and not resample:
            raise ModalityError(f"Panako requires 8 kHz mono input (got {sample_rate} Hz); resample upstream")
        self._start(PanakoStreams(1, cfg, sample_rate=sample_rate, resample=resample), tenant_id, record_id)

    def _buffer(self, rows: int) -> np.ndarray:
        return _aligned_records(rows)
