"""What the device-resident stream sets share on the host side of the C ABI: audio.WangStreams, audio.HaitsmaStreams,
audio.PanakoStreams and text.MinHashStreams / text.SimHashStreams (the slot rules themselves live once in csrc/stream_slots.h).

A set's entries are `<_abi>_create*`, `_open`, `_close`, `_push_dev`, `_push`, `_destroy`.  The three audio kinds also
share the shape of a push -- float32 chunks in, ragged int32 rows out -- and differ in the capacity entry and the
trailing shape of a row.  The two kinds that keep live windows (Wang, Panako) share `_windows_dev` / `_windows`.
"""
import ctypes as C
from typing import List

import numpy as np

from . import _lib


def slot_arrays(slots, counts, final):
    """(slots, units per slot, the slots that end) -> the uint32 / uint64 / uint8 arrays a push entry takes."""
    final = set(final)
    sl = np.ascontiguousarray(slots, dtype=np.uint32)
    ns = np.ascontiguousarray(counts, dtype=np.uint64)
    fi = np.array([1 if s in final else 0 for s in sl.tolist()], np.uint8)
    return sl, ns, fi


class StreamSet:
    """Handle, `open`, `close` and `destroy` of a stream set."""
    _abi = ""                         # the prefix of the set's entries, e.g. "ucfp_wang_streams"

    def _fn(self, name: str):
        return getattr(self._lib, f"{self._abi}_{name}")

    def _create(self, ctx, entry: str, *args) -> None:
        """`<_abi>_<entry>(ctx, *args, &handle)` on `ctx` or the current context."""
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        h = C.c_void_p()
        _lib.check(self._fn(entry)(self.ctx.handle, *args, C.byref(h)))
        self.handle = h

    def open(self, *args) -> int:
        slot = C.c_uint32(0)
        _lib.check(self._fn("open")(self.handle, *args, C.byref(slot)))
        return int(slot.value)

    def close(self, slot: int) -> None:
        """Discards the stream; emits nothing."""
        _lib.check(self._fn("close")(self.handle, slot))

    def destroy(self):
        if getattr(self, "handle", None):
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class AudioStreamSet(StreamSet):
    """A set whose push takes float32 samples and emits rows of int32 [*_row] per slot."""
    _cap_entry = ""                   # "max_hashes" / "max_frames": the rows a push can emit
    _row = ()                         # trailing shape of an output row

    def _max_rows(self, slots, counts, final=()) -> int:
        sl, ns, fi = slot_arrays(slots, counts, final)
        return int(self._fn(self._cap_entry)(self.handle, sl.ctypes.data, ns.ctypes.data, fi.ctypes.data, sl.size))

    def _push_dev(self, slots, counts, pcm, out, out_offsets, final, cap, stream) -> None:
        sl, ns, fi = slot_arrays(slots, counts, final)
        cap = out.shape[0] if cap is None else cap
        _lib.check(self._fn("push_dev")(self.handle, sl.ctypes.data, ns.ctypes.data, fi.ctypes.data, sl.size,
                                        pcm.data_ptr() if pcm.numel() else None, out.data_ptr() if cap else None, cap,
                                        out_offsets.data_ptr(), stream or None))

    def _ragged(self, n: int, cap: int, row, call, unit: int = 1) -> List[np.ndarray]:
        """Allocates an int32 [max(cap, 1), *row] tensor and n + 1 int64 offsets (in rows of `unit` offset units), runs
        `call(out, offsets, cap, stream)` and returns the n slices as uint32 arrays."""
        import torch
        dev = f"cuda:{self.ctx.device}"
        d_out = torch.zeros((max(cap, 1), *row), dtype=torch.int32, device=dev)
        d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        call(d_out, d_oo, cap, torch.cuda.current_stream().cuda_stream)
        oo = d_oo.cpu().numpy() // unit
        out = d_out.cpu().numpy().view(np.uint32)
        return [out[oo[i]:oo[i + 1]].copy() for i in range(n)]

    def _push(self, chunks: dict, final=()) -> dict:
        import torch
        final = set(final)
        slots = list(chunks)
        arrs = [np.ascontiguousarray(chunks[s], dtype=np.float32).reshape(-1) for s in slots]
        counts = [a.size for a in arrs]
        cap = self._max_rows(slots, counts, final)
        blob = np.concatenate(arrs) if sum(counts) else np.zeros(0, np.float32)
        d_pcm = torch.from_numpy(blob).to(f"cuda:{self.ctx.device}")
        rows = self._ragged(len(slots), cap, self._row,
                            lambda out, oo, cap, st: self._push_dev(slots, counts, d_pcm, out, oo, final, cap, st))
        return dict(zip(slots, rows))


    def _windows_dev(self, slots, rows, offsets, origins, cap, stream) -> None:
        """`<_abi>_windows_dev`: the live window of slots[i] -> the bytes rows[offsets[i]:offsets[i+1]] of an int32
        [cap, *_row] tensor, `origins` an optional int32 [len(slots)] tensor; no sync."""
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        cap = rows.shape[0] if cap is None else cap
        _lib.check(self._fn("windows_dev")(self.handle, sl.ctypes.data, sl.size, rows.data_ptr() if cap else None, cap,
                                           offsets.data_ptr(), origins.data_ptr() if origins is not None else None,
                                           stream or None))

    def _windows(self, slots) -> dict:
        """{slot: (uint32 [m, *_row] rows rebased to the window's origin, origin)}, oldest row first."""
        import torch
        slots = list(slots)
        d_org = torch.zeros(max(len(slots), 1), dtype=torch.int32, device=f"cuda:{self.ctx.device}")
        rows = self._ragged(len(slots), len(slots) * self.window_cap, self._row,
                            lambda out, off, cap, st: self._windows_dev(slots, out, off, d_org, cap, st),
                            unit=4 * int(np.prod(self._row)))
        org = d_org.cpu().numpy().view(np.uint32)
        return {s: (rows[i], int(org[i])) for i, s in enumerate(slots)}
