"""kNN index -- host-side mirror of `trait IndexBackend` (src/index/mod.rs:17-78) for the vector
path, backed by the GPU-resident shard behind the C ABI (ucfp_index_*).

    GpuIndex.upsert(records)          IndexBackend::upsert   src/index/mod.rs:20-22
    GpuIndex.delete(tenant, ids)      IndexBackend::delete   :24-27
    GpuIndex.knn(tenant, query, k)    IndexBackend::knn      :29-35  (cosine over Record.embedding,
                                      as EmbeddedBackend::knn src/index/embedded/mod.rs:268-360)
    GpuIndex.hamming(tenant, h, k)    the new Hamming search behind /v1/query
    GpuIndex.identify(tenant, lm, k)  audio identification over Wang landmarks (DESIGN A10; LandmarkIndex), or with
                                      algorithm=ALGORITHM_PANAKO over Panako (hash, t_anchor) pairs (DESIGN A13)
    GpuIndex.identify_stretched(tenant, records, k)  the same over whole Panako triplets, by a (scale, offset) vote that
                                      survives a change of tempo (DESIGN A14; PanakoIndex) or, with bins="scaled",
                                      a resampled copy whose pitch moved with its speed (DESIGN A22)
    GpuIndex.identify_live(tenant, streams, slots, k)  identify / identify_stretched over the live windows of a WangStreams
                                      / PanakoStreams, windows and queries on the device (DESIGN A20)
    GpuIndex.identify_frames(tenant, frames, k)  the same over Haitsma sub-fingerprints (DESIGN A12; HaitsmaIndex)
    GpuIndex.nearest_tlsh(tenant, digest, k)  the `tlsh-128-1` records at the smallest TLSH distance (DESIGN A15; TlshIndex)
    GpuIndex.similar_images(tenant, record, k)  the image records that score highest with global and block hashes
                                      together (DESIGN A16; ImageMatchIndex)
    GpuIndex.similar_text(tenant, record_or_text, k)  the MinHash records of the same slot count that agree with a record (or a text's
                                      record) in the most slots (DESIGN A17; MinHashIndex)
    GpuIndex.bm25(tenant, terms, k)   IndexBackend::bm25 / bm25_explain :37-50 over Record.text (DESIGN A11; Bm25Index)
    GpuIndex.flush()                  IndexBackend::flush    :63

The reference keeps redb as the source of truth; this object is the device mirror of one shard
(one process per GPU).  `ShardedIndex` in ucfp_amd/sharded.py spreads a corpus over the ranks of a
node and merges per-shard top-k after an RCCL all-gather.
"""
import ctypes as C
import hashlib
from collections import OrderedDict
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import _lib
from .audio import ALGORITHM_HAITSMA, ALGORITHM_PANAKO, ALGORITHM_WANG, PanakoStreams, WangStreams, panako_landmarks
from .core import Hit, HitSource, Record, TermHit
from .errors import InvalidArgument, UnsupportedError
from .image import MultiHashConfig, match_algo
from .image import _TAG as _IMAGE_TAG
from .terms import query_terms, term_key, terms_batch, tokenize
from .text import ALGORITHM_LSH, ALGORITHM_MINHASH_128, ALGORITHM_TLSH, DEFAULT_H, MINHASH_BYTES, _check_h, minhash_slots

HAMMING64, COSINE_F32 = 1, 2
APPEND_ONLY = 1
MAX_K = 128
MAX_VIEWS = 4              # filter views a GpuIndex keeps (DESIGN F5)
INVALID_ID = 0xFFFFFFFFFFFFFFFF
BM25_LDS_POSTINGS = 6144   # UCFP_BM25_LDS_POSTINGS: a query with more postings is scored by ordinal ranges
TERM_HITS_PER_DOC = 16     # bm25.rs:503
HAITSMA_MAX_QUERY_FRAMES = 4096   # UCFP_HAITSMA_MAX_QUERY_FRAMES


class SearchBatcher:
    """Host micro-batcher for the query route (ucfp_index_search_batcher_*): request threads `submit` ONE query each (their
    own k); the library coalesces them into one search launch per flush.  /v1/query is one query per request
    (src/server/handlers.rs:143-187), up to 512 in flight (src/bin/ucfp.rs:267)."""

    def __init__(self, index: "DeviceIndex", tenant: int = 0, *, max_batch: int = 256, max_delay_us: int = 0):
        self._lib = _lib.load()
        self.index = index
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_index_search_batcher_create(index.handle, tenant, max_batch, max_delay_us, C.byref(h)))
        self.handle = h

    def submit(self, query, k: int):
        """query: int (64-bit hash) or float32 [dim].  -> (ids u64 [n], scores f32 [n], dist u32 [n]) with n <= k hits."""
        if self.index.kind == HAMMING64:
            q = np.array([query], dtype=np.uint64)
        else:
            q = np.ascontiguousarray(query, dtype=np.float32).reshape(self.index.dim)
        kk = max(int(k), 1)
        ids = np.empty(kk, np.uint64)
        sc = np.empty(kk, np.float32)
        d = np.empty(kk, np.uint32)
        cnt = C.c_uint32(0)
        _lib.check(self._lib.ucfp_index_search_batcher_submit(self.handle, q.ctypes.data, int(k), ids.ctypes.data, sc.ctypes.data,
                                                              d.ctypes.data, C.byref(cnt)))
        n = int(cnt.value)
        return ids[:n], sc[:n], d[:n]

    def stats(self):
        b, i = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.ucfp_index_search_batcher_stats(self.handle, C.byref(b), C.byref(i)))
        return int(b.value), int(i.value)

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_index_search_batcher_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiSearchBatcher(SearchBatcher):
    """The micro-batcher for the requests of MANY tenants (DESIGN M5): one per HAMMING64 index; `submit(tenant, query, k)`; one
    flush is one multi-tenant search (ucfp_index_search_multi_dev) whatever tenants its requests name."""

    def __init__(self, index: "DeviceIndex", *, max_batch: int = 256, max_delay_us: int = 0):
        self._lib = _lib.load()
        self.index = index
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_index_search_batcher_create_multi(index.handle, max_batch, max_delay_us, C.byref(h)))
        self.handle = h

    def submit(self, tenant: int, query: int, k: int):
        """query: int (64-bit hash).  -> (ids u64 [n], scores f32 [n], dist u32 [n]) with n <= k hits."""
        q = np.array([query], dtype=np.uint64)
        kk = max(int(k), 1)
        ids = np.empty(kk, np.uint64)
        sc = np.empty(kk, np.float32)
        d = np.empty(kk, np.uint32)
        cnt = C.c_uint32(0)
        _lib.check(self._lib.ucfp_index_search_batcher_submit_tenant(self.handle, int(tenant), q.ctypes.data, int(k), ids.ctypes.data,
                                                                     sc.ctypes.data, d.ctypes.data, C.byref(cnt)))
        n = int(cnt.value)
        return ids[:n], sc[:n], d[:n]


def search_multi_limits():
    """-> (rows per work item, queries per work item, tie-list capacity) of the multi-tenant search (host only)."""
    t, q, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _lib.check(_lib.load().ucfp_index_search_multi_limits(C.byref(t), C.byref(q), C.byref(c)))
    return int(t.value), int(q.value), int(c.value)


def _filter_ids(ids) -> np.ndarray:
    """Any iterable of ints in [0, 2^64), in any order, duplicates allowed -> sorted unique uint64."""
    if isinstance(ids, np.ndarray):
        if ids.dtype.kind not in "iu":
            raise InvalidArgument("filter ids must be integers")
        if ids.dtype.kind == "i" and ids.size and int(ids.min()) < 0:
            raise InvalidArgument("filter ids must lie in [0, 2^64)")
        a = ids.astype(np.uint64).reshape(-1)
    else:
        items = list(ids)
        if not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) and 0 <= int(x) < 1 << 64 for x in items):
            raise InvalidArgument("filter ids must be integers in [0, 2^64)")
        a = np.array([int(x) for x in items], dtype=np.uint64)
    return np.unique(a)


def _bitmap32_bytes(low: np.ndarray, runs: bool) -> bytes:
    """One 32-bit Roaring bitmap (DESIGN F1) over sorted unique uint32 values."""
    uk, first = np.unique(low >> np.uint32(16), return_index=True)
    n = int(uk.size)
    bounds = np.append(first, low.size)
    bodies, cards, flags = [], [], []
    for i in range(n):
        vals = (low[bounds[i]:bounds[i + 1]] & np.uint32(0xFFFF)).astype("<u2")
        card = int(vals.size)
        body, is_run = None, False
        if runs:
            brk = np.flatnonzero(np.diff(vals.astype(np.int32)) != 1)
            starts, ends = vals[np.r_[0, brk + 1]], vals[np.r_[brk, card - 1]]
            if 2 + 4 * starts.size < (2 * card if card <= 4096 else 8192):
                pairs = np.empty((starts.size, 2), "<u2")
                pairs[:, 0], pairs[:, 1] = starts, ends - starts
                body, is_run = np.array([starts.size], "<u2").tobytes() + pairs.tobytes(), True
        if body is None and card <= 4096:
            body = vals.tobytes()
        elif body is None:
            bits = np.zeros(65536, np.uint8)
            bits[vals] = 1
            body = np.packbits(bits, bitorder="little").tobytes()
        bodies.append(body)
        cards.append(card)
        flags.append(is_run)
    if any(flags):
        head = np.array([12347 | (n - 1) << 16], "<u4").tobytes() + np.packbits(np.array(flags, np.uint8), bitorder="little").tobytes()
    else:
        head = np.array([12346, n], "<u4").tobytes()
    desc = np.empty((n, 2), "<u2")
    desc[:, 0], desc[:, 1] = uk, np.array(cards, np.int64) - 1
    head += desc.tobytes()
    if not any(flags) or n >= 4:
        sizes = np.array([len(b) for b in bodies], np.int64)
        head += (len(head) + 4 * n + np.concatenate(([0], np.cumsum(sizes)[:-1]))).astype("<u4").tobytes()
    return head + b"".join(bodies)


def filter_bytes(ids, runs: bool = False) -> bytes:
    """A query filter (DESIGN F1): the portable serialization of the 64-bit Roaring treemap of `ids` -- what
    RoaringTreemap::serialize_into writes.  Containers of up to 4096 values are arrays, larger ones bitmaps; with `runs`
    a container is written as runs where that is smaller."""
    a = _filter_ids(ids)
    uh, first = np.unique(a >> np.uint64(32), return_index=True)
    bounds = np.append(first, a.size)
    out = [np.array([uh.size], "<u8").tobytes()]
    for i in range(int(uh.size)):
        out.append(np.array([uh[i]], "<u4").tobytes())
        out.append(_bitmap32_bytes((a[bounds[i]:bounds[i + 1]] & np.uint64(0xFFFFFFFF)).astype(np.uint32), runs))
    return b"".join(out)


def roaring_cardinality(data: bytes) -> int:
    """ucfp_roaring_validate: the number of ids in a filter; InvalidArgument (with the byte offset) for malformed bytes."""
    card = C.c_uint64(0)
    data = bytes(data)
    _lib.check(_lib.load().ucfp_roaring_validate(data, len(data), C.byref(card)))
    return int(card.value)


class IndexFilter:
    """A filter view (ucfp_index_filter_*, DESIGN F5): the rows of one tenant that a filter allows, as a compact sub-shard
    on the device.  Made by DeviceIndex.filter; pass it to DeviceIndex.search / search_dev."""

    def __init__(self, index: "DeviceIndex", tenant: int, data):
        self._lib = _lib.load()
        self.index, self.tenant = index, int(tenant)
        data = bytes(data) if isinstance(data, (bytes, bytearray, memoryview)) else filter_bytes(data)
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_index_filter_create(index.handle, self.tenant, data, len(data), C.byref(h)))
        self.handle = h

    def stats(self) -> dict:
        v = [C.c_size_t(0) for _ in range(4)]
        _lib.check(self._lib.ucfp_index_filter_stats(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("rows_allowed", "rows_seen", "containers", "device_bytes"), (int(x.value) for x in v)))

    def build_ms(self) -> dict:
        """Device milliseconds of the last build: probe, scan, read-back (+ allocation), gather."""
        v = [C.c_float(0) for _ in range(4)]
        _lib.check(self._lib.ucfp_index_filter_build_ms(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("probe", "scan", "readback", "gather"), (float(x.value) for x in v)))

    def check_guards(self) -> None:
        """Raises if anything wrote outside the view's own device buffers (ucfp_index_filter_check)."""
        _lib.check(self._lib.ucfp_index_filter_check(self.handle))

    @property
    def stale(self) -> bool:
        rc = self._lib.ucfp_index_filter_stale(self.handle)
        if rc < 0:
            _lib.check(rc)
        return bool(rc)

    def refresh(self) -> None:
        _lib.check(self._lib.ucfp_index_filter_refresh(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_index_filter_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceIndex:
    """Thin RAII wrapper over one ucfp_index handle (one kind, one dim)."""

    def __init__(self, kind: int, dim: int = 0, flags: int = 0, ctx=None):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.kind, self.dim, self.flags = kind, dim, flags
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_index_create(self.ctx.handle, kind, dim, flags, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- mutation ----
    def _rows(self, rows):
        if self.kind == HAMMING64:
            a = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        else:
            a = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.dim)
        return a

    def upsert(self, tenant: int, ids, rows) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        rows = self._rows(rows)
        if rows.shape[0] != ids.shape[0]:
            raise InvalidArgument("ids and rows disagree on the number of records")
        _lib.check(self._lib.ucfp_index_upsert(self.handle, tenant, ids.ctypes.data, rows.ctypes.data,
                                               ids.shape[0]))

    def save(self, path: str) -> None:
        """Snapshot every tenant's ids + rows to a flat file (the device mirror's checkpoint)."""
        _lib.check(self._lib.ucfp_index_save(self.handle, str(path).encode()))

    def load(self, path: str) -> None:
        """Upsert a snapshot written by `save` (same kind / dim)."""
        _lib.check(self._lib.ucfp_index_load(self.handle, str(path).encode()))

    def append_dev(self, tenant: int, ids_ptr: int, rows_ptr: int, n: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_index_append_dev(self.handle, tenant, ids_ptr, rows_ptr, n, stream or None))

    def delete(self, tenant: int, ids) -> int:
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        removed = C.c_size_t(0)
        _lib.check(self._lib.ucfp_index_delete(self.handle, tenant, ids.ctypes.data, ids.shape[0],
                                               C.byref(removed)))
        return int(removed.value)

    def size(self, tenant: int) -> int:
        out = C.c_size_t(0)
        _lib.check(self._lib.ucfp_index_size(self.handle, tenant, C.byref(out)))
        return int(out.value)

    def flush(self) -> None:
        _lib.check(self._lib.ucfp_index_flush(self.handle))

    # ---- search ----
    def filter(self, tenant: int, filter_bytes_or_ids) -> IndexFilter:
        """The view of `tenant` that a filter allows: bytes (DESIGN F1, e.g. `filter_bytes`) or an iterable of record ids."""
        return IndexFilter(self, tenant, filter_bytes_or_ids)

    def _view(self, tenant: int, filter) -> IndexFilter:
        if not isinstance(filter, IndexFilter):
            raise InvalidArgument("`filter` must be an IndexFilter (DeviceIndex.filter)")
        if filter.tenant != tenant:
            raise InvalidArgument(f"the filter view was made for tenant {filter.tenant}, not {tenant}")
        return filter

    def search(self, tenant: int, queries, k: int, filter: Optional[IndexFilter] = None):
        """Host-memory batch search. Returns (ids [nq,k] u64, scores [nq,k] f32, keys [nq,k] u32,
        counts [nq] u32); keys = Hamming distance, or the inverted order image of the cosine score.
        With `filter` (a view of this index and tenant) only the rows it allows answer; a stale view is refreshed."""
        q = self._rows(queries)
        nq = q.shape[0]
        kk = max(k, 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        scores = np.zeros((nq, kk), np.float32)
        keys = np.full((nq, kk), 0xFFFFFFFF, np.uint32)
        counts = np.zeros(nq, np.uint32)
        if filter is not None:
            _lib.check(self._lib.ucfp_index_search_filtered(self.handle, self._view(tenant, filter).handle, q.ctypes.data, nq, k,
                                                            ids.ctypes.data, scores.ctypes.data, keys.ctypes.data,
                                                            counts.ctypes.data))
            return ids[:, :k], scores[:, :k], keys[:, :k], counts
        _lib.check(self._lib.ucfp_index_search(self.handle, tenant, q.ctypes.data, nq, k, ids.ctypes.data,
                                               scores.ctypes.data, keys.ctypes.data, counts.ctypes.data))
        return ids[:, :k], scores[:, :k], keys[:, :k], counts

    def search_dev(self, tenant: int, queries_ptr: int, nq: int, k: int, out_ids_ptr: int,
                   out_scores_ptr: int, out_keys_ptr: int, out_counts_ptr: int, stream: int = 0,
                   filter: Optional[IndexFilter] = None) -> None:
        if filter is not None:   # (a stale view is refused here: refresh it, or search through the host entry)
            _lib.check(self._lib.ucfp_index_search_filtered_dev(self.handle, self._view(tenant, filter).handle, queries_ptr, nq, k,
                                                                out_ids_ptr, out_scores_ptr or None, out_keys_ptr or None,
                                                                out_counts_ptr, stream or None))
            return
        _lib.check(self._lib.ucfp_index_search_dev(self.handle, tenant, queries_ptr, nq, k, out_ids_ptr,
                                                   out_scores_ptr or None, out_keys_ptr or None,
                                                   out_counts_ptr, stream or None))

    def search_multi(self, tenants, queries, k: int):
        """`search` for a batch in which query i names its own tenant, tenants[i] (HAMMING64; DESIGN M1 - M6): one call and a
        number of launches that does not depend on the tenants.  Row i is what search(tenants[i], queries[i:i + 1], k) returns."""
        q = self._rows(queries)
        t = np.ascontiguousarray(tenants, dtype=np.uint32).reshape(-1)
        nq = q.shape[0]
        if t.shape[0] != nq:
            raise InvalidArgument("tenants and queries disagree on the number of queries")
        kk = max(k, 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        scores = np.zeros((nq, kk), np.float32)
        keys = np.full((nq, kk), 0xFFFFFFFF, np.uint32)
        counts = np.zeros(nq, np.uint32)
        _lib.check(self._lib.ucfp_index_search_multi(self.handle, t.ctypes.data, q.ctypes.data, nq, k, ids.ctypes.data,
                                                     scores.ctypes.data, keys.ctypes.data, counts.ctypes.data))
        return ids[:, :k], scores[:, :k], keys[:, :k], counts

    def search_multi_dev(self, tenants, queries_ptr: int, nq: int, k: int, out_ids_ptr: int, out_scores_ptr: int,
                         out_keys_ptr: int, out_counts_ptr: int, stream: int = 0) -> None:
        """`tenants`: host array of nq tenant ids (read before the call returns); everything else as `search_dev`."""
        t = None
        if tenants is not None:
            t = np.ascontiguousarray(tenants, dtype=np.uint32).reshape(-1)
            if t.shape[0] != nq:
                raise InvalidArgument("tenants and nq disagree on the number of queries")
        _lib.check(self._lib.ucfp_index_search_multi_dev(self.handle, t.ctypes.data if t is not None and nq else None, queries_ptr,
                                                         nq, k, out_ids_ptr, out_scores_ptr or None, out_keys_ptr or None,
                                                         out_counts_ptr, stream or None))


def _pack_landmarks(items):
    """Sequence of landmark sets (bytes, or uint32 [n, 2] arrays of (hash, t)) -> (u8 blob, u64 byte offsets [n + 1]).
    Bytes go through unchanged, so a length that is not a multiple of 8 reaches the library (UCFP_E_INVALID)."""
    parts = []
    for x in items:
        if isinstance(x, (bytes, bytearray, memoryview)):
            parts.append(bytes(x))
        else:
            parts.append(np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, 2).tobytes())
    offs = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(b) for b in parts], out=offs[1:])
    blob = np.frombuffer(b"".join(parts) + b"\0" * 8, np.uint8)
    return blob, offs


class LandmarkIndex:
    """Thin RAII wrapper over one ucfp_landmark_index (DESIGN A10): records and queries are sets of Wang landmarks;
    a query answers the top-k records by offset-consistent vote count, with the best offset of each."""

    def __init__(self, max_postings: int = 0, flags: int = 0, ctx=None):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.max_postings = max_postings
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_landmark_index_create(self.ctx.handle, max_postings, flags, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_landmark_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upsert(self, tenant: int, ids, landmarks) -> None:
        """ids [n]; landmarks: n landmark sets (bytes or uint32 [m, 2] of (hash, t))."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        landmarks = list(landmarks)
        if len(landmarks) != ids.shape[0]:
            raise InvalidArgument("ids and landmark sets disagree on the number of records")
        blob, offs = _pack_landmarks(landmarks)
        _lib.check(self._lib.ucfp_landmark_index_upsert(self.handle, tenant, ids.ctypes.data, blob.ctypes.data,
                                                        offs.ctypes.data, ids.shape[0]))

    def upsert_dev(self, tenant: int, ids_ptr: int, landmarks_ptr: int, offsets_ptr: int, n: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_landmark_index_upsert_dev(self.handle, tenant, ids_ptr, landmarks_ptr or None,
                                                            offsets_ptr, n, stream or None))

    def delete(self, tenant: int, ids) -> int:
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        removed = C.c_size_t(0)
        _lib.check(self._lib.ucfp_landmark_index_delete(self.handle, tenant, ids.ctypes.data, ids.shape[0],
                                                        C.byref(removed)))
        return int(removed.value)

    def size(self, tenant: int):
        """-> (records, postings) of a tenant."""
        r, p = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self._lib.ucfp_landmark_index_size(self.handle, tenant, C.byref(r), C.byref(p)))
        return int(r.value), int(p.value)

    def flush(self) -> None:
        _lib.check(self._lib.ucfp_landmark_index_flush(self.handle))

    def query(self, tenant: int, queries, k: int, min_votes: int = 1):
        """queries: landmark sets (bytes or uint32 [m, 2]).  -> (ids [nq,k] u64, votes [nq,k] u32, offsets [nq,k] i32,
        scores [nq,k] f32, counts [nq] u32)."""
        blob, offs = _pack_landmarks(list(queries))
        nq = offs.size - 1
        kk = max(int(k), 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        votes = np.zeros((nq, kk), np.uint32)
        offsets = np.zeros((nq, kk), np.int32)
        scores = np.zeros((nq, kk), np.float32)
        counts = np.zeros(nq, np.uint32)
        _lib.check(self._lib.ucfp_landmark_index_query(self.handle, tenant, blob.ctypes.data, offs.ctypes.data, nq, int(k),
                                                       int(min_votes), ids.ctypes.data, votes.ctypes.data,
                                                       offsets.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids[:, :k], votes[:, :k], offsets[:, :k], scores[:, :k], counts

    def query_dev(self, tenant: int, landmarks_ptr: int, offsets_ptr: int, nq: int, k: int, min_votes: int,
                  out_ids_ptr: int, out_votes_ptr: int, out_offsets_ptr: int, out_scores_ptr: int, out_n_ptr: int,
                  stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_landmark_index_query_dev(self.handle, tenant, landmarks_ptr or None, offsets_ptr, nq, k,
                                                           min_votes, out_ids_ptr or None, out_votes_ptr or None,
                                                           out_offsets_ptr or None, out_scores_ptr or None, out_n_ptr,
                                                           stream or None))


def _pack_triplets(items):
    """Sequence of Panako records (bytes, or uint32 [n, 4] arrays of (hash, t_a, t_b, t_c)) -> (u8 blob, u64 byte
    offsets [n + 1]).  Bytes go through unchanged, so a length that is not a multiple of 16 reaches the library
    (UCFP_E_INVALID)."""
    parts = []
    for x in items:
        if isinstance(x, (bytes, bytearray, memoryview)):
            parts.append(bytes(x))
        else:
            parts.append(np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, 4).tobytes())
    offs = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([len(b) for b in parts], out=offs[1:])
    blob = np.frombuffer(b"".join(parts) + b"\0" * 16, np.uint8)
    return blob, offs


PANAKO_MATCH_DEFAULTS = dict(scale_min=204, scale_max=320, scale_step=4, window=16, slack=2, r_slack=1)


PANAKO_BINS = {"kept": 0, "scaled": 1}
# what bins="scaled" changes in the defaults: measured on resampled tone-burst excerpts at speeds 0.85 ... 1.2
# (DESIGN A22): a 4/256 scale grid is up to 3.5 bins off at bin 440 and needs f_slack = 3 for the votes that a 2/256
# grid gets with f_slack = 1, from three times the buckets
PANAKO_SCALED_DEFAULTS = dict(scale_step=2, f_slack=1)


def panako_match_config(**match) -> "_lib.PanakoMatchConfigEx":
    """ucfp_panako_match_config_ex from keyword arguments over PANAKO_MATCH_DEFAULTS (scales in units of 1/256), plus
    bins = "kept" (the default: the vote of DESIGN A14, for time-stretched copies) or "scaled" (A22, for resampled
    copies, whose frequencies move with the speed) and f_slack (0 ... 3 bins, scaled mode only).  With bins="scaled"
    the defaults become scale_step = 2 and f_slack = 1; these were measured, not derived (PANAKO_SCALED_DEFAULTS)."""
    match = dict(match)
    bins = match.pop("bins", "kept")
    if not isinstance(bins, str) or bins not in PANAKO_BINS:
        raise InvalidArgument(f"bins is one of {sorted(PANAKO_BINS)}, not {bins!r}")
    unknown = set(match) - set(PANAKO_MATCH_DEFAULTS) - {"f_slack"}
    if unknown:
        raise InvalidArgument(f"unknown match parameters: {sorted(unknown)}")
    v = {**PANAKO_MATCH_DEFAULTS, "f_slack": 0, **(PANAKO_SCALED_DEFAULTS if bins == "scaled" else {}), **match}
    if not all(isinstance(x, (int, np.integer)) and 0 <= int(x) < 1 << 32 for x in v.values()):
        raise InvalidArgument("match parameters are integers in 0 ... 2^32 - 1")
    return _lib.PanakoMatchConfigEx(*(int(v[name]) for name in PANAKO_MATCH_DEFAULTS), PANAKO_BINS[bins], int(v["f_slack"]))


class PanakoIndex:
    """Thin RAII wrapper over one ucfp_panako_index (DESIGN A14): records and queries are Panako records; a query
    answers the top-k records by votes that agree on a (scale, offset) pair, so a time-stretched copy still matches."""

    def __init__(self, max_postings: int = 0, flags: int = 0, ctx=None):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.max_postings = max_postings
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_panako_index_create(self.ctx.handle, max_postings, flags, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_panako_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def lds_votes() -> int:
        """Expanded votes up to which a query is answered in on-chip memory."""
        return int(_lib.load().ucfp_panako_index_lds_votes())

    def upsert(self, tenant: int, ids, records) -> None:
        """ids [n]; records: n Panako records (bytes or uint32 [m, 4] of (hash, t_a, t_b, t_c))."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        records = list(records)
        if len(records) != ids.shape[0]:
            raise InvalidArgument("ids and records disagree on the number of records")
        blob, offs = _pack_triplets(records)
        _lib.check(self._lib.ucfp_panako_index_upsert(self.handle, tenant, ids.ctypes.data, blob.ctypes.data,
                                                      offs.ctypes.data, ids.shape[0]))

    def upsert_dev(self, tenant: int, ids_ptr: int, records_ptr: int, offsets_ptr: int, n: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_panako_index_upsert_dev(self.handle, tenant, ids_ptr, records_ptr or None, offsets_ptr, n,
                                                          stream or None))

    def delete(self, tenant: int, ids) -> int:
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        removed = C.c_size_t(0)
        _lib.check(self._lib.ucfp_panako_index_delete(self.handle, tenant, ids.ctypes.data, ids.shape[0], C.byref(removed)))
        return int(removed.value)

    def size(self, tenant: int):
        """-> (records, postings) of a tenant."""
        r, p = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self._lib.ucfp_panako_index_size(self.handle, tenant, C.byref(r), C.byref(p)))
        return int(r.value), int(p.value)

    def flush(self) -> None:
        _lib.check(self._lib.ucfp_panako_index_flush(self.handle))

    def query(self, tenant: int, queries, k: int, min_votes: int = 1, **match):
        """queries: Panako records (bytes or uint32 [m, 4]); match: fields of PANAKO_MATCH_DEFAULTS, bins="kept" |
        "scaled" and f_slack (panako_match_config).  -> (ids [nq,k] u64,
        votes [nq,k] u32, offsets [nq,k] i32, scales [nq,k] u32 in 1/256, scores [nq,k] f32, counts [nq] u32)."""
        cfg = panako_match_config(**match)
        blob, offs = _pack_triplets(list(queries))
        nq = offs.size - 1
        kk = max(int(k), 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        votes = np.zeros((nq, kk), np.uint32)
        offsets = np.zeros((nq, kk), np.int32)
        scales = np.zeros((nq, kk), np.uint32)
        scores = np.zeros((nq, kk), np.float32)
        counts = np.zeros(nq, np.uint32)
        _lib.check(self._lib.ucfp_panako_index_query_ex(self.handle, tenant, blob.ctypes.data, offs.ctypes.data, nq, int(k),
                                                     int(min_votes), C.byref(cfg), ids.ctypes.data, votes.ctypes.data,
                                                     offsets.ctypes.data, scales.ctypes.data, scores.ctypes.data,
                                                     counts.ctypes.data))
        return ids[:, :k], votes[:, :k], offsets[:, :k], scales[:, :k], scores[:, :k], counts

    def query_dev(self, tenant: int, records_ptr: int, offsets_ptr: int, nq: int, k: int, min_votes: int, out_ids_ptr: int,
                  out_votes_ptr: int, out_offsets_ptr: int, out_scales_ptr: int, out_scores_ptr: int, out_n_ptr: int,
                  stream: int = 0, **match) -> None:
        cfg = panako_match_config(**match)
        _lib.check(self._lib.ucfp_panako_index_query_ex_dev(self.handle, tenant, records_ptr or None, offsets_ptr, nq, k,
                                                         min_votes, C.byref(cfg), out_ids_ptr or None, out_votes_ptr or None,
                                                         out_offsets_ptr or None, out_scales_ptr or None,
                                                         out_scores_ptr or None, out_n_ptr, stream or None))


def _pack_frames(items):
    """Sequence of sub-fingerprint blocks (bytes, or uint32 [m] arrays) -> (u32 frames, u64 element offsets [n + 1])."""
    parts = []
    for x in items:
        if isinstance(x, (bytes, bytearray, memoryview)):
            if len(x) % 4:
                raise InvalidArgument("sub-fingerprint bytes must be a multiple of 4 (one u32 per frame)")
            parts.append(np.frombuffer(bytes(x), "<u4"))
        else:
            parts.append(np.ascontiguousarray(x, dtype=np.uint32).reshape(-1))
    offs = np.zeros(len(parts) + 1, np.uint64)
    np.cumsum([p.size for p in parts], out=offs[1:])
    frames = np.ascontiguousarray(np.concatenate(parts + [np.zeros(1, np.uint32)]), dtype=np.uint32)
    return frames, offs


class HaitsmaIndex:
    """Thin RAII wrapper over one ucfp_haitsma_index (DESIGN A12): records and queries are sequences of Haitsma
    sub-fingerprints; a query answers the top-k records by bit errors over the whole block at the best alignment."""

    def __init__(self, max_postings: int = 0, flags: int = 0, ctx=None):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.max_postings = max_postings
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_haitsma_index_create(self.ctx.handle, max_postings, flags, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_haitsma_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upsert(self, tenant: int, ids, frames) -> None:
        """ids [n]; frames: n blocks (bytes, 4 per frame, or uint32 [m])."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        frames = list(frames)
        if len(frames) != ids.shape[0]:
            raise InvalidArgument("ids and frame blocks disagree on the number of records")
        flat, offs = _pack_frames(frames)
        _lib.check(self._lib.ucfp_haitsma_index_upsert(self.handle, tenant, ids.ctypes.data, flat.ctypes.data,
                                                       offs.ctypes.data, ids.shape[0]))

    def upsert_dev(self, tenant: int, ids_ptr: int, frames_ptr: int, offsets_ptr: int, n: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_haitsma_index_upsert_dev(self.handle, tenant, ids_ptr, frames_ptr or None, offsets_ptr, n,
                                                           stream or None))

    def delete(self, tenant: int, ids) -> int:
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        removed = C.c_size_t(0)
        _lib.check(self._lib.ucfp_haitsma_index_delete(self.handle, tenant, ids.ctypes.data, ids.shape[0], C.byref(removed)))
        return int(removed.value)

    def size(self, tenant: int):
        """-> (records, frames) of a tenant."""
        r, f = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self._lib.ucfp_haitsma_index_size(self.handle, tenant, C.byref(r), C.byref(f)))
        return int(r.value), int(f.value)

    def flush(self) -> None:
        _lib.check(self._lib.ucfp_haitsma_index_flush(self.handle))

    def query(self, tenant: int, queries, k: int, flip_bits: int = 2, max_ber_ppm: int = 350_000):
        """queries: blocks (bytes or uint32 [m]).  -> (ids [nq,k] u64, dist [nq,k] u32, offsets [nq,k] i32,
        scores [nq,k] f32, counts [nq] u32)."""
        flat, offs = _pack_frames(list(queries))
        nq = offs.size - 1
        kk = max(int(k), 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        dist = np.full((nq, kk), 0xFFFFFFFF, np.uint32)
        offsets = np.zeros((nq, kk), np.int32)
        scores = np.full((nq, kk), -1.0, np.float32)
        counts = np.zeros(nq, np.uint32)
        _lib.check(self._lib.ucfp_haitsma_index_query(self.handle, tenant, flat.ctypes.data, offs.ctypes.data, nq, int(k),
                                                      int(flip_bits), int(max_ber_ppm), ids.ctypes.data, dist.ctypes.data,
                                                      offsets.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids[:, :k], dist[:, :k], offsets[:, :k], scores[:, :k], counts

    def query_dev(self, tenant: int, frames_ptr: int, offsets_ptr: int, nq: int, k: int, flip_bits: int, max_ber_ppm: int,
                  out_ids_ptr: int, out_dist_ptr: int, out_offsets_ptr: int, out_scores_ptr: int, out_n_ptr: int,
                  stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_haitsma_index_query_dev(self.handle, tenant, frames_ptr or None, offsets_ptr, nq, k,
                                                          flip_bits, max_ber_ppm, out_ids_ptr or None, out_dist_ptr or None,
                                                          out_offsets_ptr or None, out_scores_ptr or None, out_n_ptr,
                                                          stream or None))


def _pack_rows(rows, rec_bytes: int, to_bytes=None) -> np.ndarray:
    """A uint8 array of whole records, or a list of records, -> uint8 [n, rec_bytes] (one spare row behind it, so the
    pointer is never to an empty buffer).  A list item goes through `to_bytes`, which checks it; without one every item
    (and an array) must be rec_bytes bytes each."""
    if isinstance(rows, np.ndarray) and rows.dtype == np.uint8:
        if to_bytes is None and rows.size % rec_bytes:
            raise InvalidArgument(f"records must be {rec_bytes} bytes each")
        rows = rows.reshape(-1, rec_bytes)
    else:
        rows = [(to_bytes or bytes)(r) for r in rows]
        if to_bytes is None and any(len(r) != rec_bytes for r in rows):
            raise InvalidArgument(f"records must be {rec_bytes} bytes each")
        rows = np.frombuffer(b"".join(rows), np.uint8).reshape(-1, rec_bytes)
    buf = np.zeros((rows.shape[0] + 1, rec_bytes), np.uint8)
    buf[:rows.shape[0]] = rows
    return buf[:rows.shape[0]]


class _ScanIndex:
    """What TlshIndex, MinHashIndex and ImageMatchIndex share, as their C side does (scan_index.h): the calls
    ucfp_<_name>_index_* that do not depend on what a row is.  A subclass creates `handle` and packs rows in `_pack`."""
    _name = ""              # the C symbol prefix
    _what = "records"       # how messages call the rows

    def _call(self, fn: str, *args) -> None:
        _lib.check(getattr(self._lib, f"ucfp_{self._name}_index_{fn}")(self.handle, *args))

    def close(self):
        if getattr(self, "handle", None):
            getattr(self._lib, f"ucfp_{self._name}_index_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upsert(self, tenant: int, ids, records) -> None:
        """ids [n]; records: uint8 [n, bytes of a record], or n records as bytes."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        rows = self._pack(records)
        if rows.shape[0] != ids.shape[0]:
            raise InvalidArgument(f"ids and {self._what} disagree on the number of rows")
        self._call("upsert", tenant, ids.ctypes.data, rows.ctypes.data, ids.shape[0])

    def upsert_dev(self, tenant: int, ids_ptr: int, records_ptr: int, n: int, stream: int = 0) -> None:
        self._call("upsert_dev", tenant, ids_ptr, records_ptr, n, stream or None)

    def delete(self, tenant: int, ids) -> int:
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        removed = C.c_size_t(0)
        self._call("delete", tenant, ids.ctypes.data, ids.shape[0], C.byref(removed))
        return int(removed.value)

    def size(self, tenant: int) -> int:
        r = C.c_size_t(0)
        self._call("size", tenant, C.byref(r))
        return int(r.value)

    def flush(self) -> None:
        self._call("flush")


class TlshIndex(_ScanIndex):
    """Thin RAII wrapper over one ucfp_tlsh_index (DESIGN A15): rows and queries are TLSH digests (35 bytes each, or
    any form text.tlsh_digest_bytes takes); a query answers the k rows at the smallest TLSH distance, exactly."""
    _name, _what = "tlsh", "digests"

    def __init__(self, flags: int = 0, ctx=None):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_tlsh_index_create(self.ctx.handle, flags, C.byref(h)))
        self.handle = h

    def _pack(self, digests) -> np.ndarray:
        return _pack_digests(digests)

    def upsert(self, tenant: int, ids, digests) -> None:
        """ids [n]; digests: uint8 [n, 35], or n digests as bytes / strings."""
        super().upsert(tenant, ids, digests)

    def upsert_dev(self, tenant: int, ids_ptr: int, digests_ptr: int, n: int, stream: int = 0) -> None:
        super().upsert_dev(tenant, ids_ptr, digests_ptr, n, stream)

    def query(self, tenant: int, digests, k: int, max_distance: Optional[int] = None):
        """-> (ids [nq,k] u64, dist [nq,k] u32, scores [nq,k] f32, counts [nq] u32); rows farther than `max_distance`
        are left out (None: no cut)."""
        q = _pack_digests(digests)
        nq = q.shape[0]
        kk = max(int(k), 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        dist = np.full((nq, kk), 0xFFFFFFFF, np.uint32)
        scores = np.full((nq, kk), -1.0, np.float32)
        counts = np.zeros(nq, np.uint32)
        md = 0xFFFFFFFF if max_distance is None else int(max_distance)
        _lib.check(self._lib.ucfp_tlsh_index_query(self.handle, tenant, q.ctypes.data, nq, int(k), md, ids.ctypes.data,
                                                   dist.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids[:, :k], dist[:, :k], scores[:, :k], counts

    def query_dev(self, tenant: int, digests_ptr: int, nq: int, k: int, max_distance: int, out_ids_ptr: int,
                  out_dist_ptr: int, out_scores_ptr: int, out_n_ptr: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_tlsh_index_query_dev(self.handle, tenant, digests_ptr, nq, k, max_distance,
                                                       out_ids_ptr or None, out_dist_ptr or None, out_scores_ptr or None,
                                                       out_n_ptr, stream or None))


def _pack_digests(digests) -> np.ndarray:
    """-> uint8 [n, 35]; a single bytes or str is one digest."""
    from .text import TLSH_BYTES, tlsh_digest_bytes
    if isinstance(digests, (bytes, bytearray, str)):
        digests = [digests]
    return _pack_rows(digests, TLSH_BYTES, tlsh_digest_bytes)


class MinHashIndex(_ScanIndex):
    """Thin RAII wrapper over one ucfp_minhash_index (DESIGN A17, T10): rows and queries are MinHash records of `h`
    slots (8 + 8 h bytes each; 1032 at the default 128); a query answers the k rows that agree with it in the most slots,
    exactly, with score = agree / h."""
    _name = "minhash"

    def __init__(self, flags: int = 0, ctx=None, h: int = DEFAULT_H):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.h = _check_h(h)
        self.rec_bytes = 8 + 8 * self.h
        handle = C.c_void_p()
        _lib.check(self._lib.ucfp_minhash_index_create_h(self.ctx.handle, flags, self.h, C.byref(handle)))
        self.handle = handle

    def _pack(self, records) -> np.ndarray:
        return _pack_minhash(records, self.rec_bytes)

    def query(self, tenant: int, records, k: int, min_agree: int = 1):
        """-> (ids [nq,k] u64, agree [nq,k] u32, scores [nq,k] f32, counts [nq] u32); rows that agree in fewer than
        `min_agree` slots are left out (0: every row is a hit)."""
        if not 0 <= int(min_agree) <= self.h:
            raise InvalidArgument(f"min_agree must be in [0, {self.h}] (got {min_agree!r})")
        q = self._pack(records)
        nq = q.shape[0]
        kk = max(int(k), 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        agree = np.full((nq, kk), 0xFFFFFFFF, np.uint32)
        scores = np.full((nq, kk), -1.0, np.float32)
        counts = np.zeros(nq, np.uint32)
        _lib.check(self._lib.ucfp_minhash_index_query(self.handle, tenant, q.ctypes.data, nq, int(k), int(min_agree),
                                                      ids.ctypes.data, agree.ctypes.data, scores.ctypes.data,
                                                      counts.ctypes.data))
        return ids[:, :k], agree[:, :k], scores[:, :k], counts

    def query_dev(self, tenant: int, records_ptr: int, nq: int, k: int, min_agree: int, out_ids_ptr: int,
                  out_agree_ptr: int, out_scores_ptr: int, out_n_ptr: int, stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_minhash_index_query_dev(self.handle, tenant, records_ptr, nq, k, min_agree,
                                                          out_ids_ptr or None, out_agree_ptr or None, out_scores_ptr or None,
                                                          out_n_ptr, stream or None))


def _pack_minhash(records, rec_bytes: int = MINHASH_BYTES) -> np.ndarray:
    """-> uint8 [n, rec_bytes]; bytes are one record or several back to back."""
    if isinstance(records, (bytes, bytearray)):
        records = np.frombuffer(bytes(records), np.uint8)
    if isinstance(records, np.ndarray) and records.dtype == np.uint8 and records.ndim == 2 and records.shape[1] != rec_bytes:
        raise InvalidArgument(f"records must be {rec_bytes} bytes each")
    return _pack_rows(records, rec_bytes)


class ImageMatchIndex(_ScanIndex):
    """Thin RAII wrapper over one ucfp_image_match_index (DESIGN A16): rows and queries are whole image records of one
    size -- 168 bytes (`algo` AHASH, PHASH or DHASH) or the 536-byte bundle (MULTI); a query answers the k rows that score
    highest with global and block hashes together, exactly.  The MultiHashConfig is passed per query."""
    _name = "image_match"

    def __init__(self, algo: int, flags: int = 0, ctx=None):
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.algo = int(algo)
        self.record_bytes = int(self._lib.ucfp_image_record_bytes(self.algo))
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_image_match_index_create(self.ctx.handle, self.algo, flags, C.byref(h)))
        self.handle = h

    def _pack(self, records) -> np.ndarray:
        """-> uint8 [n, record_bytes]; bytes are exactly one record."""
        if isinstance(records, (bytes, bytearray)):
            records = [records]
        return _pack_rows(records, self.record_bytes)

    def query(self, tenant: int, records, k: int, config: Optional[MultiHashConfig] = None):
        """-> (ids [nq,k] u64, scores [nq,k] f32, counts [nq] u32); rows scoring below config.min_score are left out."""
        q = self._pack(records)
        nq = q.shape[0]
        kk = max(int(k), 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        scores = np.full((nq, kk), -1.0, np.float32)
        counts = np.zeros(nq, np.uint32)
        cfg = (config or MultiHashConfig())._c()
        _lib.check(self._lib.ucfp_image_match_index_query(self.handle, tenant, q.ctypes.data, nq, int(k), C.byref(cfg),
                                                          ids.ctypes.data, scores.ctypes.data, counts.ctypes.data))
        return ids[:, :k], scores[:, :k], counts

    def query_dev(self, tenant: int, records_ptr: int, nq: int, k: int, config: Optional[MultiHashConfig], out_ids_ptr: int,
                  out_scores_ptr: int, out_n_ptr: int, stream: int = 0) -> None:
        cfg = (config or MultiHashConfig())._c()
        _lib.check(self._lib.ucfp_image_match_index_query_dev(self.handle, tenant, records_ptr, nq, k, C.byref(cfg),
                                                              out_ids_ptr or None, out_scores_ptr or None, out_n_ptr,
                                                              stream or None))


class Bm25Index:
    """Thin RAII wrapper over one ucfp_bm25_index (DESIGN A11): BM25 over documents of (key, tf) pairs.  It keeps the
    term -> key dictionary of the index (keys number the terms in order of first sight); query terms it has never
    seen are dropped on the host.  With keys="hashed" (DESIGN A23) a term's key is its hash (terms.term_key): the device
    tokenises, hashes and counts the texts (terms.terms_batch), the dictionary stays empty, and an unseen query term is a
    key that matches nothing."""

    def __init__(self, flags: int = 0, ctx=None, keys: str = "numbered"):
        if keys not in ("numbered", "hashed"):
            raise InvalidArgument(f"unknown BM25 key mode {keys!r}: 'numbered' or 'hashed'")
        self.hashed = keys == "hashed"
        self._lib = _lib.load()
        self.ctx = ctx or _lib.current_context()
        self.keys = {}     # term -> key (numbered mode)
        h = C.c_void_p()
        _lib.check(self._lib.ucfp_bm25_index_create(self.ctx.handle, flags, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ucfp_bm25_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _key(self, term: str) -> int:
        k = self.keys.get(term)
        if k is None:
            k = self.keys[term] = len(self.keys)
        return k

    def upsert_pairs(self, tenant: int, ids, keys, tfs, offsets) -> None:
        """The ABI form: document i is (keys, tfs)[offsets[i] .. offsets[i + 1])."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
        tfs = np.ascontiguousarray(tfs, dtype=np.uint32).reshape(-1)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if offsets.size != ids.size + 1:
            raise InvalidArgument("offsets needs one entry more than ids")
        if keys.size != tfs.size:
            raise InvalidArgument("keys and tfs disagree on the number of pairs")
        _lib.check(self._lib.ucfp_bm25_index_upsert(self.handle, tenant, ids.ctypes.data, keys.ctypes.data,
                                                    tfs.ctypes.data, offsets.ctypes.data, ids.size))

    def upsert(self, tenant: int, ids, texts: Sequence[str], preprocess=None) -> None:
        """Tokenize each text (terms.tokenize) and store its term counts; a text without tokens is an empty document.
        `preprocess` (TextOpts.preprocess) is not built into this entry and is refused: strip pages first with
        text.html_to_text_batch."""
        if preprocess is not None:
            raise UnsupportedError(f"preprocess `{preprocess}` is not built into the BM25 index: strip the pages first "
                                   "(text.html_to_text_batch)")
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        texts = list(texts)
        if len(texts) != ids.size:
            raise InvalidArgument("ids and texts disagree on the number of documents")
        if self.hashed:
            keys, tfs, offs, _ = terms_batch(texts, "counts", self.ctx)
            self.upsert_pairs(tenant, ids, keys, tfs, offs)
            return
        keys, tfs, offs = [], [], [0]
        for t in texts:
            counts = {}
            for tok in tokenize(t):
                counts[tok] = counts.get(tok, 0) + 1
            keys.extend(self._key(tok) for tok in counts)
            tfs.extend(counts.values())
            offs.append(len(keys))
        self.upsert_pairs(tenant, ids, np.array(keys, np.uint64), np.array(tfs, np.uint32), np.array(offs, np.uint64))

    def upsert_dev(self, tenant: int, ids_ptr: int, keys_ptr: int, tfs_ptr: int, offsets_ptr: int, n: int,
                   stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_bm25_index_upsert_dev(self.handle, tenant, ids_ptr, keys_ptr or None, tfs_ptr or None,
                                                        offsets_ptr, n, stream or None))

    def delete(self, tenant: int, ids) -> int:
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        removed = C.c_size_t(0)
        _lib.check(self._lib.ucfp_bm25_index_delete(self.handle, tenant, ids.ctypes.data, ids.shape[0], C.byref(removed)))
        return int(removed.value)

    def size(self, tenant: int):
        """-> (documents, postings) of a tenant."""
        d, p = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self._lib.ucfp_bm25_index_size(self.handle, tenant, C.byref(d), C.byref(p)))
        return int(d.value), int(p.value)

    def flush(self) -> None:
        _lib.check(self._lib.ucfp_bm25_index_flush(self.handle))

    def query_keys(self, tenant: int, queries, k: int, explain: bool = False):
        """queries: key lists.  -> (ids [nq,k] u64, scores [nq,k] f32, counts [nq] u32) and, with explain, (idf [total] f32,
        tf [total * k] u32, contributions [total * k] f32) laid out as ucfp_hip.h says."""
        qs = [np.ascontiguousarray(q, dtype=np.uint64).reshape(-1) for q in queries]
        offs = np.zeros(len(qs) + 1, np.uint64)
        np.cumsum([q.size for q in qs], out=offs[1:])
        keys = np.concatenate(qs + [np.zeros(1, np.uint64)])
        nq, total, kk = len(qs), int(offs[-1]), max(int(k), 1)
        ids = np.full((nq, kk), INVALID_ID, np.uint64)
        scores = np.zeros((nq, kk), np.float32)
        counts = np.zeros(nq, np.uint32)
        idf = np.zeros(max(total, 1), np.float32)
        tf = np.zeros(max(total * kk, 1), np.uint32)
        con = np.zeros(max(total * kk, 1), np.float32)
        x = (idf.ctypes.data, tf.ctypes.data, con.ctypes.data) if explain else (None, None, None)
        _lib.check(self._lib.ucfp_bm25_index_query(self.handle, tenant, keys.ctypes.data, offs.ctypes.data, nq, int(k),
                                                   ids.ctypes.data, scores.ctypes.data, counts.ctypes.data, *x))
        out = (ids[:, :k], scores[:, :k], counts)
        return out + (idf[:total], tf[:total * k], con[:total * k]) if explain else out

    def query_dev(self, tenant: int, keys_ptr: int, offsets_ptr: int, nq: int, k: int, out_ids_ptr: int,
                  out_scores_ptr: int, out_n_ptr: int, out_idf_ptr: int = 0, out_tf_ptr: int = 0, out_contrib_ptr: int = 0,
                  stream: int = 0) -> None:
        _lib.check(self._lib.ucfp_bm25_index_query_dev(self.handle, tenant, keys_ptr or None, offsets_ptr, nq, k,
                                                       out_ids_ptr or None, out_scores_ptr or None, out_n_ptr,
                                                       out_idf_ptr or None, out_tf_ptr or None, out_contrib_ptr or None,
                                                       stream or None))

    def search(self, tenant: int, terms: Sequence[str], k: int, explain: bool = False) -> List[Hit]:
        """bm25.rs `search_explain`: the query terms are re-tokenized and flattened; each hit explains at most 16
        matched positions, sorted stably by contribution, descending."""
        toks = query_terms(terms)
        if not self.hashed:
            toks = [t for t in toks if t in self.keys]
        if k == 0 or not toks:
            return []
        k = min(k, MAX_K)
        res = self.query_keys(tenant, [[term_key(t) if self.hashed else self.keys[t] for t in toks]], k, explain)
        return self._hits(tenant, res, 0, 0, toks, k, explain)

    def _hits(self, tenant: int, res, q: int, base: int, toks, k: int, explain: bool) -> List[Hit]:
        """The hits of query q of a query_keys result; its m = len(toks) positions begin at `base` of the explain arrays."""
        ids, scores, counts = res[:3]
        hits = []
        m = len(toks)
        for h in range(int(counts[q])):
            th = []
            if explain:
                idf, tf, con = res[3:]
                o = k * base + h * m
                th = [TermHit(term=toks[j], idf=float(idf[base + j]), tf=int(tf[o + j]), contribution=float(con[o + j]))
                      for j in range(m) if tf[o + j]]
                th = sorted(th, key=lambda t: t.contribution, reverse=True)[:TERM_HITS_PER_DOC]
            hits.append(Hit(tenant_id=tenant, record_id=int(ids[q, h]), score=float(scores[q, h]), source=HitSource.Bm25,
                            term_hits=th))
        return hits

    def search_texts(self, tenant: int, texts: Sequence[str], k: int, explain: bool = False) -> List[List[Hit]]:
        """A batch of query strings (hashed mode): the device tokenises and hashes them (the SEQUENCE form of
        terms.terms_batch), one query_keys call scores them.  -> one hit list per text, each what
        search(tenant, [text], k, explain) returns."""
        if not self.hashed:
            raise InvalidArgument("search_texts needs keys='hashed'")
        texts = list(texts)
        if k == 0 or not texts:
            return [[] for _ in texts]
        k = min(k, MAX_K)
        keys, _, offs, _ = terms_batch(texts, "sequence", self.ctx)
        res = self.query_keys(tenant, [keys[int(offs[i]):int(offs[i + 1])] for i in range(len(texts))], k, explain)
        out = []
        for i, t in enumerate(texts):
            toks = tokenize(t) if explain else [None] * int(offs[i + 1] - offs[i])
            out.append(self._hits(tenant, res, i, int(offs[i]), toks, k, explain))
        return out


def topk_merge_dev(kind: int, part_ids_ptr: int, part_keys_ptr: int, parts: int, nq: int, k: int,
                   out_ids_ptr: int, out_scores_ptr: int, out_keys_ptr: int, out_counts_ptr: int,
                   stream: int = 0, ctx=None) -> None:
    ctx = ctx or _lib.current_context()
    _lib.check(_lib.load().ucfp_topk_merge_dev(ctx.handle, kind, part_ids_ptr, part_keys_ptr, parts, nq, k,
                                               out_ids_ptr, out_scores_ptr or None, out_keys_ptr,
                                               out_counts_ptr, stream or None))


class GpuIndex:
    """IndexBackend-shaped facade: cosine kNN over `Record.embedding` plus Hamming search over
    64-bit hashes pulled out of `Record.fingerprint`.  Embedding indexes are keyed by dimension,
    like the reference skips rows whose stored length differs from the query's
    (src/index/embedded/mod.rs:307-309)."""

    def __init__(self, ctx=None, sidecar=None, bm25_keys: str = "numbered"):
        if bm25_keys not in ("numbered", "hashed"):
            raise InvalidArgument(f"unknown BM25 key mode {bm25_keys!r}: 'numbered' or 'hashed'")
        self._bm25_keys = bm25_keys   # how the Bm25Index keys its terms (DESIGN A23)
        self.ctx = ctx or _lib.current_context()
        self._cos = {}        # dim -> DeviceIndex
        self._ham = {}        # hash space name -> DeviceIndex
        self._lm = None       # LandmarkIndex of the audiofp-wang-v1 records (DESIGN A10)
        self._pk = None       # LandmarkIndex of the audiofp-panako-v1 records' (hash, t_anchor) pairs (DESIGN A13)
        self._ps = None       # PanakoIndex of the same records' triples: the (scale, offset) vote (DESIGN A14)
        self._hx = None       # HaitsmaIndex of the audiofp-haitsma-v1 records (DESIGN A12)
        self._bm = None       # Bm25Index of the records with text (DESIGN A11)
        self._tl = None       # TlshIndex of the tlsh-128-1 records (DESIGN A15)
        self._im = {}         # image algorithm tag -> ImageMatchIndex of its whole records (DESIGN A16)
        self._mh = {}         # MinHash algorithm tag -> MinHashIndex of its 1032-byte records (DESIGN A17)
        self._mh_h = {}       # (tag, H) -> MinHashIndex of the tag's records of H != 128 slots (DESIGN T10): one index per (tag, H)
        self._sidecar = sidecar   # ucfp_amd.store.Sidecar: the stored-table mirror written at upsert
        self._views = OrderedDict()   # (id of the DeviceIndex, tenant, digest of the filter bytes) -> IndexFilter, at most MAX_VIEWS

    def _view(self, ix: DeviceIndex, tenant_id: int, filter) -> IndexFilter:
        """The cached view of a query's filter bytes (DESIGN F5): least recently used out at MAX_VIEWS; a stale one is
        refreshed by the search itself."""
        if not isinstance(filter, (bytes, bytearray, memoryview)):
            raise InvalidArgument("`filter` must be bytes (a serialized Roaring treemap: index.filter_bytes)")
        data = bytes(filter)
        key = (id(ix), int(tenant_id), hashlib.blake2b(data, digest_size=16).digest())
        view = self._views.get(key)
        if view is None:
            view = self._views[key] = ix.filter(tenant_id, data)
            while len(self._views) > MAX_VIEWS:
                self._views.popitem(last=False)[1].close()
        else:
            self._views.move_to_end(key)
        return view

    def attach_sidecar(self, sidecar) -> None:
        self._sidecar = sidecar

    def _cosine(self, dim: int) -> DeviceIndex:
        ix = self._cos.get(dim)
        if ix is None:
            ix = self._cos[dim] = DeviceIndex(COSINE_F32, dim, 0, self.ctx)
        return ix

    def _hamming(self, space: str) -> DeviceIndex:
        ix = self._ham.get(space)
        if ix is None:
            ix = self._ham[space] = DeviceIndex(HAMMING64, 0, 0, self.ctx)
        return ix

    def _landmarks(self) -> LandmarkIndex:
        if self._lm is None:
            self._lm = LandmarkIndex(0, 0, self.ctx)
        return self._lm

    def _panako(self) -> LandmarkIndex:
        if self._pk is None:
            self._pk = LandmarkIndex(0, 0, self.ctx)
        return self._pk

    def _panako_stretch(self) -> PanakoIndex:
        if self._ps is None:
            self._ps = PanakoIndex(0, 0, self.ctx)
        return self._ps

    def _haitsma(self) -> HaitsmaIndex:
        if self._hx is None:
            self._hx = HaitsmaIndex(0, 0, self.ctx)
        return self._hx

    def _tlsh(self) -> TlshIndex:
        if self._tl is None:
            self._tl = TlshIndex(0, self.ctx)
        return self._tl

    def _image_match(self, tag: str) -> ImageMatchIndex:
        ix = self._im.get(tag)
        if ix is None:
            ix = self._im[tag] = ImageMatchIndex(_IMAGE_ALGO[tag], 0, self.ctx)
        return ix

    def _minhash(self, tag: str, h: int = DEFAULT_H) -> MinHashIndex:
        """The MinHash index of (tag, H), made on first use: every H carries the tag `minhash-h128`, so H is part of the key."""
        table, key = (self._mh, tag) if h == DEFAULT_H else (self._mh_h, (tag, h))
        ix = table.get(key)
        if ix is None:
            ix = table[key] = MinHashIndex(0, self.ctx, h)
        return ix

    def _minhash_get(self, tag: str, h: int) -> Optional[MinHashIndex]:
        return self._mh.get(tag) if h == DEFAULT_H else self._mh_h.get((tag, h))

    def _minhash_keys(self):
        """(tag, H) of every MinHash index present."""
        return [(tag, DEFAULT_H) for tag in self._mh] + list(self._mh_h)

    def _bm25(self) -> Bm25Index:
        if self._bm is None:
            self._bm = Bm25Index(0, self.ctx, self._bm25_keys)
        return self._bm

    def _all(self):
        return (list(self._cos.values()) + list(self._ham.values()) + ([self._lm] if self._lm is not None else [])
                + ([self._pk] if self._pk is not None else [])
                + ([self._ps] if self._ps is not None else [])
                + ([self._hx] if self._hx is not None else [])
                + ([self._bm] if self._bm is not None else [])
                + ([self._tl] if self._tl is not None else []) + list(self._im.values()) + list(self._mh.values())
                + list(self._mh_h.values()))

    def upsert(self, records: Sequence[Record]) -> None:
        """Embeddings go to the cosine index of their dimension; image records also feed the
        Hamming spaces `<algorithm>` with their 64-bit global hashes (SURVEY 8f N2 offsets) and, whole, the image match
        index of their algorithm tag (DESIGN A16); `minhash-h128` and `minhash-lsh-h128` records of 8 + 8 H bytes feed the
        MinHash index of their tag and slot count H, told by the fingerprint's length (DESIGN A17, T10: the two tags carry
        the same bytes and mean different things to the index layer, so they are never searched together; records of
        different H cannot be compared);
        `audiofp-wang-v1` records feed the landmark index with their landmarks, `audiofp-panako-v1` records a second
        landmark index with their (hash, t_anchor) pairs (the two never share postings) and `audiofp-haitsma-v1` records
        the sub-fingerprint index with their frames; every record with `text`, whatever its
        modality, feeds BM25, and a record without text leaves it (src/index/embedded/mod.rs:208-219).

        Overwrite semantics are the reference's: everything is keyed by (tenant_id, record_id), a re-ingested record
        REPLACES the old one -- "Drop any stale vector for this key" when the new record has no embedding
        (src/index/embedded/mod.rs:184-191), a new dimension or algorithm replaces the old row.  So before inserting,
        the key is removed from every cosine index of another dimension, every hash space, both landmark indexes, the sub-fingerprint index
        and the image match and MinHash indexes when the new record does not feed them.  Within one batch the last record of a key wins, as successive `insert`s in one redb transaction do."""
        if self._sidecar is not None:     # the log first (the host does this right after its redb commit), then the mirror
            self._sidecar.append(records)
        last = {}
        for r in records:
            last[(r.tenant_id, r.record_id)] = r
        by_cos, by_ham, stale_cos, stale_ham, by_lm, stale_lm, by_bm, stale_bm = {}, {}, {}, {}, {}, {}, {}, {}
        by_hx, stale_hx, by_pk, stale_pk, by_tl, stale_tl = {}, {}, {}, {}, {}, {}
        by_im, stale_im, by_mh, stale_mh = {}, {}, {}, {}
        for r in last.values():
            if r.text is not None:
                by_bm.setdefault(r.tenant_id, []).append(r)
            elif self._bm is not None:
                stale_bm.setdefault(r.tenant_id, []).append(r.record_id)
            if r.algorithm == ALGORITHM_WANG:
                by_lm.setdefault(r.tenant_id, []).append(r)
            elif self._lm is not None:
                stale_lm.setdefault(r.tenant_id, []).append(r.record_id)
            if r.algorithm == ALGORITHM_PANAKO:
                by_pk.setdefault(r.tenant_id, []).append(r)
            elif self._pk is not None:
                stale_pk.setdefault(r.tenant_id, []).append(r.record_id)
            if r.algorithm == ALGORITHM_HAITSMA:
                by_hx.setdefault(r.tenant_id, []).append(r)
            elif self._hx is not None:
                stale_hx.setdefault(r.tenant_id, []).append(r.record_id)
            if r.algorithm == ALGORITHM_TLSH:
                by_tl.setdefault(r.tenant_id, []).append(r)
            elif self._tl is not None:
                stale_tl.setdefault(r.tenant_id, []).append(r.record_id)
            im_tag = r.algorithm if _feeds_image_match(r) else None
            if im_tag is not None:
                by_im.setdefault((r.tenant_id, im_tag), []).append(r)
            for tag in self._im:
                if tag != im_tag:
                    stale_im.setdefault((r.tenant_id, tag), []).append(r.record_id)
            mh_key = (r.algorithm, minhash_slots(r.fingerprint)) if _feeds_minhash(r) else None
            if mh_key is not None:
                by_mh.setdefault((r.tenant_id, mh_key), []).append(r)
            for key in self._minhash_keys():
                if key != mh_key:
                    stale_mh.setdefault((r.tenant_id, key), []).append(r.record_id)
            dim = len(r.embedding) if r.embedding is not None else 0
            if dim > 0:
                by_cos.setdefault((r.tenant_id, dim), []).append(r)
            for d in self._cos:
                if d != dim:
                    stale_cos.setdefault((r.tenant_id, d), []).append(r.record_id)
            fed = set()
            for space, h in _hash_spaces(r):
                by_ham.setdefault((r.tenant_id, space), []).append((r.record_id, h))
                fed.add(space)
            for space in self._ham:
                if space not in fed:
                    stale_ham.setdefault((r.tenant_id, space), []).append(r.record_id)
        for (tenant, d), ids in stale_cos.items():
            self._cos[d].delete(tenant, np.array(ids, np.uint64))
        for (tenant, space), ids in stale_ham.items():
            self._ham[space].delete(tenant, np.array(ids, np.uint64))
        for tenant, ids in stale_lm.items():
            self._lm.delete(tenant, np.array(ids, np.uint64))
        for tenant, ids in stale_pk.items():
            self._pk.delete(tenant, np.array(ids, np.uint64))
            self._ps.delete(tenant, np.array(ids, np.uint64))
        for tenant, ids in stale_hx.items():
            self._hx.delete(tenant, np.array(ids, np.uint64))
        for tenant, ids in stale_tl.items():
            self._tl.delete(tenant, np.array(ids, np.uint64))
        for (tenant, tag), ids in stale_im.items():
            self._im[tag].delete(tenant, np.array(ids, np.uint64))
        for (tenant, (tag, h)), ids in stale_mh.items():
            self._minhash_get(tag, h).delete(tenant, np.array(ids, np.uint64))
        for tenant, ids in stale_bm.items():
            self._bm.delete(tenant, np.array(ids, np.uint64))
        for tenant, recs in by_bm.items():
            self._bm25().upsert(tenant, np.array([r.record_id for r in recs], np.uint64), [r.text for r in recs])
        for tenant, recs in by_lm.items():
            self._landmarks().upsert(tenant, np.array([r.record_id for r in recs], np.uint64),
                                     [bytes(r.fingerprint) for r in recs])
        for tenant, recs in by_pk.items():
            self._panako().upsert(tenant, np.array([r.record_id for r in recs], np.uint64),
                                  [panako_landmarks(bytes(r.fingerprint)) for r in recs])
            self._panako_stretch().upsert(tenant, np.array([r.record_id for r in recs], np.uint64),
                                          [bytes(r.fingerprint) for r in recs])
        for tenant, recs in by_hx.items():
            self._haitsma().upsert(tenant, np.array([r.record_id for r in recs], np.uint64),
                                   [bytes(r.fingerprint) for r in recs])
        for tenant, recs in by_tl.items():
            self._tlsh().upsert(tenant, np.array([r.record_id for r in recs], np.uint64),
                                [bytes(r.fingerprint) for r in recs])
        for (tenant, tag), recs in by_im.items():
            self._image_match(tag).upsert(tenant, np.array([r.record_id for r in recs], np.uint64),
                                          [bytes(r.fingerprint) for r in recs])
        for (tenant, (tag, h)), recs in by_mh.items():
            self._minhash(tag, h).upsert(tenant, np.array([r.record_id for r in recs], np.uint64),
                                      [bytes(r.fingerprint) for r in recs])
        for (tenant, dim), recs in by_cos.items():
            ids = np.array([r.record_id for r in recs], np.uint64)
            rows = np.array([r.embedding for r in recs], np.float32)
            self._cosine(dim).upsert(tenant, ids, rows)
        for (tenant, space), items in by_ham.items():
            ids = np.array([i for i, _ in items], np.uint64)
            rows = np.array([h for _, h in items], np.uint64)
            self._hamming(space).upsert(tenant, ids, rows)

    def delete(self, tenant_id: int, record_ids: Iterable[int]) -> None:
        ids = np.array(list(record_ids), np.uint64)
        if self._sidecar is not None:
            self._sidecar.delete(tenant_id, ids.tolist())
        for ix in self._all():
            ix.delete(tenant_id, ids)

    def knn(self, tenant_id: int, query: Sequence[float], k: int, _filter: Optional[bytes] = None) -> List[Hit]:
        """EmbeddedBackend::knn: empty query or k == 0 -> [] (src/index/embedded/mod.rs:275-277)."""
        q = np.asarray(query, np.float32).reshape(-1)
        if q.size == 0 or k == 0:
            return []
        ix = self._cos.get(q.size)
        if ix is None:
            return []
        view = self._view(ix, tenant_id, _filter) if _filter is not None else None
        ids, scores, _, counts = ix.search(tenant_id, q[None, :], min(k, MAX_K), view)
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]),
                    source=HitSource.Vector) for i in range(int(counts[0]))]

    def hamming(self, tenant_id: int, space: str, query_hash: int, k: int, filter: Optional[bytes] = None) -> List[Hit]:
        if k == 0 or space not in self._ham:
            return []
        ix = self._ham[space]
        view = self._view(ix, tenant_id, filter) if filter is not None else None
        ids, scores, dist, counts = ix.search(
            tenant_id, np.array([query_hash], np.uint64), min(k, MAX_K), view)
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]),
                    source=HitSource.Hamming, distance=int(dist[0, i])) for i in range(int(counts[0]))]

    def hamming_many(self, space: str, requests, k: int) -> List[List[Hit]]:
        """[hamming(t, space, h, k) for t, h in requests] through ONE multi-tenant search (DESIGN M6): `requests` is an
        iterable of (tenant_id, query_hash)."""
        reqs = [(int(t), int(h)) for t, h in requests]
        if k == 0 or space not in self._ham or not reqs:
            return [[] for _ in reqs]
        ids, scores, dist, counts = self._ham[space].search_multi(
            np.array([t for t, _ in reqs], np.uint32), np.array([h for _, h in reqs], np.uint64), min(k, MAX_K))
        return [[Hit(tenant_id=t, record_id=int(ids[q, i]), score=float(scores[q, i]), source=HitSource.Hamming,
                     distance=int(dist[q, i])) for i in range(int(counts[q]))] for q, (t, _) in enumerate(reqs)]

    def identify(self, tenant_id: int, landmarks, k: int, min_votes: int = 1, algorithm: str = ALGORITHM_WANG) -> List[Hit]:
        """Which recording is this clip, and where in it: landmarks = bytes (8 per landmark) or uint32 [n, 2] of
        (hash, t).  Hits by offset-consistent votes (DESIGN A10); `offset` = the clip's frame 0 in the record.
        `algorithm` picks the index: Wang landmarks, or the (hash, t_anchor) pairs of Panako records
        (audio.panako_landmarks, DESIGN A13)."""
        if algorithm not in (ALGORITHM_WANG, ALGORITHM_PANAKO):
            raise InvalidArgument(f"no landmark index for algorithm {algorithm!r}")
        ix = self._pk if algorithm == ALGORITHM_PANAKO else self._lm
        if k == 0 or ix is None:
            return []
        ids, votes, offs, scores, counts = ix.query(tenant_id, [landmarks], min(k, MAX_K), min_votes)
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]), source=HitSource.Landmark,
                    votes=int(votes[0, i]), offset=int(offs[0, i])) for i in range(int(counts[0]))]

    def identify_stretched(self, tenant_id: int, records, k: int, min_votes: int = 1, **match) -> List[Hit]:
        """Which recording is this clip, where in it and at what tempo: records = Panako records as bytes (16 per
        triplet) or uint32 [n, 4] of (hash, t_a, t_b, t_c).  Hits by votes that agree on a scale and an offset window
        (DESIGN A14; `match` overrides PANAKO_MATCH_DEFAULTS): `offset` = the clip's frame 0 in the record, `scale` =
        the record's frames per frame of the clip.  bins="scaled" in `match` (DESIGN A22, panako_match_config) finds a
        resampled copy, whose frequencies moved with its speed, instead of a time-stretched one; a caller who does not
        know which change a copy went through asks both ways."""
        if self._ps is None:
            panako_match_config(**match)
            return []
        ids, votes, offs, scales, scores, counts = self._ps.query(tenant_id, [records], min(k, MAX_K), min_votes, **match)
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]), source=HitSource.Landmark,
                    votes=int(votes[0, i]), offset=int(offs[0, i]), scale=int(scales[0, i]) / 256.0)
                for i in range(int(counts[0]))]

    def identify_live(self, tenant_id: int, streams, slots, k: int, min_votes: int = 1, **match) -> dict:
        """What are these live streams playing right now: {slot: (hits, origin)} for open `slots` of a `WangStreams` or a
        `PanakoStreams` created with window_frames > 0 (DESIGN A20).  The windows go from the set to the index on the
        device (`windows_dev` -> `LandmarkIndex.query_dev` / `PanakoIndex.query_dev`, one stream); only the answers
        come back.  The hits of a slot are those of `identify` (Wang) / `identify_stretched` (Panako, with `match`) on
        the host copy of its window, [] for an empty window; `offset` = frame `origin` of the stream in the record.
        bins="scaled" in `match` finds a feed that runs fast or slow (DESIGN A22), still without a host trip.  A
        set that resamples its feed (`resample=True`, DESIGN A21) needs nothing else: its windows and origins are in
        8 kHz frames like any other's.  A set without windows raises InvalidArgument.  Haitsma sets are left out on
        purpose: `blocks_dev` reports no origin, so a hit's offset could not be placed in the stream."""
        import torch
        if isinstance(streams, WangStreams):
            if match:
                raise InvalidArgument(f"unknown match parameters: {sorted(match)}")
            ix, width = self._lm, 2
        elif isinstance(streams, PanakoStreams):
            panako_match_config(**match)
            ix, width = self._ps, 4
        else:
            raise InvalidArgument("identify_live takes a WangStreams or a PanakoStreams")
        slots = [int(s) for s in slots]
        nq, kk = len(slots), min(int(k), MAX_K)
        dev = f"cuda:{streams.ctx.device}"
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream().cuda_stream
            d_win = torch.zeros((max(nq * streams.window_cap, 1), width), dtype=torch.int32, device=dev)
            d_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            d_org = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
            streams.windows_dev(slots, d_win, d_off, d_org, nq * streams.window_cap, st)
            answered = bool(nq and kk and ix is not None)
            if answered:
                o_ids = torch.zeros((nq, kk), dtype=torch.int64, device=dev)
                o_v, o_o, o_c = (torch.zeros((nq, kk), dtype=torch.int32, device=dev) for _ in range(3))
                o_f = torch.zeros((nq, kk), dtype=torch.float32, device=dev)
                o_n = torch.zeros(nq, dtype=torch.int32, device=dev)
                scales = (o_c.data_ptr(),) if width == 4 else ()
                ix.query_dev(tenant_id, d_win.data_ptr(), d_off.data_ptr(), nq, kk, min_votes, o_ids.data_ptr(),
                             o_v.data_ptr(), o_o.data_ptr(), *scales, o_f.data_ptr(), o_n.data_ptr(), st, **match)
                ids, votes, offs = o_ids.cpu().numpy().view(np.uint64), o_v.cpu().numpy(), o_o.cpu().numpy()
                sc, scores, counts = o_c.cpu().numpy(), o_f.cpu().numpy(), o_n.cpu().numpy()
            org = d_org.cpu().numpy().view(np.uint32)
        out = {}
        for q, s in enumerate(slots):
            out[s] = ([Hit(tenant_id=tenant_id, record_id=int(ids[q, i]), score=float(scores[q, i]),
                           source=HitSource.Landmark, votes=int(votes[q, i]), offset=int(offs[q, i]),
                           scale=int(sc[q, i]) / 256.0 if width == 4 else None)
                       for i in range(int(counts[q]) if answered else 0)], int(org[q]))
        return out

    def identify_frames(self, tenant_id: int, frames, k: int, flip_bits: int = 2, max_ber: float = 0.35) -> List[Hit]:
        """Which recording is this clip, and where in it: frames = Haitsma sub-fingerprints as bytes (4 per frame) or
        uint32 [m], m <= HAITSMA_MAX_QUERY_FRAMES.  Hits by bit errors over the whole block at the best alignment found
        within `flip_bits` of some frame, under the bit-error rate `max_ber` (DESIGN A12); `distance` = the bit errors,
        `offset` = the clip's frame 0 in the record."""
        if k == 0 or self._hx is None:
            return []
        ids, dist, offs, scores, counts = self._hx.query(tenant_id, [frames], min(k, MAX_K), flip_bits,
                                                         int(round(max_ber * 1_000_000)))
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]), source=HitSource.Haitsma,
                    distance=int(dist[0, i]), offset=int(offs[0, i])) for i in range(int(counts[0]))]

    def nearest_tlsh(self, tenant_id: int, digest, k: int, max_distance: Optional[int] = None) -> List[Hit]:
        """The `tlsh-128-1` records nearest to a digest (35 bytes, or the digest string a record stores): hits by TLSH
        distance, nearest first (DESIGN A15); `distance` = the TLSH distance, score = (2473 - distance) / 2473."""
        if k == 0 or self._tl is None:
            return []
        ids, dist, scores, counts = self._tl.query(tenant_id, [digest], min(k, MAX_K), max_distance)
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]), source=HitSource.Tlsh,
                    distance=int(dist[0, i])) for i in range(int(counts[0]))]

    def similar_images(self, tenant_id: int, record_bytes, k: int, algorithm: Optional[str] = None,
                       config: Optional[MultiHashConfig] = None) -> List[Hit]:
        """The image records most similar to a whole record (168 bytes, or the 536-byte bundle), global and block hashes
        scored together under `config` (DESIGN A16): a copy with a local edit -- a caption, a logo, an occluded corner --
        keeps most of its block hashes and is still found.  `algorithm` names the tag of the records searched: it must
        match the length; with none, a bundle searches the bundles and a 168-byte record the only single-algorithm
        index present."""
        rec = bytes(record_bytes)
        algo = match_algo(len(rec), algorithm)
        tag = algorithm
        if tag is None:
            if len(rec) == 536:
                tag = _IMAGE_TAG[algo]
            else:
                present = [t for t in self._im if t != _IMAGE_TAG[7]]
                if len(present) > 1:
                    raise InvalidArgument("`algorithm` is required when 168-byte records of several algorithms are indexed")
                tag = present[0] if present else None
        cfg = config or MultiHashConfig()
        ix = self._im.get(tag)
        if ix is None or k == 0:
            cfg_c = cfg._c()      # an invalid config is refused whether or not anything is indexed
            _lib.check(_lib.load().ucfp_image_match_score(rec, rec, algo, C.byref(cfg_c), C.byref(C.c_float(0.0))))
            return []
        ids, scores, counts = ix.query(tenant_id, [rec], min(k, MAX_K), cfg)
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]), source=HitSource.ImageMatch)
                for i in range(int(counts[0]))]

    def similar_text(self, tenant_id: int, record_or_text, k: int, *, algorithm: Optional[str] = None,
                     min_agree: Optional[int] = None, threshold: Optional[float] = None) -> List[Hit]:
        """The MinHash records that agree with a record in the most slots (DESIGN A17): `record_or_text` is the 8 + 8 H
        record bytes, or a `str` that is fingerprinted with the default TextOpts first.  The record's length tells H, and
        only stored records of that H are searched (none stored: no hits).  Hits need `min_agree` equal slots
        (default 1), or the Jaccard estimate `threshold` (text.min_agree_for); score = agree / H, `distance` =
        H - agree.  `algorithm` names the tag of the records searched (`minhash-h128` or `minhash-lsh-h128`); with
        none, the only tag with a MinHash index."""
        if min_agree is not None and threshold is not None:
            raise InvalidArgument("give `min_agree` or `threshold`, not both")
        if algorithm is not None and algorithm not in _MINHASH_TAGS:
            raise InvalidArgument(f"no MinHash index for algorithm {algorithm!r}")
        if isinstance(record_or_text, str):
            from .text import TextOpts, minhash_batch, _raise_for
            recs, status = minhash_batch([record_or_text], TextOpts())
            _raise_for(int(status[0]))
            rec = recs[0].tobytes()
        else:
            rec = bytes(record_or_text)
        h = minhash_slots(rec)
        if threshold is not None:
            from .text import min_agree_for
            min_agree = min_agree_for(threshold, h)
        elif min_agree is None:
            min_agree = 1
        if not 0 <= int(min_agree) <= h:
            raise InvalidArgument(f"min_agree must be in [0, {h}] (got {min_agree!r})")
        tag = algorithm
        if tag is None:
            tags = {t for t, _ in self._minhash_keys()}
            if len(tags) > 1:
                raise InvalidArgument("`algorithm` is required when MinHash records of several algorithms are indexed")
            tag = next(iter(tags), None)
        ix = self._minhash_get(tag, h)
        if ix is None or k == 0:
            return []
        ids, agree, scores, counts = ix.query(tenant_id, [rec], min(k, MAX_K), int(min_agree))
        return [Hit(tenant_id=tenant_id, record_id=int(ids[0, i]), score=float(scores[0, i]), source=HitSource.MinHash,
                    distance=h - int(agree[0, i])) for i in range(int(counts[0]))]

    def bm25(self, tenant_id: int, terms: Sequence[str], k: int, filter: Optional[bytes] = None,
             explain: bool = False) -> List[Hit]:
        """IndexBackend::bm25 / bm25_explain (src/index/embedded/mod.rs:127-150): "bm25" hits by BM25 score (DESIGN
        A11); with `explain`, each hit's term_hits.  A metadata filter is not supported, as in the reference."""
        if filter is not None:
            raise UnsupportedError("BM25 filter pre-filtering is not yet supported")
        if k == 0 or self._bm is None:
            return []
        return self._bm.search(tenant_id, terms, k, explain)

    def query(self, req) -> List[Hit]:
        """POST /v1/query (handlers.rs:143-187) with the additive `hash` field: a vector goes to the cosine kNN,
        a hash to the Hamming space `algorithm` (default: the only hash space present), `landmarks` to identify (the Panako
        index when `algorithm` is "audiofp-panako-v1", the Wang one otherwise), `triplets` to identify_stretched (with
        bins="scaled" when `resampled` is true),
        `subfingerprints` to identify_frames, `tlsh` to nearest_tlsh, `image_record` to similar_images,
        `minhash` to similar_text;
        `terms` go through the matcher (BM25, or vector + BM25 fused by RRF: src/matcher/mod.rs:140-207)."""
        if (getattr(req, "landmarks", None) is None and getattr(req, "subfingerprints", None) is None and req.hash is None
                and getattr(req, "triplets", None) is None and getattr(req, "tlsh", None) is None
                and getattr(req, "image_record", None) is None and getattr(req, "minhash", None) is None
                and getattr(req, "terms", None)):
            from . import matcher
            hits = matcher.search(self, req)
            for rank, h in enumerate(hits):
                if h.source == HitSource.Bm25:
                    h.bm25_score, h.bm25_rank = h.score, rank + 1
            return hits
        filt = getattr(req, "filter", None)
        if filt is not None and any(getattr(req, a, None) is not None for a in
                                    ("landmarks", "subfingerprints", "triplets", "tlsh", "image_record", "minhash")):
            raise UnsupportedError("`filter` goes with a `vector` or a `hash` query; the other indexes take no filter yet")
        if getattr(req, "image_record", None) is not None:
            cfg = MultiHashConfig.from_dto(getattr(req, "multi_hash", None))
            if getattr(req, "min_score", None) is not None:
                cfg.min_score = float(req.min_score)
            hits = self.similar_images(req.tenant_id, req.image_record, req.k, getattr(req, "algorithm", None), cfg)
        elif getattr(req, "minhash", None) is not None:
            hits = self.similar_text(req.tenant_id, req.minhash, req.k, algorithm=getattr(req, "algorithm", None),
                                     threshold=getattr(req, "min_similarity", None))
        elif getattr(req, "tlsh", None) is not None:
            if getattr(req, "algorithm", None) not in (None, ALGORITHM_TLSH):
                raise InvalidArgument(f"`tlsh` goes with `algorithm` = {ALGORITHM_TLSH!r} or none")
            hits = self.nearest_tlsh(req.tenant_id, req.tlsh, req.k)
        elif getattr(req, "triplets", None) is not None:
            if getattr(req, "algorithm", None) != ALGORITHM_PANAKO:
                raise InvalidArgument(f"`triplets` need `algorithm` = {ALGORITHM_PANAKO!r}")
            match = dict(bins="scaled") if getattr(req, "resampled", False) else {}
            hits = self.identify_stretched(req.tenant_id, req.triplets, req.k, **match)
        elif getattr(req, "landmarks", None) is not None:
            panako = getattr(req, "algorithm", None) == ALGORITHM_PANAKO
            hits = self.identify(req.tenant_id, req.landmarks, req.k,
                                 algorithm=ALGORITHM_PANAKO if panako else ALGORITHM_WANG)
        elif getattr(req, "subfingerprints", None) is not None:
            hits = self.identify_frames(req.tenant_id, req.subfingerprints, req.k)
        elif req.hash is not None:
            space = req.algorithm
            if space is None:
                if len(self._ham) != 1:
                    raise InvalidArgument("`algorithm` is required when several hash spaces exist")
                space = next(iter(self._ham))
            hits = self.hamming(req.tenant_id, space, req.hash, req.k, filt)
        else:
            hits = self.knn(req.tenant_id, req.vector or [], req.k, filt)
        for rank, h in enumerate(hits):   # Matcher::search fills the rank of the only list it fused (matcher/mod.rs:140-207)
            if h.source == HitSource.Vector:
                h.vector_score, h.vector_rank = h.score, rank + 1
        return hits

    def flush(self) -> None:
        if self._sidecar is not None:
            self._sidecar.sync()
        for ix in self._all():
            ix.flush()


_IMAGE_ALGO = {tag: algo for algo, tag in _IMAGE_TAG.items()}   # image algorithm tag -> UCFP_IMG_*


def _feeds_image_match(r: Record) -> bool:
    """An `imgfprint-*-v1` record of the right length: 536 bytes for the bundle, 168 for one algorithm."""
    if r.algorithm not in _IMAGE_ALGO:
        return False
    return len(r.fingerprint) == (536 if r.algorithm == _IMAGE_TAG[7] else 168)


_MINHASH_TAGS = (ALGORITHM_MINHASH_128, ALGORITHM_LSH)


def _feeds_minhash(r: Record) -> bool:
    """A `minhash-h128` or `minhash-lsh-h128` record that is one whole MinHash signature of a valid slot count."""
    if r.algorithm not in _MINHASH_TAGS:
        return False
    try:
        minhash_slots(r.fingerprint)
    except InvalidArgument:
        return False
    return True


def _hash_spaces(r: Record):
    """(space, u64) pairs a record contributes to Hamming search."""
    fp = r.fingerprint
    rd = lambda off: int.from_bytes(fp[off:off + 8], "little")  # noqa: E731
    if r.algorithm == "imgfprint-multihash-v1" and len(fp) == 536:
        return [("imgfprint-ahash-v1", rd(64)), ("imgfprint-phash-v1", rd(232)), ("imgfprint-dhash-v1", rd(400))]
    if r.algorithm in ("imgfprint-ahash-v1", "imgfprint-phash-v1", "imgfprint-dhash-v1") and len(fp) == 168:
        return [(r.algorithm, rd(32))]
    if r.algorithm in ("simhash-b64-tf", "simhash-b64-idf") and len(fp) == 8:
        return [(r.algorithm, rd(0))]
    return []
