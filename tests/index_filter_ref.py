"""Reference for the filter tests (DESIGN F1 - F4), independent of the package: a writer of the Roaring treemap format that
can be told the type of every container (non-canonical but valid choices included), a reader, a membership function, a
brute-force filtered Hamming top-k and a damage generator.  Imports nothing from ucfp_amd."""
import struct

import numpy as np

ARRAY, BITMAP, RUN = "array", "bitmap", "run"


def _runs_of(vals):
    """Sorted distinct ints -> [(start, length - 1)] of maximal runs."""
    out = []
    for v in vals:
        if out and out[-1][0] + out[-1][1] + 1 == v:
            out[-1][1] += 1
        else:
            out.append([v, 0])
    return [(s, l) for s, l in out]


def write_container(vals, kind, split_runs=False):
    """Body bytes of one container over sorted distinct 16-bit values.  split_runs: one run per value (valid, not canonical)."""
    if kind == ARRAY:
        assert len(vals) <= 4096
        return struct.pack(f"<{len(vals)}H", *vals)
    if kind == BITMAP:
        assert len(vals) > 4096
        bits = np.zeros(65536, np.uint8)
        bits[np.asarray(vals, np.int64)] = 1
        return np.packbits(bits, bitorder="little").tobytes()      # bit v of the 1024 little-endian words
    runs = [(v, 0) for v in vals] if split_runs else _runs_of(vals)
    return struct.pack("<H", len(runs)) + b"".join(struct.pack("<HH", s, l) for s, l in runs)


def write_bitmap32(containers, force_runs_header=False):
    """containers: [(key16, sorted distinct 16-bit values, kind)] with ascending keys -> one 32-bit bitmap.  An empty list is
    the empty bitmap of form (a)."""
    n = len(containers)
    bodies = [write_container(v, kind) for _, v, kind in containers]
    has_runs = any(kind == RUN for _, _, kind in containers) or (force_runs_header and n > 0)
    if has_runs:
        flags = bytearray((n + 7) // 8)
        for i, (_, _, kind) in enumerate(containers):
            if kind == RUN:
                flags[i // 8] |= 1 << (i % 8)
        head = struct.pack("<I", 12347 | (n - 1) << 16) + bytes(flags)
    else:
        head = struct.pack("<II", 12346, n)
    head += b"".join(struct.pack("<HH", key, len(v) - 1) for key, v, _ in containers)
    if not has_runs or n >= 4:
        pos = len(head) + 4 * n
        for b in bodies:
            head += struct.pack("<I", pos)
            pos += len(b)
    return head + b"".join(bodies)


def write_treemap(maps):
    """maps: [(high32, containers)] with ascending high keys (see write_bitmap32)."""
    return struct.pack("<Q", len(maps)) + b"".join(struct.pack("<I", h) + write_bitmap32(c) for h, c in maps)


def default_kind(vals):
    return ARRAY if len(vals) <= 4096 else BITMAP


def write_ids(ids, kind_of=default_kind):
    """Any iterable of ints in [0, 2^64) -> treemap bytes; kind_of(values) picks each container's type."""
    maps = {}
    for i in sorted(set(int(x) for x in ids)):
        maps.setdefault(i >> 32, {}).setdefault((i >> 16) & 0xFFFF, []).append(i & 0xFFFF)
    return write_treemap([(h, [(k, v, kind_of(v)) for k, v in sorted(c.items())]) for h, c in sorted(maps.items())])


class Invalid(ValueError):
    pass


def read(data):
    """Treemap bytes -> (sorted list of ids, [container kinds]); Invalid for anything DESIGN F2 refuses."""
    data = bytes(data)
    pos = 0

    def take(k, what):
        nonlocal pos
        if len(data) - pos < k:
            raise Invalid(f"truncated {what} at {pos}")
        pos += k
        return data[pos - k:pos]

    (nmaps,) = struct.unpack("<Q", take(8, "count"))
    ids, kinds = [], []
    prev_high = -1
    for _ in range(nmaps):
        (high,) = struct.unpack("<I", take(4, "high key"))
        if high <= prev_high:
            raise Invalid("high keys")
        prev_high = high
        base = pos
        (cookie,) = struct.unpack("<I", take(4, "cookie"))
        if cookie == 12346:
            (n,) = struct.unpack("<I", take(4, "container count"))
            if n > 65536:
                raise Invalid("container count")
            flags, has_runs = b"", False
        elif cookie & 0xFFFF == 12347:
            n = (cookie >> 16) + 1
            flags, has_runs = take((n + 7) // 8, "run flags"), True
        else:
            raise Invalid("cookie")
        desc = struct.unpack(f"<{2 * n}H", take(4 * n, "descriptive header"))
        keys, cards = desc[0::2], [c + 1 for c in desc[1::2]]
        if any(b <= a for a, b in zip(keys, keys[1:])):
            raise Invalid("container keys")
        offs = struct.unpack(f"<{n}I", take(4 * n, "offset header")) if (not has_runs or n >= 4) else None
        for i in range(n):
            if offs is not None and offs[i] != pos - base:
                raise Invalid("offset header")
            top = high << 32 | keys[i] << 16
            if has_runs and flags[i // 8] >> (i % 8) & 1:
                (nr,) = struct.unpack("<H", take(2, "run count"))
                pairs = struct.unpack(f"<{2 * nr}H", take(4 * nr, "runs"))
                end, vals = -1, []
                for s, l in zip(pairs[0::2], pairs[1::2]):
                    if s <= end or s + l > 65535:
                        raise Invalid("runs")
                    end = s + l
                    vals.extend(range(s, end + 1))
                if len(vals) != cards[i]:
                    raise Invalid("run cardinality")
                kinds.append(RUN)
            elif cards[i] <= 4096:
                vals = list(struct.unpack(f"<{cards[i]}H", take(2 * cards[i], "array")))
                if any(b <= a for a, b in zip(vals, vals[1:])):
                    raise Invalid("array order")
                kinds.append(ARRAY)
            else:
                bits = np.unpackbits(np.frombuffer(take(8192, "bitmap"), np.uint8), bitorder="little")
                vals = np.flatnonzero(bits).tolist()
                if len(vals) != cards[i]:
                    raise Invalid("bitmap cardinality")
                kinds.append(BITMAP)
            ids.extend(top | v for v in vals)
    if pos != len(data):
        raise Invalid("trailing bytes")
    return ids, kinds


def member(data, ids):
    """bool [len(ids)]: which of the uint64 `ids` the filter holds."""
    allowed = np.array(read(data)[0], dtype=np.uint64)
    return np.isin(np.asarray(ids, dtype=np.uint64), allowed)


def hamming_topk(ids, codes, allowed_mask, queries, k):
    """Brute-force filtered Hamming top-k under (distance, id): (ids [nq, k] u64, dist [nq, k] u32, counts [nq] u32), unfilled
    places 2^64 - 1 / 2^32 - 1."""
    ids = np.asarray(ids, np.uint64)[allowed_mask]
    codes = np.asarray(codes, np.uint64)[allowed_mask]
    queries = np.asarray(queries, np.uint64)
    nq = queries.size
    out_ids = np.full((nq, k), 0xFFFFFFFFFFFFFFFF, np.uint64)
    out_d = np.full((nq, k), 0xFFFFFFFF, np.uint32)
    cnt = np.full(nq, min(k, ids.size), np.uint32)
    if ids.size == 0:
        return out_ids, out_d, cnt
    for q in range(nq):
        x = codes ^ queries[q]
        d = np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.uint32)
        order = np.lexsort((ids, d))[:k]
        out_ids[q, :order.size] = ids[order]
        out_d[q, :order.size] = d[order]
    return out_ids, out_d, cnt


def damage(data, rng):
    """One random damage of valid bytes: a flipped byte, a truncation or an extension."""
    data = bytearray(data)
    what = int(rng.integers(0, 3))
    if what == 0 and data:
        i = int(rng.integers(0, len(data)))
        data[i] ^= 1 << int(rng.integers(0, 8))
    elif what == 1 and data:
        del data[int(rng.integers(0, len(data))):]
    else:
        data += bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8))
    return bytes(data)


def hand_built():
    """name -> (bytes, sorted ids): the edge cases of DESIGN F1."""
    full = list(range(65536))
    cases = {
        "ids_0_and_max": write_ids([0, 2**64 - 1]),
        "high_key": write_ids([5 << 32 | 7, 5 << 32 | 1 << 16 | 9, 9 << 32]),
        "array_1": write_treemap([(0, [(3, [17], ARRAY)])]),
        "array_4096": write_treemap([(0, [(0, list(range(0, 8192, 2)), ARRAY)])]),
        "bitmap_4097": write_treemap([(0, [(1, list(range(0, 8194, 2)), BITMAP)])]),
        "bitmap_65536": write_treemap([(0, [(2, full, BITMAP)])]),
        "run_full": write_treemap([(0, [(0, full, RUN)])]),
        "run_to_65535": write_treemap([(0, [(7, list(range(65000, 65536)), RUN)])]),
        "run_single_value": write_treemap([(0, [(4, [123], RUN)])]),
        "run_flags_1": write_treemap([(1, [(0, [1, 2, 3, 9], RUN)])]),
        "run_flags_3": write_treemap([(0, [(0, [1, 2, 3], RUN), (1, [5, 900], ARRAY), (2, list(range(100, 300)), RUN)])]),
        "run_flags_4": write_treemap([(0, [(0, [1, 2, 3], RUN), (1, [5, 900], ARRAY), (2, list(range(100, 300)), RUN),
                                           (9, list(range(0, 10000, 2)), BITMAP)])]),
        "odd_flag_bytes": write_treemap([(0, [(i, [i, i + 1, i + 2], RUN if i % 2 else ARRAY) for i in range(9)])]),
        "empty_bitmap_inside": write_treemap([(0, []), (1, [(0, [1], ARRAY)])]),
        "count_0": write_treemap([]),
    }
    return {name: (b, read(b)[0]) for name, b in cases.items()}


def refusals():
    """name -> bytes: one case for each refusal of DESIGN F2."""
    ok = write_treemap([(0, [(0, [1, 2, 3], ARRAY), (1, list(range(0, 10000, 2)), BITMAP)])])
    runs = write_treemap([(0, [(0, [1, 2, 3, 10, 11], RUN)])])          # cookie(4) flags(1) desc(4) nruns(2) pairs
    runs4 = write_treemap([(0, [(i, [1, 2, 3], RUN) for i in range(4)])])

    def put(b, at, fmt, *v):
        b = bytearray(b)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)

    bm_at = len(ok) - 8192
    r_at = 8 + 4 + 4 + 1 + 4        # the run container of `runs`
    return {
        "truncated_count": ok[:5],
        "truncated_header": ok[:14],
        "truncated_body": ok[:-1],
        "trailing": ok + b"\0",
        "cookie": put(ok, 12, "<I", 12345),
        "high_keys": struct.pack("<Q", 2) + (struct.pack("<I", 3) + write_bitmap32([(0, [1], ARRAY)])) * 2,
        "container_keys": put(ok, 12 + 8 + 4, "<H", 0),
        "array_order": put(ok, 12 + 8 + 8 + 8, "<HHH", 1, 3, 3),
        "bitmap_popcount": put(ok, bm_at, "<Q", 0),
        "bitmap_small": write_treemap([(0, [(0, list(range(4097)), BITMAP)])])[:12 + 8 + 4 + 4]
        + struct.pack("<1024Q", *([2**64 - 1] * 64 + [0] * 960)),            # header says 4097, 4096 bits set
        "runs_unsorted": put(runs, r_at + 2, "<HHHH", 10, 1, 1, 2),
        "runs_overlap": put(runs, r_at + 2, "<HHHH", 1, 2, 3, 1),
        "runs_overflow": put(runs, r_at + 2, "<HHHH", 1, 2, 65535, 1),
        "runs_total": put(runs, r_at + 2, "<HH", 1, 3),
        "offset_header": put(ok, 12 + 8 + 8, "<I", 25),
        "offset_header_runs": put(runs4, 12 + 4 + 1 + 16, "<I", 1),
        "too_many_containers": put(ok, 16, "<I", 65537),
    }
