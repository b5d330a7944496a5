"""Query filters, the CPU half (DESIGN F1, F2): the Roaring treemap bytes as ucfp_roaring_validate and index.filter_bytes
see them, against the independent writer / reader of tests/index_filter_ref.py; the parser itself (roaring_parse.h) under
the host sanitizers in a stand-alone program."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import index_filter_ref as ref
from ucfp_amd import _lib, errors, index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "roaring_parse_check.cpp")


def validate(data):
    """(status, cardinality, message) of ucfp_roaring_validate."""
    lib = _lib.load()
    card = C.c_uint64(0)
    rc = lib.ucfp_roaring_validate(bytes(data), len(data), C.byref(card))
    return rc, int(card.value), lib.ucfp_last_error().decode() if rc else ""


def random_set(rng):
    """A random id set that mixes container shapes: sparse values, dense blocks, whole runs, several high keys."""
    ids = []
    for _ in range(int(rng.integers(0, 4))):
        top = int(rng.choice([0, 1, 7, 2**32 - 1])) << 32 | int(rng.integers(0, 4)) << 16
        shape = int(rng.integers(0, 4))
        if shape == 0:
            ids += [top | int(v) for v in rng.integers(0, 65536, int(rng.integers(1, 40)))]
        elif shape == 1:
            ids += [top | int(v) for v in rng.choice(65536, int(rng.integers(4097, 9000)), replace=False)]
        elif shape == 2:
            a = int(rng.integers(0, 65000))
            ids += [top | v for v in range(a, min(65536, a + int(rng.integers(1, 6000))))]
        else:
            ids += [top | int(v) for v in rng.integers(0, 65536, 4096)]
    return ids


def random_kind(rng):
    def kind(vals):
        if rng.integers(0, 3) == 0:
            return ref.RUN
        return ref.default_kind(vals)
    return kind


def test_round_trips_and_validate_agrees_on_cardinality():
    rng = np.random.default_rng(30)
    kinds_seen = set()
    for i in range(2000):
        ids = random_set(rng)
        data = ref.write_ids(ids, random_kind(rng))
        got, kinds = ref.read(data)
        assert got == sorted(set(ids))
        kinds_seen.update(kinds)
        rc, card, msg = validate(data)
        assert rc == 0 and card == len(got), (i, msg)
    assert kinds_seen == {ref.ARRAY, ref.BITMAP, ref.RUN}


def test_hand_built_cases():
    cases = ref.hand_built()
    assert cases["ids_0_and_max"][1] == [0, 2**64 - 1]
    assert len(cases["bitmap_65536"][1]) == 65536 and len(cases["array_4096"][1]) == 4096
    assert len(cases["bitmap_4097"][1]) == 4097 and cases["run_to_65535"][1][-1] == 7 << 16 | 65535
    assert cases["count_0"][1] == [] and cases["empty_bitmap_inside"][1] == [1 << 32 | 1]
    # the offset header of a bitmap with run flags appears at 4 containers (F1)
    assert len(cases["run_flags_4"][0]) - len(cases["run_flags_3"][0]) == 4 + 4 * 4 + 8192
    for name, (data, ids) in cases.items():
        rc, card, msg = validate(data)
        assert rc == 0 and card == len(ids), (name, msg)
        assert index.roaring_cardinality(data) == len(ids)


def test_product_writer_is_read_back_and_follows_the_4096_rule():
    rng = np.random.default_rng(31)
    sets = [[], [0], [2**64 - 1, 0, 0, 5], list(range(4096)), list(range(4097)), list(range(70000)),
            [int(x) for x in rng.integers(0, 2**64, 3000, dtype=np.uint64)],
            [int(x) for x in rng.integers(0, 1 << 18, 50000)],
            [7 << 32 | int(x) for x in rng.choice(65536, 4097, replace=False)]]
    sets += [random_set(rng) for _ in range(40)]
    for ids in sets:
        want = sorted(set(ids))
        data = index.filter_bytes(ids)
        got, kinds = ref.read(data)
        assert got == want
        assert ref.RUN not in kinds
        sizes = {}
        for v in want:
            sizes[v >> 16] = sizes.get(v >> 16, 0) + 1
        assert kinds == [ref.ARRAY if sizes[key] <= 4096 else ref.BITMAP for key in sorted(sizes)]
        assert validate(data)[:2] == (0, len(want))
        rdata = index.filter_bytes(np.array(want, np.uint64)[::-1], runs=True)      # any order, an array as well
        assert ref.read(rdata)[0] == want and validate(rdata)[:2] == (0, len(want))
    assert ref.RUN in ref.read(index.filter_bytes(range(100, 9000), runs=True))[1]
    assert ref.RUN in ref.read(index.filter_bytes([1, 2, 3, 4, 1 << 16, 2 << 16, 3 << 16 | 5], runs=True))[1]   # 4 containers
    for bad in ([-1], [2**64], [1.5], ["7"]):
        with pytest.raises(errors.UcfpError):
            index.filter_bytes(bad)


def test_every_refusal_is_refused_with_a_byte_offset():
    for name, data in ref.refusals().items():
        with pytest.raises(ref.Invalid):
            ref.read(data)
        rc, _, msg = validate(data)
        assert rc == -4 and " at byte " in msg, (name, rc, msg)
        with pytest.raises(errors.UcfpError):
            index.roaring_cardinality(data)
    assert validate(b"")[0] == -4
    assert _lib.load().ucfp_roaring_validate(None, 8, None) == -4


def test_container_and_byte_limits_are_refused():
    """F2: 2^24 containers are accepted and one 32-bit bitmap more (2^24 + 2^16) is refused; a length above 2^32 - 1 bytes is
    refused before a byte is read (so a short buffer stands in for the 4 GiB one)."""
    per = 65536
    keys = np.arange(per, dtype="<u2")
    desc = np.zeros((per, 2), "<u2")
    desc[:, 0] = keys                                                      # cardinality - 1 = 0: one value each
    head = np.array([12346, per], "<u4").tobytes() + desc.tobytes()
    offs = (len(head) + 4 * per + 2 * np.arange(per)).astype("<u4").tobytes()
    one = head + offs + (keys & np.uint16(0xFF)).astype("<u2").tobytes()   # 65536 one-value array containers
    assert ref.read(struct.pack("<QI", 1, 0) + one)[1] == [ref.ARRAY] * per

    def treemap(n_maps):
        return struct.pack("<Q", n_maps) + b"".join(struct.pack("<I", h) + one for h in range(n_maps))
    rc, card, msg = validate(treemap(256))
    assert rc == 0 and card == 1 << 24, msg
    rc, _, msg = validate(treemap(257))
    assert rc == -4 and "2^24 containers" in msg and " at byte " in msg, msg
    lib = _lib.load()
    small = treemap(1)
    assert lib.ucfp_roaring_validate(small, 1 << 32, None) == -4
    assert b"larger than 2^32 - 1 bytes" in lib.ucfp_last_error()


def damaged_cases(n=2000):
    rng = np.random.default_rng(32)
    bases = [b for b, _ in ref.hand_built().values() if len(b) < 3000]
    bases += [ref.write_ids(random_set(rng), random_kind(rng)) for _ in range(30)]
    return [ref.damage(bases[int(rng.integers(0, len(bases)))], rng) for _ in range(n)]


def probes_for(ids, rng):
    near = [i ^ 1 for i in ids[:8]] + [i + 1 for i in ids[-4:] if i + 1 < 2**64]
    return ids[:8] + ids[-8:] + near + [int(x) for x in rng.integers(0, 2**64, 4, dtype=np.uint64)]


def test_damaged_filters_always_return_a_status_and_agree_with_the_reader():
    accepted = refused = 0
    for data in damaged_cases():
        rc, card, _ = validate(data)
        try:
            ids, _ = ref.read(data)
        except ref.Invalid:
            assert rc == -4
            refused += 1
            continue
        assert rc == 0 and card == len(ids)      # (the set itself: the sanitised parser below, probe by probe)
        accepted += 1
    assert accepted > 20 and refused > 1000


def test_parser_under_asan_ubsan_agrees_with_the_reader(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "roaring_parse_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                    "-o", exe], check=True)
    rng = np.random.default_rng(33)
    cases = [b for b, _ in ref.hand_built().values()] + list(ref.refusals().values()) + damaged_cases() + [b""]
    feed, want = [], []
    for data in cases:
        try:
            ids, kinds = ref.read(data)
            probes = probes_for(ids, rng) if ids else [0, 1, 2**64 - 1]
            allowed = set(ids)
            want.append(f"0 {len(ids)} {len(kinds)} " + "".join("1" if p in allowed else "0" for p in probes))
        except ref.Invalid:
            probes = [0]
            want.append(None)
        feed.append(struct.pack("<I", len(data)) + data + struct.pack("<I", len(probes)) + struct.pack(f"<{len(probes)}Q", *probes))
    r = subprocess.run([exe], input=b"".join(feed), capture_output=True, timeout=300)
    out, err = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0 and "runtime error" not in err, out[-2000:] + err[-4000:]
    lines = out.splitlines()
    assert lines[-1] == f"ok {len(cases)}"
    for i, (line, w) in enumerate(zip(lines, want)):
        if w is None:
            assert line.startswith("-1 "), (i, line)
        else:
            assert line == w, (i, line, w)


def test_query_request_filter_field_is_additive():
    import base64
    from ucfp_amd.core import Modality, QueryRequest
    body = {"tenant_id": 7, "modality": "Image", "vector": [0.5, 0.5]}
    plain = QueryRequest.from_json(body)
    assert plain.filter is None
    assert plain == QueryRequest(tenant_id=7, modality=Modality.Image, vector=[0.5, 0.5])
    data = index.filter_bytes([3, 9])
    with_f = QueryRequest.from_json(dict(body, filter=base64.b64encode(data).decode()))
    assert with_f.filter == data and with_f.vector == plain.vector
    for bad in ("not base64 !", 5, [1, 2]):
        with pytest.raises(errors.InvalidArgument):
            QueryRequest.from_json(dict(body, filter=bad))
