"""TLSH 128/1 without a GPU: the Pearson table, the committed L table and the host distance against the
restatement (tests/tlsh_ref.py), the restatement against its stored digests, the record shape, and -- for whoever has the
`tlsh` module -- the restatement against the published implementation."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import tlsh_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    from ucfp_amd import _lib
    return _lib.load()


def test_pearson_table():
    assert sorted(ref.V) == list(range(256))
    assert hashlib.sha256(bytes(ref.V)).hexdigest() == ref.V_SHA256
    assert [ref.V[s] for s in (0, 2, 3, 5, 7, 11, 13)] == [1, 49, 12, 178, 166, 84, 230]   # the published pre-mapped salts
    assert ref.bm(2, 5, 6, 7) == ref.V[ref.V[ref.V[49 ^ 5] ^ 6] ^ 7]


def _lcap_np(n):
    ln = np.log(n.astype(np.float64))
    return np.where(n <= 656, np.floor(ln / 0.4054651),
                    np.where(n <= 3199, np.floor(ln / 0.26236426 - 8.72777), np.floor(ln / 0.095310180 - 62.5472))).astype(np.int64)


def test_lvalue_at_every_class_boundary(lib):
    n = np.arange(1, 1 << 24, dtype=np.int64)
    c = _lcap_np(n)
    assert (np.diff(c) >= 0).all()
    last = n[:-1][np.diff(c) != 0]            # the largest n of each class below 2^24
    assert last.size > 100 and 656 in last
    for m in last.tolist():
        for x in (m, m + 1):                  # both sides, against the float64 formula as the spec writes it
            assert lib.ucfp_tlsh_lvalue(x) == ref.lvalue(x), x
        assert ref.lvalue(m + 1) == ref.lvalue(m) + 1
    for x in (50, 656, 657, 3199, 3200, (1 << 24) - 1, 1 << 24, (1 << 31) - 1):
        assert lib.ucfp_tlsh_lvalue(x) == ref.lvalue(x), x
    assert lib.ucfp_tlsh_lvalue(50) == math.floor(math.log(50) / 0.4054651) == 9
    assert lib.ucfp_tlsh_lvalue((1 << 31) - 1) == 162


def _dist(lib, a, b):
    return int(lib.ucfp_tlsh_distance(bytes(a), bytes(b)))


def test_distance_header_fields_exhaustively(lib):
    body = bytes(range(32))
    want_l = np.zeros((256, 256), np.int64)
    for x in range(256):                      # every pair of L bytes (as stored: nibbles swapped)
        for y in range(256):
            a, b = bytes([7, x, 0x5A]) + body, bytes([7, y, 0x5A]) + body
            ld = min(abs(ref.swap(x) - ref.swap(y)), 256 - abs(ref.swap(x) - ref.swap(y)))
            want_l[x, y] = ld if ld <= 1 else 12 * ld
            assert _dist(lib, a, b) == want_l[x, y], (x, y)
    assert want_l.max() == 1536 and ref.distance(bytes([7, 0x00, 0]) + body, bytes([7, 0x08, 0]) + body) == 1536
    for shift in (4, 0):                      # every pair of each Q nibble
        for x in range(16):
            for y in range(16):
                a, b = bytes([7, 3, x << shift]) + body, bytes([7, 3, y << shift]) + body
                q = min(abs(x - y), 16 - abs(x - y))
                assert _dist(lib, a, b) == ref.distance(a, b) == (q if q <= 1 else 12 * (q - 1)), (shift, x, y)
    a = bytes([0x12, 3, 4]) + body
    assert _dist(lib, a, bytes([0x12, 3, 4]) + body) == 0 and _dist(lib, a, bytes([0x13, 3, 4]) + body) == 1
    # wrap-around: L 255 next to 0, a Q nibble 15 next to 0
    assert _dist(lib, bytes([0, 0xFF, 0]) + body, bytes([0, 0x00, 0]) + body) == 1
    assert _dist(lib, bytes([0, 0, 0xF0]) + body, bytes([0, 0, 0x00]) + body) == 1
    assert _dist(lib, bytes([0, 0, 0x0F]) + body, bytes([0, 0, 0x01]) + body) == 12


def test_distance_bodies(lib):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (10_000, 35), dtype=np.uint8)
    b = rng.integers(0, 256, (10_000, 35), dtype=np.uint8)
    a[:, :3] = b[:, :3] = (9, 9, 9)           # bodies only
    b[:100, 3:] = a[:100, 3:] ^ (1 << rng.integers(0, 8, (100, 32), dtype=np.uint8))   # and near ones
    for i in range(a.shape[0]):
        want = ref.distance(a[i].tobytes(), b[i].tobytes())
        assert _dist(lib, a[i].tobytes(), b[i].tobytes()) == want, i
        assert _dist(lib, b[i].tobytes(), a[i].tobytes()) == want, i
    zero, three = bytes(35), bytes(3) + b"\xff" * 32
    assert _dist(lib, zero, three) == ref.distance(zero, three) == 768
    far = bytes([0x10, 0x08, 0x88]) + b"\xff" * 32      # checksum differs, L half a ring away, both Q half a ring away
    assert _dist(lib, zero, far) == ref.distance(zero, far) == ref.MAX_DISTANCE == 2473
    for i in range(200):
        assert _dist(lib, a[i].tobytes(), a[i].tobytes()) == 0


def test_distance_matrix_is_the_scalar_distance():
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 256, (40, 35), dtype=np.uint8)
    dm = ref.distance_matrix(rows[:7], rows)
    for i in range(7):
        for j in range(40):
            assert dm[i, j] == ref.distance(rows[i].tobytes(), rows[j].tobytes())
    ids = np.arange(40, dtype=np.uint64)[::-1].copy()
    t_ids, t_d, t_s, t_n = ref.topk(ids, rows, rows[:7], 5)
    for i in range(7):
        order = sorted(range(40), key=lambda j: (dm[i, j], ids[j]))[:5]
        assert t_ids[i].tolist() == [int(ids[j]) for j in order] and t_d[i].tolist() == [int(dm[i, j]) for j in order]
    assert (t_n == 5).all() and t_s[0, 0] == np.float32(1.0)


def test_golden_digests_of_the_restatement():
    g = json.load(open(os.path.join(HERE, "golden", "tlsh_v1.json")))
    assert g["algorithm"] == "tlsh-128-1" and len(g["cases"]) >= 10
    for c in g["cases"]:
        d = ref.digest(bytes.fromhex(c["input_hex"]))
        assert (ref.hexdigest(d) if d is not None else None) == c["digest"], c["name"]


def test_refusals_and_behaviour_of_the_restatement():
    assert ref.digest(b"x" * 49) is None and ref.digest(b"a" * 100) is None
    assert ref.nonzero_buckets(b"acabacbaacacababaaccbcabccababcbcabcacabacacaaacbaaaaccbbbaaabcbcabcbaaca") == 64
    assert ref.nonzero_buckets(b"cabaabbaaacbabbaacabbccbcbbbbcaababcaacbbccabbccaabaaccabaacaaacbcbcbaaacc") == 65
    g = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "tlsh_v1.json")))["cases"]}
    a = ref.digest(bytes.fromhex(g["prose_700_words"]["input_hex"]))
    b = ref.digest(bytes.fromhex(g["prose_700_words_edited"]["input_hex"]))
    c = ref.digest(bytes.fromhex(g["pangram_x40"]["input_hex"]))
    assert ref.distance(a, a) == 0 and ref.distance(a, b) == ref.distance(b, a)
    assert ref.distance(a, b) < 30 < 150 < ref.distance(a, c)      # an edit stays near, another document does not


def test_record_shape(monkeypatch):
    """fingerprint_tlsh's record (text.rs:452-484), with the restatement standing in for the kernel."""
    from ucfp_amd import core, text
    from ucfp_amd.errors import InvalidArgument, ModalityError

    def fake_batch(docs, opts=None, ctx=None):
        return ref.digest_batch([text._tlsh_input(d, opts or text.TextOpts()) for d in docs])

    monkeypatch.setattr(text, "tlsh_batch", fake_batch)
    doc = "The Quick Brown Fox jumps over the lazy dog, again and again: 0123456789."
    rec = text.fingerprint_tlsh(doc, text.TextOpts(), 3, 77)
    want = ref.digest(doc.casefold().encode())                      # the default canonicaliser folds case
    assert rec.fingerprint == ref.hexdigest(want).encode() and len(rec.fingerprint) == 72 and rec.fingerprint[:2] == b"T1"
    assert rec.fingerprint[2:].decode() == rec.fingerprint[2:].decode().upper()
    assert (rec.algorithm, rec.modality, rec.text, rec.tenant_id, rec.record_id) == ("tlsh-128-1", core.Modality.Text, doc, 3, 77)
    assert rec.format_version == text.FORMAT_VERSION and rec.embedding is None and rec.config_hash == text.CONFIG_HASH_UNKNOWN
    assert text.fingerprint_tlsh(doc, text.TextOpts(), 3, 77, config_hash_value=5).config_hash == 5
    with pytest.raises(ModalityError):
        text.fingerprint_tlsh("too short", text.TextOpts(), 1, 1)
    # every form of a digest reaches the same 35 bytes
    for form in (want, rec.fingerprint, rec.fingerprint.decode(), rec.fingerprint[2:], np.frombuffer(want, np.uint8)):
        assert text.tlsh_digest_bytes(form) == want
        assert text.tlsh_distance(form, want) == 0
    for bad in (b"T1" + b"0" * 69, "zz" * 35, 5):
        with pytest.raises(InvalidArgument):
            text.tlsh_digest_bytes(bad)


def test_query_body_takes_a_tlsh_digest():
    from ucfp_amd.core import Hit, HitSource, Modality, QueryRequest, hit_to_json
    from ucfp_amd.errors import InvalidArgument
    raw = bytes(range(35))
    s = ref.hexdigest(raw)
    for form in (s, s[2:], list(raw), raw):
        r = QueryRequest.from_json({"tenant_id": 4, "modality": "Text", "tlsh": form, "k": 3})
        assert (r.tlsh, r.k, r.modality, r.vector, r.hash, r.algorithm) == (raw, 3, Modality.Text, None, None, None)
    assert QueryRequest.from_json({"tenant_id": 4, "modality": "Text", "tlsh": s, "algorithm": "tlsh-128-1"}).tlsh == raw
    for bad in ({"tlsh": s, "algorithm": "minhash-h128"}, {"tlsh": s[:-1]}, {"tlsh": list(raw)[:-1]}, {"tlsh": "g" * 70}, {"tlsh": 7}):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json({"tenant_id": 4, "modality": "Text", **bad})
    assert QueryRequest.from_json({"tenant_id": 7, "modality": "Image", "vector": [1.0]}).tlsh is None
    out = hit_to_json(Hit(tenant_id=1, record_id=9, score=0.5, source=HitSource.Tlsh, distance=40))
    assert out["source"] == "tlsh" and out["distance"] == 40


def test_against_the_published_implementation():
    """For whoever has the `tlsh` Python module: the restatement's digests and distances are the module's."""
    tlsh = pytest.importorskip("tlsh")
    g = json.load(open(os.path.join(HERE, "golden", "tlsh_v1.json")))
    made = []
    for c in g["cases"]:
        data = bytes.fromhex(c["input_hex"])
        theirs = tlsh.hash(data)
        if c["digest"] is None:
            assert theirs in ("TNULL", "", None), c["name"]
        else:
            assert theirs == c["digest"], c["name"]
            made.append(c["digest"])
    for a in made:
        for b in made:
            assert tlsh.diff(a, b) == ref.distance(bytes.fromhex(a[2:]), bytes.fromhex(b[2:]))
