"""Image match spec without a GPU: the numpy reference against a scalar transcription, the
host-only C function against the reference bit for bit, the config rules, and the query body."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import image_match_ref as ref
from ucfp_amd import _lib, image
from ucfp_amd.core import Hit, HitSource, Modality, QueryRequest, hit_to_json
from ucfp_amd.errors import InvalidArgument

F = np.float32
THRESHOLDS = (0, 1, 32, 63, 64)


def _records(rng, n, size):
    return rng.integers(0, 256, (n, size), dtype=np.uint8)


def _near(rng, rec, flips):
    """A copy with `flips` random bits of the code bytes flipped (so the pairs are not all near distance 32)."""
    out = rec.copy()
    starts = [32] if rec.size == 168 else [64, 232, 400]
    for _ in range(flips):
        s = starts[rng.integers(len(starts))]
        out[s + rng.integers(136)] ^= np.uint8(1 << rng.integers(8))
    return out


def _random_cfg(rng, T=None):
    w = [float(F(rng.random())) for _ in range(5)]
    for i in range(5):                       # exact zeros and ones among them, never an invalid combination
        r = rng.random()
        if r < 0.1:
            w[i] = 0.0
        elif r < 0.2:
            w[i] = 1.0
    if w[0] == w[1] == w[2] == 0.0:
        w[1] = 0.5
    if w[3] == w[4] == 0.0:
        w[4] = 0.25
    return ref.Cfg(w[0], w[1], w[2], w[3], w[4], int(rng.integers(0, 65)) if T is None else T, 0.0)


def _c_cfg(cfg):
    return _lib.ImageMatchConfig(cfg.ahash_weight, cfg.phash_weight, cfg.dhash_weight, cfg.global_weight, cfg.block_weight,
                                 cfg.block_distance_threshold, cfg.min_score)


def _c_score(a, b, algo, cfg=None):
    out = C.c_float(-7.0)
    c = _c_cfg(cfg) if cfg is not None else None
    rc = _lib.load().ucfp_image_match_score(bytes(a), bytes(b), algo, C.byref(c) if c is not None else None, C.byref(out))
    return rc, out.value


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def _scalar_score(a: bytes, b: bytes, cfg):
    """M1-M3 in plain Python: every product and sum rounded to f32 through struct."""
    starts = [32] if len(a) == 168 else [64, 232, 400]
    wg, wb = _f32(cfg.global_weight), _f32(cfg.block_weight)
    s = []
    for st in starts:
        ca = [int.from_bytes(a[st + 8 * i:st + 8 * i + 8], "little") for i in range(17)]
        cb = [int.from_bytes(b[st + 8 * i:st + 8 * i + 8], "little") for i in range(17)]
        g = bin(ca[0] ^ cb[0]).count("1")
        S = 0
        for i in range(1, 17):
            d = bin(ca[i] ^ cb[i]).count("1")
            if d <= cfg.block_distance_threshold:
                S += 64 - d
        sg = _f32(float(64 - g) * 0.015625)
        sb = _f32(float(S) * 0.0009765625)
        s.append(_f32(_f32(wg * sg) + _f32(wb * sb)))
    if len(s) == 1:
        return s[0]
    wa, wp, wd = _f32(cfg.ahash_weight), _f32(cfg.phash_weight), _f32(cfg.dhash_weight)
    return _f32(_f32(_f32(wa * s[0]) + _f32(wp * s[1])) + _f32(wd * s[2]))


@pytest.mark.parametrize("size", [168, 536])
def test_reference_equals_scalar_transcription(size):
    rng = np.random.default_rng(size)
    q = _records(rng, 6, size)
    rows = np.stack([_near(rng, q[i % 6], int(rng.integers(0, 200))) for i in range(40)])
    for cfg in [ref.Cfg()] + [_random_cfg(rng) for _ in range(4)]:
        sm = ref.score_matrix(q, rows, cfg)
        assert sm.dtype == np.float32 and sm.shape == (6, 40)
        for i in range(6):
            for j in range(40):
                assert _bits(float(sm[i, j])) == _bits(_scalar_score(q[i].tobytes(), rows[j].tobytes(), cfg)), (i, j, cfg)


def test_reference_codes_and_topk():
    rec = np.zeros((1, 536), np.uint8)
    rec[0, 64:72] = np.frombuffer((0x0102030405060708).to_bytes(8, "little"), np.uint8)
    rec[0, 408:416] = 0xFF
    c = ref.codes(rec)
    assert c.shape == (1, 3, 17) and c[0, 0, 0] == 0x0102030405060708 and c[0, 2, 1] == 0xFFFFFFFFFFFFFFFF and c[0, 1].sum() == 0
    one = np.zeros((2, 168), np.uint8)
    one[1, 160:168] = 1
    assert ref.codes(one).shape == (2, 1, 17) and ref.codes(one)[1, 0, 16] == 0x0101010101010101
    with pytest.raises(ValueError):
        ref.codes(np.zeros((1, 100), np.uint8))
    ids, sc, n = ref.topk([9, 3, 5, 7], np.array([0.5, 0.75, 0.75, 0.25], F), 3, 0.5)
    assert ids.tolist() == [3, 5, 9] and sc.tolist() == [0.75, 0.75, 0.5] and n == 3
    ids, sc, n = ref.topk([9, 3], np.array([0.5, 0.75], F), 4, 0.6)
    assert ids.tolist() == [3] + [ref.INVALID_ID] * 3 and sc.tolist() == [0.75, -1.0, -1.0, -1.0] and n == 1


@pytest.mark.parametrize("size,algo", [(168, image.PHASH), (536, image.MULTI)])
def test_c_score_equals_reference_bit_for_bit(size, algo):
    """10 200 pairs per record size: default and random valid configs, every threshold of the issue among them."""
    rng = np.random.default_rng(1000 + size)
    cfgs = [None] + [ref.Cfg(block_distance_threshold=T) for T in THRESHOLDS] + [_random_cfg(rng, T) for T in THRESHOLDS] \
        + [_random_cfg(rng) for _ in range(6)]
    pairs = 0
    for cfg in cfgs:
        q = _records(rng, 10, size)
        rows = np.stack([_near(rng, q[i % 10], int(rng.integers(0, 400))) if i % 3 else _records(rng, 1, size)[0]
                         for i in range(60)])
        sm = ref.score_matrix(q, rows, cfg)
        for i in range(10):
            for j in range(60):
                rc, got = _c_score(q[i], rows[j], algo, cfg)
                assert rc == 0
                assert _bits(got) == _bits(float(sm[i, j])), (cfg, i, j, got, float(sm[i, j]))
                pairs += 1
    assert pairs >= 10000


def test_single_algorithm_ignores_the_algorithm_weights_and_the_algo_tag():
    rng = np.random.default_rng(5)
    a, b = _records(rng, 2, 168)
    b = _near(rng, a, 60)
    base = _c_score(a, b, image.PHASH, ref.Cfg())
    for algo in (image.AHASH, image.PHASH, image.DHASH):
        assert _c_score(a, b, algo, ref.Cfg(0.0, 0.0, 0.0)) == base        # all three zero is fine on a 168-byte record
        assert _c_score(a, b, algo, ref.Cfg(1.0, 0.25, 0.5)) == base
    assert image.match_score(a, b) == base[1]


@pytest.mark.parametrize("size,algo", [(168, image.AHASH), (536, image.MULTI)])
def test_self_score_is_one_with_the_defaults(size, algo):
    rng = np.random.default_rng(7)
    for rec in _records(rng, 50, size):
        assert _c_score(rec, rec, algo) == (0, 1.0)
        assert _c_score(rec, rec, algo, ref.Cfg()) == (0, 1.0)
        assert float(ref.score_matrix(rec[None], rec[None])[0, 0]) == 1.0
        assert image.match_score(rec.tobytes(), rec.tobytes()) == 1.0
        assert image.match_score(rec.tobytes(), rec.tobytes(), image.MultiHashConfig()) == 1.0


@pytest.mark.parametrize("T", [0, 1, 31, 32, 63])
def test_block_distance_exactly_t_counts_and_t_plus_one_does_not(T):
    """global only off (block_weight 1, global_weight 0 is allowed), one algorithm: the score is S / 1024."""
    a = np.zeros(168, np.uint8)
    cfg = ref.Cfg(global_weight=0.0, block_weight=1.0, block_distance_threshold=T)

    def with_block_distance(d):
        b = a.copy()
        v = (1 << d) - 1
        b[40:48] = np.frombuffer(v.to_bytes(8, "little"), np.uint8)     # block 0 at distance d, the other 15 identical
        return b
    at, above = with_block_distance(T), with_block_distance(T + 1)
    assert _c_score(a, at, image.DHASH, cfg) == (0, (15 * 64 + 64 - T) / 1024.0)
    assert _c_score(a, above, image.DHASH, cfg) == (0, 15 * 64 / 1024.0)
    assert float(ref.score_matrix(a[None], at[None], cfg)[0, 0]) == (15 * 64 + 64 - T) / 1024.0
    assert float(ref.score_matrix(a[None], above[None], cfg)[0, 0]) == 15 * 64 / 1024.0


def test_threshold_64_is_the_plain_mean_block_similarity():
    rng = np.random.default_rng(11)
    a, b = _records(rng, 2, 168)
    cfg = ref.Cfg(global_weight=0.0, block_weight=1.0, block_distance_threshold=64)
    c = ref.codes(np.stack([a, b]))
    d = sum(bin(int(c[0, 0, i]) ^ int(c[1, 0, i])).count("1") for i in range(1, 17))
    assert _c_score(a, b, image.PHASH, cfg) == (0, (1024 - d) / 1024.0)


def test_default_config_call():
    c = _lib.ImageMatchConfig()
    _lib.load().ucfp_image_match_config_default(C.byref(c))
    d = image.MultiHashConfig()
    assert (c.ahash_weight, c.phash_weight, c.dhash_weight, c.global_weight, c.block_weight) == \
        tuple(float(F(x)) for x in (d.ahash_weight, d.phash_weight, d.dhash_weight, d.global_weight, d.block_weight))
    assert (c.block_distance_threshold, c.min_score) == (32, 0.0)
    assert (d.ahash_weight, d.phash_weight, d.dhash_weight, d.global_weight, d.block_weight, d.block_distance_threshold,
            d.min_score) == (0.1, 0.6, 0.3, 0.4, 0.6, 32, 0.0)
    _lib.load().ucfp_image_match_config_default(None)       # a NULL pointer is ignored


INVALID = [
    dict(ahash_weight=math.nan), dict(phash_weight=math.inf), dict(dhash_weight=-0.25), dict(global_weight=1.5),
    dict(block_weight=-math.inf), dict(global_weight=math.nan), dict(block_weight=1.0000001),
    dict(global_weight=0.0, block_weight=0.0),
    dict(block_distance_threshold=65), dict(block_distance_threshold=0xFFFFFFFF),
    dict(min_score=math.nan), dict(min_score=math.inf), dict(min_score=-0.5),
]


@pytest.mark.parametrize("bad", INVALID, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in INVALID])
@pytest.mark.parametrize("size,algo", [(168, image.PHASH), (536, image.MULTI)])
def test_invalid_configs_are_refused(bad, size, algo):
    rec = np.zeros(size, np.uint8)
    rc, _ = _c_score(rec, rec, algo, ref.Cfg(**bad))
    assert rc == -4                                          # UCFP_E_INVALID
    assert b"image match" in _lib.load().ucfp_last_error()
    with pytest.raises(InvalidArgument):
        image.match_score(rec.tobytes(), rec.tobytes(), image.MultiHashConfig(**bad))


def test_all_algorithm_weights_zero_is_invalid_on_a_bundle_only():
    cfg = ref.Cfg(0.0, 0.0, 0.0)
    assert _c_score(np.zeros(536, np.uint8), np.zeros(536, np.uint8), image.MULTI, cfg)[0] == -4
    assert _c_score(np.zeros(168, np.uint8), np.zeros(168, np.uint8), image.PHASH, cfg) == (0, 1.0)
    assert _c_score(np.zeros(536, np.uint8), np.zeros(536, np.uint8), image.MULTI, ref.Cfg(0.0, 1.0, 0.0)) == (0, 1.0)


def test_bad_algo_and_null_arguments():
    rec = bytes(536)
    out = C.c_float(0.0)
    lib = _lib.load()
    for algo in (0, 3, 5, 6, 8):
        assert lib.ucfp_image_match_score(rec, rec, algo, None, C.byref(out)) == -4
    assert lib.ucfp_image_match_score(None, rec, 7, None, C.byref(out)) == -4
    assert lib.ucfp_image_match_score(rec, None, 7, None, C.byref(out)) == -4
    assert lib.ucfp_image_match_score(rec, rec, 7, None, None) == -4
    # an index needs a context; the argument checks come first and need no device
    h = C.c_void_p()
    assert lib.ucfp_image_match_index_create(None, 7, 0, C.byref(h)) == -4
    assert lib.ucfp_image_match_index_query(None, 0, rec, 1, 1, None, None, None, None) == -4
    with pytest.raises(InvalidArgument):
        image.match_score(bytes(168), bytes(536))
    with pytest.raises(InvalidArgument):
        image.match_score(bytes(100), bytes(100))


def test_multi_hash_config_from_dto():
    d = image.MultiHashConfig.from_dto({"phash-weight": 0.5, "dhash-weight": 0.25, "ahash-weight": 0.125, "global-weight": 1,
                                        "block-weight": 0.75, "block-distance-threshold": 20})
    assert d == image.MultiHashConfig(0.125, 0.5, 0.25, 1, 0.75, 20, 0.0)
    assert image.MultiHashConfig.from_dto({}) == image.MultiHashConfig()
    assert image.MultiHashConfig.from_dto(None) == image.MultiHashConfig()
    # Option fields: null is the default; keys the DTO does not have (snake case included) are ignored, as serde does
    assert image.MultiHashConfig.from_dto({"phash-weight": None, "phash_weight": 0.9, "else": 1}) == image.MultiHashConfig()
    for bad in ({"phash-weight": "0.5"}, {"block-distance-threshold": 1.5}, {"block-distance-threshold": -1},
                {"global-weight": True}, {"block-distance-threshold": 1 << 32}, [1, 2]):
        with pytest.raises(InvalidArgument):
            image.MultiHashConfig.from_dto(bad)
    # the value is what fingerprint_multi_with is handed; its range is checked where it is used
    with pytest.raises(InvalidArgument):
        image.match_score(bytes(536), bytes(536), image.MultiHashConfig.from_dto({"phash-weight": 2.0}))


def test_match_algo():
    assert image.match_algo(536) == image.MULTI and image.match_algo(536, image.ALGORITHM_MULTIHASH) == image.MULTI
    assert image.match_algo(168, image.ALGORITHM_AHASH) == image.AHASH and image.match_algo(168, image.ALGORITHM_DHASH) == image.DHASH
    for n, tag in ((168, image.ALGORITHM_MULTIHASH), (536, image.ALGORITHM_PHASH), (167, None), (0, None), (168, "tlsh-128-1")):
        with pytest.raises(InvalidArgument):
            image.match_algo(n, tag)


def test_query_request_image_record_round_trips():
    rng = np.random.default_rng(3)
    for size, tag in ((168, "imgfprint-dhash-v1"), (536, "imgfprint-multihash-v1")):
        rec = _records(rng, 1, size)[0].tobytes()
        for wire in (list(rec), rec.hex(), rec.hex().upper(), rec, bytearray(rec)):
            r = QueryRequest.from_json({"tenant_id": 4, "modality": "Image", "image_record": wire})
            assert r.image_record == rec and r.algorithm is None and r.multi_hash is None and r.min_score is None
            assert (r.tenant_id, r.modality, r.k, r.vector, r.hash, r.tlsh, r.terms) == (4, Modality.Image, 10, None, None, None, [])
        r = QueryRequest.from_json({"tenant_id": 4, "modality": "Image", "k": 3, "image_record": list(rec), "algorithm": tag,
                                    "multi_hash": {"phash-weight": 0.5}, "min_score": 0.25})
        assert (r.k, r.algorithm, r.multi_hash, r.min_score) == (3, tag, {"phash-weight": 0.5}, 0.25)
        assert image.MultiHashConfig.from_dto(r.multi_hash).phash_weight == 0.5
    bundle, single = list(bytes(536)), list(bytes(168))
    for bad in ({"image_record": single[:-1]}, {"image_record": bundle + [0]}, {"image_record": []},
                {"image_record": single[:-1] + [256]}, {"image_record": single[:-1] + [-1]}, {"image_record": single[:-1] + [True]},
                {"image_record": "zz" * 168}, {"image_record": "0" * 335}, {"image_record": 5}, {"image_record": {"a": 1}},
                {"image_record": single, "algorithm": "imgfprint-multihash-v1"},
                {"image_record": bundle, "algorithm": "imgfprint-phash-v1"},
                {"image_record": bundle, "algorithm": "tlsh-128-1"},
                {"image_record": bundle, "multi_hash": [1]}, {"image_record": bundle, "multi_hash": "x"},
                {"image_record": bundle, "min_score": "0.5"}, {"image_record": bundle, "min_score": True}):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json({"tenant_id": 1, "modality": "Image", **bad})


def test_bodies_the_reference_accepts_parse_as_before():
    r = QueryRequest.from_json({"tenant_id": 7, "modality": "Image", "vector": [0.6, 0.6, 0]})
    assert (r.tenant_id, r.modality, r.k, r.vector, r.hash, r.image_record, r.multi_hash, r.min_score) == \
        (7, Modality.Image, 10, [0.6, 0.6, 0.0], None, None, None, None)
    # `multi_hash` and `min_score` belong to an `image_record` query: elsewhere they are not looked at
    r = QueryRequest.from_json({"tenant_id": 7, "modality": "Image", "vector": [1.0], "multi_hash": "x", "min_score": "y"})
    assert r.multi_hash is None and r.min_score is None and r.image_record is None
    with pytest.raises(InvalidArgument):
        QueryRequest.from_json({"tenant_id": 1, "modality": "Image"})
    out = hit_to_json(Hit(tenant_id=1, record_id=9, score=0.5, source=HitSource.ImageMatch))
    assert HitSource.ImageMatch == "image-match" and out["source"] == "image-match"
    assert list(out) == ["tenant_id", "record_id", "score", "source", "vector_score", "bm25_score", "vector_rank", "bm25_rank",
                         "term_hits"]
