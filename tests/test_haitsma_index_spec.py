"""Haitsma sub-fingerprint index spec on the CPU: the numpy reference against the literal definitions,
the `subfingerprints` field of a query body, the host-only entry points, and the inputs of the end-to-end GPU test
checked on the oracle."""
import ctypes as C

import numpy as np
import pytest

import haitsma_ref as hr
from haitsma_ref import HaitsmaRef, brute_force
from ucfp_amd.core import Hit, HitSource, QueryRequest, hit_to_json
from ucfp_amd.errors import InvalidArgument

FEATURES = ("plain", "m=1", "m=n_r", "m>n_r", "empty record", "equal records", "segment twice", "long run")


def _flip(rng, v, nbits):
    for b in rng.choice(32, nbits, replace=False):
        v ^= 1 << int(b)
    return v


def _case(seed):
    """-> (feature, records, query): every feature comes round once in eight seeds."""
    rng = np.random.default_rng(seed)
    feature = FEATURES[seed % len(FEATURES)]
    base = [int(x) for x in rng.integers(0, 2**32, 4, dtype=np.uint64)]
    alpha = base + [_flip(rng, v, n) for v in base for n in (1, 2, 3)]
    draw = lambda n: [alpha[i] for i in rng.integers(0, len(alpha), n)]  # noqa: E731
    recs = {}
    for _ in range(int(rng.integers(1, 7))):
        recs[int(rng.integers(0, 50))] = draw(int(rng.integers(1, 21)))
    src = recs[sorted(recs)[int(rng.integers(0, len(recs)))]]
    m = int(rng.integers(1, len(src) + 1))
    if feature == "m=1":
        m = 1
    elif feature == "m=n_r":
        m = len(src)
    elif feature == "empty record":
        recs[int(rng.integers(50, 60))] = []
    elif feature == "equal records":
        recs[int(rng.integers(50, 60))] = list(src)
    elif feature == "segment twice":
        seg = draw(int(rng.integers(2, 6)))
        recs[60] = seg + draw(int(rng.integers(0, 4))) + seg + draw(2)
        src, m = seg, len(seg)
    elif feature == "long run":
        m = int(rng.integers(1, 6))
        recs[61] = draw(2) + [base[0]] * (m + int(rng.integers(1, 10))) + draw(2)
        src = [base[0]] * m
    a = int(rng.integers(0, len(src) - m + 1))
    q = [_flip(rng, v, int(rng.choice([0, 0, 1, 2, 3]))) for v in src[a:a + m]]
    if feature == "m>n_r":
        q = draw(max(len(f) for f in recs.values()) + 1)
    elif feature == "plain" and rng.random() < 0.3:
        q = draw(m)                                        # unrelated to any record
    return feature, recs, q


@pytest.mark.parametrize("seed", range(320))
def test_reference_matches_definition(seed):
    _, recs, q = _case(seed)
    m = len(q)
    for max_postings in (0, 2, 5):
        ref = HaitsmaRef(recs, max_postings)
        for flip_bits in (0, 1, 2):
            full = brute_force(recs, q, 128, flip_bits, 1_000_000, max_postings)
            assert ref.query(q, 128, flip_bits, 1_000_000) == full
            cut = full[len(full) // 2][1] * 1_000_000 // (32 * m) if full else 0   # a threshold inside the list
            for k, ppm in ((1, 1_000_000), (5, 350_000), (3, cut), (128, cut), (0, 1_000_000)):
                assert ref.query(q, k, flip_bits, ppm) == brute_force(recs, q, k, flip_bits, ppm, max_postings)


def test_random_cases_cover_the_corners():
    seen = {f: 0 for f in FEATURES}
    cut = stopped = tie = twice = 0
    for seed in range(320):
        feature, recs, q = _case(seed)
        m = len(q)
        full = brute_force(recs, q, 128, 2, 1_000_000)
        seen[feature] += 1
        if feature == "m>n_r":
            assert all(len(f) < m for f in recs.values()) and full == []
        if feature == "empty record":
            assert any(len(f) == 0 for f in recs.values())
        if feature == "long run":
            assert any(f[i:i + m + 1] == [f[i]] * (m + 1) for f in recs.values() for i in range(len(f) - m))
        if full:
            ppm = full[len(full) // 2][1] * 1_000_000 // (32 * m)
            cut += 0 < len(brute_force(recs, q, 128, 2, ppm)) < len(full)
        stopped += brute_force(recs, q, 128, 2, 1_000_000, 2) != full
        tie += any(x[1] == y[1] and x[0] < y[0] for x, y in zip(full, full[1:]))
        if feature == "segment twice":
            hit = [h for h in full if h[0] == 60]
            twice += bool(hit) and hit[0][2] == 0 and recs[60][:m] == recs[60][-m - 2:-2]
    assert all(n >= 30 for n in seen.values()), seen
    assert min(cut, stopped, tie, twice) >= 10, (cut, stopped, tie, twice)


@pytest.mark.parametrize("name,recs,q,max_postings", hr.fixed_cases(), ids=[c[0] for c in hr.fixed_cases()])
def test_fixed_cases(name, recs, q, max_postings):
    ref = HaitsmaRef(recs, max_postings)
    for flip_bits in (0, 1, 2):
        for k, ppm in ((10, 1_000_000), (1, 1_000_000), (10, 350_000)):
            assert ref.query(q, k, flip_bits, ppm) == brute_force(recs, q, k, flip_bits, ppm, max_postings)


def test_fixed_cases_say_what_they_claim():
    cases = {c[0]: c[1:] for c in hr.fixed_cases()}
    q = lambda name, flip, ppm=1_000_000: HaitsmaRef(cases[name][0], cases[name][2]).query(cases[name][1], 10, flip, ppm)  # noqa: E731
    assert q("exact", 0) == [(7, 0, 1, 1.0)]
    assert [h[:3] for h in q("m=1", 0)] == [(7, 0, 1)]
    assert [h[:3] for h in q("m=1", 1)] == [h[:3] for h in q("m=1", 2)] == [(7, 0, 1), (2, 1, 1)]   # a ^ 1 beats a ^ 3
    assert [h[:3] for h in q("m=n_r", 0)] == [(7, 0, 0), (8, 3, 0)]
    assert q("m>n_r", 2) == []
    assert [h[:3] for h in q("empty record", 0)] == [(7, 0, 1)]
    assert [h[:3] for h in q("equal records", 0)] == [(5, 0, 1), (11, 0, 1)]          # the tie goes to the smaller id
    assert [h[:3] for h in q("segment twice", 0)] == [(4, 0, 0), (6, 0, 0)]           # the smaller d wins
    assert [h[:3] for h in q("long run", 0)] == [(4, 0, 0), (6, 0, 0)]
    assert [h[:3] for h in q("long run stopped", 0)] == [(4, 0, 38), (6, 0, 7)]       # only through b: a is stopped
    # record 6 lies 3 bits from the query in every frame: never a candidate, though its dist (9) is under the threshold
    assert q("flips", 0) == [] and q("flips", 1) == [] and [h[:3] for h in q("flips", 2)] == [(4, 6, 1)]
    assert [h[:3] for h in q("two bits on one frame only", 1)] == [(6, 3, 0)]
    assert [h[:3] for h in q("two bits on one frame only", 2)] == [(6, 3, 0), (4, 10, 0)]
    # 3 of 96 bits = 31 250 ppm exactly: the threshold is inclusive, and cuts the list
    assert [h[:3] for h in q("two bits on one frame only", 2, 31_250)] == [(6, 3, 0)]
    assert q("two bits on one frame only", 2, 31_249) == []


def test_query_body_subfingerprints():
    r = QueryRequest.from_json({"tenant_id": 3, "modality": "Audio", "subfingerprints": [1, 0xFFFFFFFF, 7], "k": 4})
    assert r.subfingerprints == np.array([1, 0xFFFFFFFF, 7], "<u4").tobytes() and r.k == 4 and r.landmarks is None
    raw = np.array([9, 1], "<u4").tobytes()
    assert QueryRequest.from_json({"tenant_id": 0, "modality": "Audio", "subfingerprints": raw}).subfingerprints == raw
    assert QueryRequest.from_json({"tenant_id": 0, "modality": "Audio", "subfingerprints": []}).subfingerprints == b""
    for bad in (raw[:7], raw + b"\0", [1 << 32], [-1], ["1"], [[1, 2]], [1.5], 5):
        with pytest.raises(InvalidArgument):
            QueryRequest.from_json({"tenant_id": 0, "modality": "Audio", "subfingerprints": bad})
    with pytest.raises(InvalidArgument, match="subfingerprints"):
        QueryRequest.from_json({"tenant_id": 1, "modality": "Audio"})
    assert QueryRequest.from_json({"tenant_id": 1, "modality": "Image", "vector": [1]}).subfingerprints is None


def test_haitsma_hit_json():
    h = hit_to_json(Hit(tenant_id=1, record_id=9, score=0.9, source=HitSource.Haitsma, distance=819, offset=412))
    assert h["source"] == "haitsma" and h["distance"] == 819 and h["offset"] == 412 and "votes" not in h
    v = hit_to_json(Hit(tenant_id=1, record_id=9, score=0.5))
    assert "distance" not in v and "offset" not in v


def test_host_only_abi():
    from ucfp_amd import _lib
    lib = _lib.load()
    assert [lib.ucfp_haitsma_index_probes(f) for f in (0, 1, 2, 3, 99)] == [1, 33, 529, 0, 0]
    assert [hr.masks(f).size for f in (0, 1, 2)] == [1, 33, 529] and np.unique(hr.masks(2)).size == 529
    out = C.c_void_p(0x1)
    assert lib.ucfp_haitsma_index_create(None, 0, 0, C.byref(out)) == -4      # UCFP_E_INVALID
    lib.ucfp_haitsma_index_destroy(None)


@pytest.mark.parametrize("name,gen,corpus_seed,excerpt_seed,snr,flips", hr.END_TO_END, ids=[c[0] for c in hr.END_TO_END])
def test_end_to_end_inputs_identify_on_the_oracle(name, gen, corpus_seed, excerpt_seed, snr, flips):
    """The inputs of the end-to-end GPU test, on the CPU oracle: the source record first with its offset within one frame
    of s0 / 64 and no other record, for 24 of 24 excerpts at every listed flip_bits."""
    import oracle
    oracle.build()
    xs = hr.corpus(gen, corpus_seed)
    ref = HaitsmaRef({hr.FIRST_ID + i: oracle.haitsma(x, hr.SR) for i, x in enumerate(xs)})
    qs = [(s0, oracle.haitsma(clip, hr.SR)) for s0, clip in hr.excerpts(xs, snr, excerpt_seed)]
    assert all(q.size == 256 for _, q in qs)
    for flip_bits in flips:
        good = [hr.identified(ref.query(q, 5, flip_bits, 350_000), hr.FIRST_ID + i, s0) for i, (s0, q) in enumerate(qs)]
        print(name, "flip_bits", flip_bits, "identified", sum(good), "of", len(good))
        assert sum(good) == 24, (name, flip_bits, good)
