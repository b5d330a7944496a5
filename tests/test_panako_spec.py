"""Panako triplets on the CPU: the two readings of the spec in tests/panako_ref.py agree; with the triplet
stage switched off the walk is `oracle.wang`; every record keeps the invariants of P3-P6; the host-only sizing helper;
the wire format of a Panako identification query; and the identification condition of P7, with `LandmarkRef` alone."""
import ctypes as C

import numpy as np
import pytest

import panako_ref as pr
from landmark_ref import LandmarkRef

WANG_CONFIGS = [(10, 63, 64, 30, -50.0), (5, 96, 96, 30, -50.0), (12, 96, 96, 30, -50.0), (3, 20, 500, 50, -80.0),
                (64, 512, 1024, 256, -120.0)]


def _random_peaks(rng, n, t_span, pow_lo=0.0):
    """Synthetic peak lists in (t, k) order, several peaks per frame, powers around the default floor."""
    t = np.sort(rng.integers(0, t_span, n))
    k = rng.integers(0, 512, n)
    order = np.lexsort((k, t))
    keep = np.ones(n, bool)
    tk = t[order] * 512 + k[order]
    keep[1:] = tk[1:] != tk[:-1]
    p = (10.0 ** rng.uniform(pow_lo - 2, pow_lo + 2, n)).astype(np.float32)
    return t[order][keep], k[order][keep], p[keep]


def test_walk_and_literal_readings_agree():
    rng = np.random.default_rng(1)
    fl = float(pr.floor_power(-50.0))
    total = 0
    for trial in range(40):
        cfg = pr.Cfg(int(rng.integers(1, 65)), int(rng.integers(1, 120)), int(rng.integers(1, 600)), 30, -50.0)
        t, k, p = _random_peaks(rng, int(rng.integers(0, 250)), int(rng.integers(1, 300)), np.log10(fl))
        a, b = pr.triplets(t, k, p, cfg), pr.triplets_literal(t, k, p, cfg)
        assert a.shape == b.shape and np.array_equal(a, b), (trial, cfg)
        total += a.shape[0]
    assert total > 5000


@pytest.mark.parametrize("cfg", WANG_CONFIGS)
def test_walk_without_triplets_is_wang(oracle, cfg):
    c = pr.Cfg(*cfg)
    for kind, seconds, seed in (("chirps", 6.0, 2), ("noise", 3.0, 5)):
        x = pr.signal(kind, seconds, seed)
        t, k, p = pr.peaks(oracle, x, c.peaks_per_sec)
        o = oracle.wang(x, oracle.WangCfg(*cfg), cap=400000)
        g = pr.wang_pairs(t, k, p, c)
        assert o.shape[0] > 100 and g.shape == o.shape and np.array_equal(g, o), (cfg, kind)


@pytest.mark.parametrize("cfg", [(5, 96, 96, 30, -50.0), (64, 512, 1024, 256, -120.0), (5, 3, 2, 30, -50.0),
                                 (11, 40, 30, 60, -70.0)])
def test_record_invariants(oracle, cfg):
    c = pr.Cfg(*cfg)
    saw_r31 = False
    for kind, seconds, seed in (("noise", 4.0, 1), ("chirps", 6.0, 3)):
        x = pr.signal(kind, seconds, seed)
        t, k, p = pr.peaks(oracle, x, c.peaks_per_sec)
        assert (k < 512).all() and (np.diff(t * 512 + k) > 0).all()
        per = []
        rec = pr.triplets(t, k, p, c, per).astype(np.int64)
        assert rec.shape[0] == sum(per) and max(per) <= c.fan_out
        assert rec.shape[0] <= pr.max_hashes(x.size, c)
        if cfg[1] >= 40:
            assert rec.shape[0] > 50
        h, ta, tb, tc = rec.T
        assert (ta < tb).all() and (tb <= tc).all() and (tc <= ta + c.target_zone_t).all()
        r = np.minimum(31, (32 * (tb - ta)) // (tc - ta))
        assert np.array_equal(h & 31, r)
        raw = (32 * (tb - ta)) // (tc - ta)
        assert (raw <= 32).all() and np.array_equal(raw == 32, tb == tc)   # the clamp is reached only when t_b = t_c
        ka, kb, kc = h >> 23, (h >> 14) & 511, (h >> 5) & 511
        assert (np.abs(kb - ka) <= c.target_zone_f).all() and (np.abs(kc - ka) <= c.target_zone_f).all()
        # hash >> 23 is the anchor's bin: every (t_a, k_a) is a peak above the floor, anchors in peak order
        anchors = np.repeat(np.arange(t.size), per)
        assert np.array_equal(ta, t[anchors]) and np.array_equal(ka, k[anchors])
        assert (p[anchors] >= pr.floor_power(c.min_anchor_mag_db)).all()
        if kind == "noise" and cfg[1] >= 40:
            saw_r31 = saw_r31 or bool(((h & 31) == 31).any())
    if cfg[1] >= 40:
        assert saw_r31                                             # r = 31 is present in the noise inputs


def test_widest_config_reaches_64_triplets(oracle):
    per = []
    pr.panako_ref(oracle, pr.signal("chirps", 6.0, 3), pr.Cfg(64, 512, 1024, 256, -120.0), per)
    assert max(per) == 64


def test_max_hashes_is_host_only():
    from ucfp_amd import _lib
    lib = _lib.load()
    cfg = _lib.PanakoConfig(5, 96, 96, 30, -50.0)
    assert lib.ucfp_audio_panako_max_hashes(80000, C.byref(cfg)) == 10 * 30 * 5
    assert lib.ucfp_audio_panako_max_hashes(80000, None) == 10 * 30 * 5          # NULL = the defaults
    assert lib.ucfp_audio_panako_max_hashes(1000, C.byref(cfg)) == 0             # shorter than one frame
    assert pr.max_hashes(80000, pr.Cfg()) == 1500 and pr.max_hashes(1000, pr.Cfg()) == 0
    assert lib.ucfp_audio_panako_batch_max_hashes(0, 0, 8000, None) == 0
    n = C.c_size_t(0)
    assert lib.ucfp_audio_panako(None, None, 0, 8000, None, None, 0, C.byref(n)) == -4


def test_host_mirror_defaults_and_projection():
    from ucfp_amd import audio
    from ucfp_amd.errors import ModalityError
    assert audio.ALGORITHM_PANAKO == "audiofp-panako-v1"
    c = audio.PanakoConfig()
    assert (c.fan_out, c.target_zone_t, c.target_zone_f, c.peaks_per_sec, c.min_anchor_mag_db) == pr.Cfg().astuple()
    rec = np.arange(24, dtype=np.uint32).reshape(6, 4)
    lm = audio.panako_landmarks(rec.tobytes())
    assert lm.dtype == np.uint32 and lm.shape == (6, 2) and np.array_equal(lm, rec[:, :2])
    assert np.array_equal(audio.panako_landmarks(rec), pr.landmarks(rec))
    assert audio.panako_landmarks(b"").shape == (0, 2)
    with pytest.raises(ModalityError):
        audio.panako_landmarks(b"\0" * 24)


def test_query_wire_format_with_algorithm():
    """A `landmarks` body with `algorithm` parses to the same landmarks and carries the tag; without it, as before."""
    from ucfp_amd.core import Modality, QueryRequest
    pairs = [[0x80402011, 7], [5, 125]]
    r = QueryRequest.from_json({"tenant_id": 1, "modality": "Audio", "k": 3, "landmarks": pairs,
                                "algorithm": "audiofp-panako-v1"})
    raw = np.array(pairs, np.uint32).tobytes()
    assert (r.tenant_id, r.modality, r.k, r.algorithm, r.landmarks) == (1, Modality.Audio, 3, "audiofp-panako-v1", raw)
    r2 = QueryRequest.from_json({"tenant_id": 1, "modality": "Audio", "landmarks": pairs})
    assert r2.algorithm is None and r2.landmarks == raw


@pytest.fixture(scope="module")
def corpus(oracle):
    return {100 + i: pr.panako_ref(oracle, pr.recording(i)) for i in range(pr.N_RECORDINGS)}


def test_identification_condition_holds_on_the_reference(oracle, corpus):
    """P7 with LandmarkRef alone: each of the 24 (recording, excerpt) cases is rank 1 with the exact offset; the
    generator's seeds are chosen so that this holds with a margin (the GPU test relies on it)."""
    ref = LandmarkRef({rid: pr.landmarks(rec) for rid, rec in corpus.items()})
    cases = 0
    for i in range(pr.N_RECORDINGS):
        x = pr.recording(i)
        for start_s, length_s in pr.EXCERPTS:
            q = pr.landmarks(pr.panako_ref(oracle, pr.excerpt(x, start_s, length_s)))
            hits = ref.query(q, 5)
            assert hits, (i, start_s)
            rid, votes, offset, score = hits[0]
            print(f"recording {i} start {start_s} s: votes {votes} of {q.shape[0]} share {score:.3f} "
                  f"runner-up {hits[1][1] if len(hits) > 1 else 0}")
            assert rid == 100 + i and offset == int(start_s * pr.FRAMES_PER_S), (i, start_s, hits[:2])
            assert score >= 0.5 and (len(hits) == 1 or votes >= 3 * hits[1][1]), (i, start_s, hits[:2])
            cases += 1
    assert cases == 24
