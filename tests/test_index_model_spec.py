"""CPU checks under the index lifecycle tests (tests/test_index_lifecycle_gpu.py).

1. The host model (tests/index_model.py) against expectations written out by hand and against a brute force over the
   operation log, on tiny cases.
2. The scenarios themselves: they are deterministic, reach the sizes their docstrings name, and aim their deletes at the
   rows they say.
3. For every cosine check of every scenario -- same builder, same seed, same sizes -- the float64 reference's own answer is
   fed back into its checker: the inputs alone stay inside MAX_EXEMPT_SHARE, so a GPU failure there is the GPU's."""
import numpy as np
import pytest

import test_index_lifecycle_gpu as life
from cosine_ref import CosineRef
from index_model import IndexModel
from test_index_gpu import COS_TOL


def brute_force(log, tenant):
    """{id: row} of a tenant from the whole operation log: every (id, row) pair in order, deletes as tombstones."""
    flat = [(t, int(i), r) for op, t, ids, rows in log for i, r in zip(ids, rows if op == "upsert" else [None] * len(ids))]
    last = {i: r for t, i, r in flat if t == tenant}
    return {i: r for i, r in last.items() if r is not None}


def as_dict(model, tenant):
    ids, rows = model.arrays(tenant)
    return {int(i): r.tolist() for i, r in zip(ids, rows)}


def test_model_tiny_cases_by_hand():
    m = IndexModel(np.uint64)
    m.upsert(1, [10, 11, 10], [100, 110, 101])                      # a duplicate id in a batch: the last one wins
    assert as_dict(m, 1) == {10: 101, 11: 110} and m.size(1) == 2 and m.device_order(1) == [11, 10]
    m.upsert(1, [12, 13], [120, 130])
    assert m.delete(1, [11]) == 1                                   # row 0 <- the last row (13)
    assert m.device_order(1) == [13, 10, 12]
    assert m.delete(1, [13]) == 1                                   # the moved row
    assert as_dict(m, 1) == {10: 101, 12: 120} and m.device_order(1) == [12, 10]
    assert m.delete(1, [99]) == 0 and m.delete(1, [10, 10]) == 1 and m.delete(2, [10]) == 0
    assert m.delete(1, [12, 10, 99]) == 1                           # everything
    assert m.size(1) == 0 and as_dict(m, 1) == {} and m.device_order(1) == []
    ids, rows = m.arrays(1)
    assert ids.shape == (0,) and ids.dtype == np.uint64 and rows.shape == (0,)
    m.upsert(1, [10], [7])                                          # re-upsert into the emptied tenant
    assert as_dict(m, 1) == {10: 7} and m.size(1) == 1 and m.size(3) == 0
    c = IndexModel(np.float32, (2,))
    c.upsert(0, [5, 5, 6], [[1, 2], [3, 4], [5, 6]])
    ids, rows = c.arrays(0)
    assert ids.tolist() == [5, 6] and rows.tolist() == [[3.0, 4.0], [5.0, 6.0]] and rows.dtype == np.float32
    assert c.arrays(9)[1].shape == (0, 2)


def test_model_against_brute_force_over_the_log():
    rng = np.random.default_rng(12)
    m, log = IndexModel(np.uint64), []
    for step in range(120):
        tenant = int(rng.integers(0, 2))
        ids = rng.integers(0, 25, int(rng.integers(1, 9))).astype(np.uint64)       # few ids: duplicates and repeats abound
        if rng.random() < 0.6:
            rows = rng.integers(0, 2**64, len(ids), dtype=np.uint64)
            m.upsert(tenant, ids, rows)
            log.append(("upsert", tenant, ids, rows))
        else:
            before = brute_force(log, tenant)
            log.append(("delete", tenant, ids, None))
            assert m.delete(tenant, ids) == len(before) - len(brute_force(log, tenant))
        for t in (0, 1):
            assert as_dict(m, t) == {i: int(r) for i, r in brute_force(log, t).items()}
            assert m.size(t) == len(brute_force(log, t)) and sorted(m.device_order(t)) == sorted(brute_force(log, t))


class Trace:
    """Sizes a scenario passes through and the notes of its checks."""
    def __init__(self):
        self.sizes, self.notes = {}, []

    def __call__(self, ix, model, tenant, queries, shapes, note):
        self.sizes.setdefault(tenant, []).append(model.size(tenant))
        self.notes.append(note)


@pytest.mark.parametrize("name", life.WALKS)
def test_walk_reaches_what_it_names(name):
    kit = life.kit_of(name)
    model, trace = kit.model(), Trace()
    events = []
    for ev in life.walk_events(kit, model, life.WALK_SEED[name]):
        events.append(ev[0])
        life.run_events([ev], model, None, trace)
    ops = sum(e != "check" for e in events)
    assert 55 <= ops <= 85, ops
    main, copies = trace.sizes[life.T_MAIN], trace.sizes[life.T_COPIES]
    for edge in (5, 1023, 1024, 1025, 2048, 2049, 4096, 4097):
        assert edge in main, edge
    assert max(main) <= 5000 and {1024, 1025, 2049, 0, 30} <= set(copies) and copies.count(0) >= 2
    for kind in ("last row", "middle row", "previous delete moved", "unknown id", "listed twice", "every row", "duplicate ids"):
        assert sum(kind in n for n in trace.notes) >= 2, kind
    if kit.dim:
        for kind in ("-> zeros", "-> NaN", "zero row -> vector", "planted last row"):
            assert any(kind in n for n in trace.notes), kind
    again = kit.model()
    life.run_events(life.walk_events(kit, again, life.WALK_SEED[name]), again, None, None)
    for t in (life.T_MAIN, life.T_COPIES):                                         # deterministic
        assert np.array_equal(again.arrays(t)[0], model.arrays(t)[0])
        assert np.array_equal(again.arrays(t)[1], model.arrays(t)[1], equal_nan=True)


def test_hamming_scenarios_land_where_they_say():
    model, trace = IndexModel(np.uint64), Trace()
    life.run_events(life.hamming_growth_events(), model, None, trace)
    assert tuple(dict.fromkeys(trace.sizes[0])) == life.HAMMING_LANDINGS
    model, trace = IndexModel(np.uint64), Trace()
    life.run_events(life.hamming_reuse_events(model), model, None, trace)
    assert tuple(dict.fromkeys(trace.sizes[0])) == (300_000, 262_143, 271_143)
    assert len(trace.notes) == 2 * (10 + 10 + 4)
    assert life.big_batch_rows(4097).tolist() == list(range(64)) + list(range(4032, 4097))
    assert life.big_batch_rows(4096).tolist() == list(range(64)) + list(range(4032, 4096))
    assert len(life.big_batch_rows(9000)) == 256


def reference_alone(ix, model, tenant, queries, shapes, note):
    """The reference's answer through the reference's checker: only the cap on exempt places can fail."""
    ids, rows = model.arrays(tenant)
    ref = CosineRef(ids, rows, queries, max(k for _, k in shapes))
    for nq, k in shapes:
        g_ids, g_sc, g_c = ref.answer(k)
        assert ref.check(g_ids[:nq], g_sc[:nq], g_c[:nq], k, COS_TOL) <= 1e-7, (note, nq, k)


@pytest.mark.parametrize("name", [w for w in life.WALKS if w != "hamming"])
def test_cosine_walk_and_snapshot_inputs_stay_inside_the_exempt_share(name):
    kit = life.kit_of(name)
    model = kit.model()
    life.run_events(life.walk_events(kit, model, life.WALK_SEED[name]), model, None, reference_alone)
    before, prepop, rng = life.snapshot_events(kit, model, life.WALK_SEED[name] + 1)       # (the order of the GPU test)
    life.run_events(before, model, None, None)
    life.run_events(life.snapshot_checks(kit, model, rng, "fresh"), model, None, reference_alone)
    other = kit.model()
    life.run_events(prepop, other, None, None)
    life.replay_file_into(model, other)
    n_main = model.size(life.T_MAIN)
    assert other.size(life.T_MAIN) == n_main + 300 and other.size(life.T_EMPTIED) == 1 and model.size(life.T_EMPTIED) == 0
    life.run_events(life.snapshot_checks(kit, other, rng, "other"), other, None, reference_alone)
    life.run_events(life.snapshot_checks(kit, model, rng, "source"), model, None, reference_alone)


def test_cosine_growth_inputs_stay_inside_the_exempt_share():
    model = IndexModel(np.float32, (life.COSINE_GROWTH_DIM,))
    events = (ev for ev in life.cosine_growth_events() if len(ev) < 6)              # (the repeats share inputs and reference)
    life.run_events(events, model, None, reference_alone)
    assert model.size(0) == 262_145
    assert {q for s in life.COSINE_LANDINGS.values() for q, _ in s} == {1, 3, 5, 48, 49, 64, 65, 300}
    assert {k for s in life.COSINE_LANDINGS.values() for _, k in s} == {1, 10, 64, 65}


def test_cosine_stream_inputs_stay_inside_the_exempt_share():
    ids, rows, blocks, queries = life.stream_case(life.CosineKit(64), 6464)
    assert blocks == ((0, 3000), (3000, 5000)) and (np.diff(ids.astype(np.int64)) > 0).all()
    for _, n in blocks:
        ref = CosineRef(ids[:n], rows[:n], queries, life.STREAM_K)
        ref.check(*ref.answer(life.STREAM_K), life.STREAM_K, COS_TOL)
    h_ids, codes, h_blocks, h_q = life.stream_case(life.HammingKit(), 5150)
    assert h_blocks == ((0, 200_000), (200_000, 300_000)) and (np.diff(h_ids.astype(np.int64)) > 0).all() and len(h_q) == 64
    assert len(np.unique(codes)) == 40


@pytest.mark.parametrize("dim,n", [(100, 50), (64, 1020), (64, 2049)])
def test_reference_gives_bit_identical_rows_one_score(dim, n):
    """A matrix product may round the dots of two copies of a row differently; the reference must still order copies by id
    alone and give them one score (a shard of copies is what the lifecycle walks keep in tenant 9)."""
    kit = life.CosineKit(dim)
    rng = np.random.default_rng(dim + n)
    rows = kit.new_rows(rng, n, True)
    ids = rng.permutation(n).astype(np.uint64) * np.uint64(5) + np.uint64(11)
    ref = CosineRef(ids, rows, rng.standard_normal((20, dim), dtype=np.float32), 128)
    for order, sc in ref.best:
        groups = {}
        for r, s in zip(order, sc):
            groups.setdefault(rows[r].tobytes(), []).append((int(ids[r]), s))
        for hits in groups.values():
            assert len({s for _, s in hits}) == 1 and [i for i, _ in hits] == sorted(i for i, _ in hits)
        assert (np.diff(sc) <= 0).all()
    ref.check(*ref.answer(128), 128, COS_TOL)
