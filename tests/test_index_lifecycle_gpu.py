"""One DeviceIndex kept alive through growth, overwrites, deletes and changing search shapes, against the host model.

Every scenario is a generator of events -- ("upsert", tenant, ids, rows), ("delete", tenant, ids),
("check", tenant, queries, ((nq, k), ...)) -- driven by `run_events`, which applies each mutation to the model
(tests/index_model.py) and to the index and answers each check from the project's references over the model:
oracle.hamming_topk bit-exactly, cosine_ref.CosineRef.check within COS_TOL.  The scenario builders touch no GPU, so
tests/test_index_model_spec.py replays the same events (same seeds, same sizes) on the CPU.

Which branch a size reaches is read from the code (index.hip shard_reserve / search_shard_dev, hamming.hip hamming_plan /
few_queries, hamming_direct_ok, cosine.hip cosine_*_ok), not observed through a counter: the index exports none."""
import os
import struct

import numpy as np
import pytest

from cosine_ref import CosineRef
from index_model import IndexModel
from test_index_gpu import COS_TOL

pytestmark = pytest.mark.gpu


# =====================================================================================================================
# driver
# =====================================================================================================================
def big_batch_rows(nq):
    """The queries of a > 4000-query batch that are compared: the first 64, the last 64 and the 128 around the chunk seam
    (kHammingMaxBatch = 4096), as far as the batch has them."""
    rows = np.r_[0:64, 4096 - 64:min(4096 + 64, nq), nq - 64:nq]
    return np.unique(rows[(rows >= 0) & (rows < nq)])


def hamming_window(queries, j, nq):
    """The nq queries the j-th shape of a check takes out of the check's pool: a different window per shape."""
    off = (37 * j) % (len(queries) - nq + 1)
    return queries[off:off + nq]


class HammingChecker:
    def __init__(self, oracle):
        self.oracle = oracle

    def __call__(self, ix, model, tenant, queries, shapes, note):
        ids, codes = model.arrays(tenant)
        assert ix.size(tenant) == len(ids), note
        for j, (nq, k) in enumerate(shapes):
            q = hamming_window(queries, j, nq)
            g_ids, g_sc, g_d, g_c = ix.search(tenant, q, k)
            rows = big_batch_rows(nq) if nq > 4000 else np.arange(nq)
            o_ids, o_d, o_c = self.oracle.hamming_topk(ids, codes, q[rows], k)
            what = (note, len(ids), nq, k)
            assert np.array_equal(g_c[rows], o_c), what
            assert np.array_equal(g_d[rows], o_d), what
            assert np.array_equal(g_ids[rows], o_ids), what
            hit = g_d[rows] != 0xFFFFFFFF
            assert np.array_equal(g_sc[rows][hit], (1.0 - g_d[rows][hit] / 64.0).astype(np.float32)), what


_last_ref = [None] * 5


def cosine_checker(ix, model, tenant, queries, shapes, note):
    """One float64 reference per check; every (nq, k) of it searches the first nq queries."""
    ids, rows = model.arrays(tenant)
    assert ix.size(tenant) == len(ids), note
    kmax = max(k for _, k in shapes)
    key = (queries, ids, rows, kmax)
    if not all(a is b for a, b in zip(_last_ref[:4], key)):   # (a check repeated under another switch shares the reference)
        _last_ref[:] = list(key) + [CosineRef(ids, rows, queries, kmax)]
    ref = _last_ref[4]
    for nq, k in shapes:
        g_ids, g_sc, _, g_c = ix.search(tenant, queries[:nq], k)
        try:
            ref.check(g_ids, g_sc, g_c, k, COS_TOL)
        except AssertionError as e:
            raise AssertionError((note, len(ids), nq, k) + e.args) from None


def run_events(events, model, ix, checker):
    """Applies a scenario to the model and (when given) the index; `checker` answers the checks.  A delete must report the
    model's count."""
    for ev in events:
        if ev[0] == "upsert":
            _, tenant, ids, rows = ev
            model.upsert(tenant, ids, rows)
            if ix is not None:
                ix.upsert(tenant, ids, rows)
        elif ev[0] == "delete":
            _, tenant, ids = ev
            want = model.delete(tenant, ids)
            if ix is not None:
                assert ix.delete(tenant, ids) == want, (tenant, want)
        else:
            _, tenant, queries, shapes, note = ev[:5]
            if checker is None:
                continue
            env = ev[5] if len(ev) > 5 else {}       # switches the library already reads at every search
            os.environ.update(env)
            try:
                checker(ix, model, tenant, queries, shapes, note)
            finally:
                for name in env:
                    del os.environ[name]


# =====================================================================================================================
# rows and queries
# =====================================================================================================================
def flip_bits(rng, codes):
    """Each code with 0 .. 8 random bits flipped."""
    out = np.array(codes, dtype=np.uint64)
    for j in range(out.size):
        m = 0
        for b in rng.choice(64, size=int(rng.integers(0, 9)), replace=False):
            m |= 1 << int(b)
        out[j] ^= np.uint64(m)
    return out


class HammingKit:
    """Rows and queries of the Hamming scenarios.  Tenant COPIES holds copies of one code (and, after overwrites, of a
    second one two bits away): every distance ties and the id order alone decides."""
    kind_name, dim = "HAMMING64", 0
    CODE, CODE2 = np.uint64(0x5DEECE66D1234567), np.uint64(0x5DEECE66D1234567 ^ 0b11)

    def model(self):
        return IndexModel(np.uint64)

    def new_rows(self, rng, m, copies):
        if copies:
            return np.full(m, self.CODE, np.uint64)
        return rng.integers(0, 2**64, m, dtype=np.uint64)

    def changed_rows(self, rng, m, copies):
        return np.full(m, self.CODE2, np.uint64) if copies else self.new_rows(rng, m, False)

    def queries(self, rng, model, tenant, probes, nq):
        ids, codes = model.arrays(tenant)
        src = [np.asarray(probes, dtype=np.uint64).reshape(-1)[:nq]]
        if len(ids):
            src.append(codes[rng.integers(0, len(ids), max(0, (nq - src[0].size + 1) // 2))])
        near = flip_bits(rng, np.concatenate(src)[:nq])
        return np.concatenate([near, rng.integers(0, 2**64, nq - near.size, dtype=np.uint64)])

    def special(self, rng, model, tenant, fresh, probe):
        return iter(())


class CosineKit:
    """Rows and queries of the cosine scenarios, with cosine_ref.make_case's plants: bit-identical copies, zero rows, rows
    with a NaN or an Inf component.  Row lengths spread over 2^-2 .. 2^2, so a norm that stayed behind when its row
    moved, or was not carried into a grown buffer, changes the score by far more than the tolerance."""
    kind_name = "COSINE_F32"

    def __init__(self, dim):
        self.dim = dim
        self.bases = np.random.default_rng(1000 + dim).standard_normal((6, dim), dtype=np.float32)

    def model(self):
        return IndexModel(np.float32, (self.dim,))

    def new_rows(self, rng, m, copies):
        if copies:
            return self.bases[rng.integers(0, 5, m)]                    # (base 5 enters with the overwrites)
        rows = rng.standard_normal((m, self.dim), dtype=np.float32)
        rows *= np.exp2(rng.uniform(-2, 2, (m, 1))).astype(np.float32)
        if m >= 8:
            p = rng.permutation(m)
            rows[p[1:4]] = rows[p[0]]                                    # four bit-identical copies
            rows[p[4]] = 0.0
            if m >= 64:
                rows[p[5], int(rng.integers(0, self.dim))] = np.nan
                rows[p[6]] = np.inf
                rows[p[7:7 + m // 64]] = 0.0
        return rows

    def changed_rows(self, rng, m, copies):
        return np.repeat(self.bases[5:6], m, axis=0) if copies else self.new_rows(rng, m, False)

    def queries(self, rng, model, tenant, probes, nq):
        """Probes first (the first one scaled by 3: score 1; the others with a little noise), then neighbours of stored
        rows, a zero query, and free directions."""
        ids, rows = model.arrays(tenant)
        q = rng.standard_normal((nq, self.dim), dtype=np.float32)
        src = [np.asarray(p, dtype=np.float32) for p in probes][:nq]
        if len(ids):
            src += list(rows[rng.integers(0, len(ids), max(0, (nq - len(src) + 1) // 2))])
        src = [s for s in src[:nq] if np.isfinite(s).all() and np.any(s != 0)]
        for j, s in enumerate(src):
            q[j] = s * np.float32(3.0) if j == 0 else s + np.float32(0.05) * np.abs(s).max() * q[j]
        if nq >= 9:
            q[nq - 1] = 0.0
        return q

    def special(self, rng, model, tenant, fresh, probe):
        """The cosine-only steps of the walk: a scorable row overwritten with zeros and with a NaN component must leave
        every answer, a zero row overwritten with a vector must enter, and a planted best row that a delete moves must
        keep its norm (16 times the norm of the row whose place it takes)."""
        ids, rows = model.arrays(tenant)
        good = [int(i) for i, r in zip(ids, rows) if np.isfinite(r).all() and np.any(r != 0)]
        a, b = good[len(good) // 3], good[2 * len(good) // 3]
        old_a, old_b = model.row(tenant, a).copy(), model.row(tenant, b).copy()
        yield ("upsert", tenant, np.array([a], np.uint64), np.zeros((1, self.dim), np.float32))
        yield probe(tenant, [old_a], "scorable row -> zeros")
        nan_row = old_b.copy()
        nan_row[int(rng.integers(0, self.dim))] = np.nan
        yield ("upsert", tenant, np.array([b], np.uint64), nan_row[None])
        yield probe(tenant, [old_b, old_a], "scorable row -> NaN component")
        v = rng.standard_normal((1, self.dim), dtype=np.float32) * np.float32(0.5)
        yield ("upsert", tenant, np.array([a], np.uint64), v)
        yield probe(tenant, [v[0], old_b], "zero row -> vector")
        planted = rng.standard_normal((1, self.dim), dtype=np.float32)
        planted *= np.float32(16.0 / np.linalg.norm(planted))
        small = planted * np.float32(1.0 / 16.0) + rng.standard_normal((1, self.dim), dtype=np.float32) * np.float32(0.3)
        hole, last = fresh(2)
        yield ("upsert", tenant, np.array([hole], np.uint64), small)
        yield ("upsert", tenant, np.array(fresh(3), np.uint64), self.new_rows(rng, 3, False))
        yield ("upsert", tenant, np.array([last], np.uint64), planted)
        assert model.device_order(tenant)[-1] == last
        yield ("delete", tenant, np.array([hole], np.uint64))
        yield probe(tenant, [planted[0], small[0]], "planted last row moved by a delete")


# =====================================================================================================================
# scenario (c) / (d): the mutation walk
# =====================================================================================================================
WALK_SHAPES = ((1, 10), (9, 10), (70, 128))
T_MAIN, T_COPIES = 5, 9


def walk_events(kit, model, seed):
    """About sixty operations on two tenants whose sizes cross the 1024 / 2048 / 4096 capacity edges (n <= 5000), a check
    after each: upserts of new ids, overwrites with a duplicate id inside the batch (the probes hold the first AND the last
    occurrence's row), deletes of the last row, a middle row, the row the previous delete moved, an unknown id, one id
    listed twice, every row of a tenant, and re-upserts into the emptied tenant."""
    rng = np.random.default_rng(seed)
    pool = (rng.permutation(40_000).astype(np.uint64) * np.uint64(5) + np.uint64(11)).tolist()
    step = [0]

    def fresh(m):
        out, pool[:] = pool[:m], pool[m:]
        return out

    def probe(tenant, probes, note):
        nq, k = WALK_SHAPES[step[0] % 3]
        step[0] += 1
        return ("check", tenant, kit.queries(rng, model, tenant, probes, nq), ((nq, k),), note)

    def tail_rows(tenant, m=2):
        return [model.row(tenant, i) for i in model.device_order(tenant)[-m:]]

    def up_new(tenant, m):
        rows = kit.new_rows(rng, m, tenant == T_COPIES)
        yield ("upsert", tenant, np.array(fresh(m), np.uint64), rows)
        yield probe(tenant, list(rows[-3:]), "upsert of %d new ids" % m)

    def up_to(tenant, n):
        yield from up_new(tenant, n - model.size(tenant))

    def overwrite(tenant, m):
        order = model.device_order(tenant)
        pick = [order[int(j)] for j in rng.choice(len(order), size=min(m, len(order)), replace=False)]
        ids = pick + [pick[0], pick[-1]]                                 # two ids twice in the batch
        rows = kit.changed_rows(rng, len(ids), tenant == T_COPIES)
        if tenant != T_COPIES:
            assert not np.array_equal(rows[0], rows[-2], equal_nan=True)
        yield ("upsert", tenant, np.array(ids, np.uint64), rows)
        yield probe(tenant, [rows[-2], rows[0], rows[-1], rows[len(pick) - 1]], "overwrite, duplicate ids in the batch")

    def delete(tenant, ids, note):
        gone = [model.row(tenant, i) for i in ids if i in model.tenants.get(tenant, {})][:3]
        probes = gone + tail_rows(tenant)
        yield ("delete", tenant, np.array(ids, np.uint64))
        yield probe(tenant, probes, note)

    def delete_last(tenant):
        yield from delete(tenant, [model.device_order(tenant)[-1]], "delete of the last row")

    def delete_middle_then_moved(tenant):
        order = model.device_order(tenant)
        at = len(order) // 2
        mid, last = order[at], order[-1]
        yield from delete(tenant, [mid], "delete of a middle row")
        assert model.device_order(tenant)[at] == last
        yield from delete(tenant, [last], "delete of the row the previous delete moved")

    def delete_odd(tenant):
        yield from delete(tenant, [3], "delete of an unknown id")
        x = model.device_order(tenant)[model.size(tenant) // 4]
        yield from delete(tenant, [x, x], "delete of one id listed twice")

    def delete_many(tenant, m):
        order = model.device_order(tenant)
        ids = [order[int(j)] for j in rng.choice(len(order), size=m, replace=False)]
        ids += [ids[0], 7, order[-1]]
        yield from delete(tenant, ids, "delete of %d rows, a repeat and an unknown id among them" % m)

    def delete_all(tenant):
        ids = list(model.device_order(tenant))
        rng.shuffle(ids)
        yield from delete(tenant, ids, "delete of every row")
        yield probe(T_MAIN if tenant == T_COPIES else T_COPIES, [], "the other tenant after that")

    yield from up_new(T_MAIN, 5)                      # k > n
    yield from up_to(T_MAIN, 1000)
    yield from up_new(T_COPIES, 1020)
    for n in (1023, 1024, 1025):                      # 1025: first doubling
        yield from up_to(T_MAIN, n)
    yield from up_to(T_COPIES, 1024)
    yield from up_to(T_COPIES, 1025)
    yield from overwrite(T_MAIN, 40)
    yield from delete_last(T_MAIN)
    yield from delete_middle_then_moved(T_MAIN)
    yield from delete_odd(T_MAIN)
    yield from kit.special(rng, model, T_MAIN, fresh, probe)
    yield from overwrite(T_COPIES, 30)
    yield from delete_middle_then_moved(T_COPIES)
    yield from up_to(T_MAIN, 2048)
    yield from up_to(T_MAIN, 2049)                    # second doubling
    yield from delete_all(T_COPIES)
    yield from up_new(T_COPIES, 30)                   # re-upsert into the emptied tenant; k = 128 > n
    yield from delete_many(T_MAIN, 600)
    yield from up_to(T_MAIN, 4096)
    yield from up_to(T_MAIN, 4097)                    # third doubling
    yield from up_to(T_COPIES, 2049)
    for _ in range(26):
        tenant = T_MAIN if rng.random() < 0.6 else T_COPIES
        op = int(rng.integers(0, 7))
        if model.size(tenant) > 4700:
            yield from delete_many(tenant, 900)
        elif op == 0 or model.size(tenant) < 8:
            yield from up_new(tenant, int(rng.integers(1, 300)))
        elif op == 1:
            yield from overwrite(tenant, int(rng.integers(1, 60)))
        elif op == 2:
            yield from delete_last(tenant)
        elif op == 3:
            yield from delete_middle_then_moved(tenant)
        elif op == 4:
            yield from delete_odd(tenant)
        elif op == 5:
            yield from delete_many(tenant, int(rng.integers(1, min(200, model.size(tenant)))))
        else:
            yield from up_new(tenant, int(rng.integers(1, 40)))
    yield from delete_all(T_COPIES)
    yield from up_new(T_COPIES, 1030)


def kit_of(name):
    return HammingKit() if name == "hamming" else CosineKit(int(name[len("cosine"):]))


WALKS = ("hamming", "cosine64", "cosine100")
WALK_SEED = {"hamming": 31, "cosine64": 64, "cosine100": 100}


def open_index(kit, gpu_ctx, flags=0):
    from ucfp_amd import index
    return index.DeviceIndex(getattr(index, kit.kind_name), kit.dim, flags, gpu_ctx)


def checker_of(kit, oracle):
    return HammingChecker(oracle) if kit.dim == 0 else cosine_checker


@pytest.mark.parametrize("name", WALKS)
def test_mutation_walk(gpu_ctx, oracle, name):
    """(c), (d) -- capacity doublings 1024 -> 2048 -> 4096 -> 8192 in tenant 5 and 1024 -> 2048 -> 4096 in tenant 9 with old rows
    probed after each; Hamming shapes (1, 10) single launch, (9, 10) and (70, 128) robust tier (n < 2^18), both slots in
    turn; cosine: dim 64 (GEMM for 70 queries, LDS-resident kernel below, select_pruned for few), dim 100 (no GEMM:
    100 % 32 != 0), slot 0; the empty-shard branch of both kinds."""
    kit = kit_of(name)
    model, ix = kit.model(), open_index(kit, gpu_ctx)
    run_events(walk_events(kit, model, WALK_SEED[name]), model, ix, checker_of(kit, oracle))
    ix.close()


# =====================================================================================================================
# scenario (f): snapshot against the reference
# =====================================================================================================================
T_EMPTIED, T_ONLY_THERE = 77, 78


def snapshot_events(kit, model_saved, seed):
    """-> (events for the walked index before `save`, events that fill the second index before `load`, the generator the
    checks after it go on drawing from).  Before the save a tenant is filled and emptied again.  The second index holds, per walked tenant, a quarter of the
    saved ids under OTHER rows plus ids of its own, and one tenant the file does not have."""
    rng = np.random.default_rng(seed)
    before = [("upsert", T_EMPTIED, np.arange(10, dtype=np.uint64) + np.uint64(1), kit.new_rows(rng, 10, False)),
              ("delete", T_EMPTIED, np.arange(10, dtype=np.uint64) + np.uint64(1))]
    prepop = []
    for tenant in (T_MAIN, T_COPIES):
        ids, _ = model_saved.arrays(tenant)
        both = ids[rng.permutation(len(ids))[:len(ids) // 4]]
        own = np.arange(300, dtype=np.uint64) * np.uint64(5) + np.uint64(1_000_002)     # (walk ids are 1 mod 5)
        rows = np.concatenate([kit.changed_rows(rng, len(both), False), kit.new_rows(rng, 300, False)])
        prepop.append(("upsert", tenant, np.concatenate([both, own]), rows))
    prepop.append(("upsert", T_ONLY_THERE, np.arange(7, dtype=np.uint64), kit.new_rows(rng, 7, False)))
    prepop.append(("upsert", T_EMPTIED, np.array([4], np.uint64), kit.new_rows(rng, 1, False)))
    return before, prepop, rng


def snapshot_checks(kit, model, rng, note):
    for tenant in (T_MAIN, T_COPIES, T_EMPTIED, T_ONLY_THERE):
        ids, rows = model.arrays(tenant)
        probes = list(rows[rng.integers(0, len(ids), 6)]) if len(ids) else []
        yield ("check", tenant, kit.queries(rng, model, tenant, probes, 70), ((70, 128), (9, 10), (1, 10)), note)


def replay_file_into(model_saved, model_other):
    """`load` upserts every tenant of the file: ids present in both take the file's rows, the others stay."""
    for tenant in model_saved.tenants:
        ids, rows = model_saved.arrays(tenant)
        if len(ids):
            model_other.upsert(tenant, ids, rows)


def snapshot_tenants(path):
    """Tenant numbers in a snapshot file (index.hip: "UCFPIDX1" | kind | dim | row_bytes u64 | tenants | 0 | per tenant ...)."""
    with open(path, "rb") as f:
        blob = f.read()
    assert blob[:8] == b"UCFPIDX1"
    _, _, row_bytes, tenants, _ = struct.unpack_from("<IIQII", blob, 8)
    at, out = 32, []
    for _ in range(tenants):
        tenant, _, n = struct.unpack_from("<IIQ", blob, at)
        out.append(tenant)
        at += 16 + n * (8 + row_bytes)
    assert at == len(blob)
    return out


@pytest.mark.parametrize("name", WALKS)
def test_snapshot_after_walk_against_reference(gpu_ctx, oracle, tmp_path, name):
    """(f) -- the walked index (rows moved by deletes, overwritten rows, grown buffers) is saved; a fresh index loaded from the
    file, and a non-empty one, answer like the REFERENCE over the model, not like the source index."""
    kit = kit_of(name)
    checker = checker_of(kit, oracle)
    model, ix = kit.model(), open_index(kit, gpu_ctx)
    run_events(walk_events(kit, model, WALK_SEED[name]), model, ix, None)
    before, prepop, rng = snapshot_events(kit, model, WALK_SEED[name] + 1)
    run_events(before, model, ix, None)
    path = tmp_path / "walked.idx"
    ix.save(path)
    assert model.size(T_EMPTIED) == 0 and sorted(snapshot_tenants(path)) == sorted(t for t in model.tenants if model.size(t))
    fresh = open_index(kit, gpu_ctx)
    fresh.load(path)
    run_events(snapshot_checks(kit, model, rng, "fresh index after load"), model, fresh, checker)
    assert fresh.size(T_EMPTIED) == 0
    fresh.close()
    other_model, other = kit.model(), open_index(kit, gpu_ctx)
    run_events(prepop, other_model, other, None)
    other.load(path)
    replay_file_into(model, other_model)
    assert other_model.size(T_EMPTIED) == 1 and other_model.size(T_ONLY_THERE) == 7
    run_events(snapshot_checks(kit, other_model, rng, "non-empty index after load"), other_model, other, checker)
    run_events(snapshot_checks(kit, model, rng, "source index after save"), model, ix, checker)
    other.close()
    ix.close()


# =====================================================================================================================
# scenario (a) / (b): a Hamming shard through every capacity and plan edge; workspace reuse
# =====================================================================================================================
HAMMING_LANDINGS = (1, 1023, 1024, 1025, 2048, 2049, 4097, 65_537, 262_143, 262_144, 262_145, 300_000)
HAMMING_SHAPES = ((1, 10), (8, 32), (8, 33), (9, 10), (64, 128), (65, 65), (256, 16), (257, 16), (300, 64))
OLDEST = 1023        # rows placed before the first doubling: copied by every one of them


def hamming_corpus(seed, n):
    """Random codes under shuffled ids; three thousand later rows are near neighbours of the oldest rows, so the answers
    about an old row mix rows of many batches and tie on distance."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 2**64, n, dtype=np.uint64)
    ids = rng.permutation(n).astype(np.uint64) * np.uint64(7) + np.uint64(3)
    late = rng.integers(OLDEST, n, 3000)
    codes[late] = flip_bits(rng, codes[rng.integers(0, OLDEST, 3000)])
    return rng, ids, codes


def hamming_growth_queries(rng, codes, n0, n, nq):
    """Near neighbours (0 .. 8 bits) of the oldest rows -- row 0, the first batch, first -- and of the newest batch
    [n0, n), then free codes."""
    a = nq // 3
    src = np.concatenate([[0], rng.integers(0, min(n, OLDEST), a), rng.integers(n0, n, a)])
    near = flip_bits(rng, codes[src])
    q = np.concatenate([near, rng.integers(0, 2**64, max(0, nq - near.size), dtype=np.uint64)])[:nq]
    return np.concatenate([q[:1], rng.permutation(q[1:])])


def hamming_growth_events(seed=2026):
    rng, ids, codes = hamming_corpus(seed, HAMMING_LANDINGS[-1])
    n0 = 0
    for n in HAMMING_LANDINGS:
        yield ("upsert", 0, ids[n0:n], codes[n0:n])
        yield ("check", 0, hamming_growth_queries(rng, codes, n0, n, 420), HAMMING_SHAPES, "landing %d" % n)
        n0 = n
    yield ("check", 0, hamming_growth_queries(rng, codes, 0, n0, 4097), ((4097, 10),), "landing 300000, two chunks")


def test_hamming_shard_grows_through_capacity_and_plan_edges(gpu_ctx, oracle):
    """(a) -- capacities 1024, 2048, 4096, 8192, 131 072, 262 144, 524 288 (seven allocations, the last on 262 145) with rows
    of the first allocation queried after each.  Plans, per landing, all nine shapes: (1, 10), (8, 32) single launch;
    (8, 33) first shape outside it (lane scan); n < 2^18: robust tier, cap 24 / 64 / 160 by k; n >= 2^18: (8, 33) lanes
    (few_queries drops from 64 to 8 queries), the others the matrix filter -- (9, 10), (256, 16) bound + short chain + fused
    thresholds, (257, 16) bound without either, (300, 64) bound, (64, 128) and (65, 65) no bound pass.  The searches
    alternate between the two slots; 4097 queries are a chunk of 4096 and a tail of one with its own plan (lanes)."""
    from ucfp_amd import index
    model, ix = IndexModel(np.uint64), index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    run_events(hamming_growth_events(), model, ix, HammingChecker(oracle))
    ix.close()


REUSE_SHAPES = ((4097, 10), (1, 10), (300, 64), (8, 32), (9, 33), (64, 128), (65, 65), (1, 32), (4096, 1), (5, 10))


def reuse_round(rng, codes, n0, n, shapes, note):
    """Each shape twice in a row, with different queries: searches alternate between the two slots, so each slot meets each
    shape behind a different one -- and a launch that wrote nothing cannot pass on what the first issue left behind."""
    for nq, k in shapes:
        for issue in (0, 1):
            yield ("check", 0, hamming_growth_queries(rng, codes, n0, n, nq), ((nq, k),), "%s, issue %d" % (note, issue))


def hamming_reuse_events(model, seed=4242):
    rng, ids, codes = hamming_corpus(seed, 300_000)
    for a, b in ((0, 100_000), (100_000, 200_000), (200_000, 300_000)):
        yield ("upsert", 0, ids[a:b], codes[a:b])
    yield from reuse_round(rng, codes, 200_000, 300_000, REUSE_SHAPES, "300 000 rows")
    # down to 2^18 - 1 rows: a hundred from the middle (each moves the last row into the hole), the others from the end
    order = model.device_order(0)
    middle = [order[int(j)] for j in rng.choice(200_000, size=100, replace=False)]
    yield ("delete", 0, np.array(middle, np.uint64))
    tail = model.device_order(0)[262_143:][::-1]
    yield ("delete", 0, np.array(tail, np.uint64))
    yield from reuse_round(rng, codes, 200_000, 300_000, REUSE_SHAPES, "262 143 rows behind 300 000")   # (about deleted rows too)
    more = np.arange(9000, dtype=np.uint64) * np.uint64(7) + np.uint64(4)       # (the corpus ids are 3 mod 7)
    more_codes = flip_bits(rng, codes[rng.integers(0, OLDEST, 9000)])
    yield ("upsert", 0, more, more_codes)
    yield from reuse_round(rng, np.concatenate([codes[:OLDEST], more_codes]), OLDEST, OLDEST + 9000, REUSE_SHAPES[:4],
                           "271 143 rows behind 262 143")


def test_hamming_workspace_reuse_across_plans(gpu_ctx, oracle):
    """(b) -- both ws_slot / direct_state pairs see the sequence of plans twice over: matrix tier (300 000 rows), robust
    tier behind it in the same slots (262 143 rows: the workspace is not re-allocated, the layout changes), matrix tier
    again (271 143 rows).  Single launches ((1, 10), (8, 32), (1, 32), (5, 10)) run between staged searches in the same slot,
    so their ticket and histogram must have been left at zero."""
    from ucfp_amd import index
    model, ix = IndexModel(np.uint64), index.DeviceIndex(index.HAMMING64, ctx=gpu_ctx)
    run_events(hamming_reuse_events(model), model, ix, HammingChecker(oracle))
    assert model.size(0) == 271_143
    ix.close()


# =====================================================================================================================
# scenario (d), second half: a cosine shard grows through the doublings and the 2^17 / 2^18 pass switches
# =====================================================================================================================
COSINE_GROWTH_DIM = 64
COSINE_LANDINGS = {      # n -> the (nq, k) searched there
    1024: ((1, 1), (5, 10), (48, 64), (300, 65)),
    1025: ((3, 10), (49, 1), (64, 65), (65, 64)),
    2049: ((1, 65), (5, 64), (65, 10), (300, 1)),
    131_071: ((3, 10), (48, 64), (49, 10), (64, 1), (65, 65)),
    131_073: ((1, 10), (3, 64), (5, 1), (48, 10), (49, 64), (64, 10), (5, 65), (65, 64), (65, 10)),
    262_143: ((3, 1), (48, 10), (49, 65), (64, 10), (64, 64), (65, 65)),
    262_145: ((1, 1), (5, 10), (48, 64), (49, 65), (64, 10), (65, 65), (300, 10), (300, 64)),
}
NO_F16 = {"UCFP_COSINE_NO_F16": "1"}     # (an existing switch, read at every search: the passes the f16 minima pre-empt at dim 64)


def cosine_growth_events(seed=640):
    kit = CosineKit(COSINE_GROWTH_DIM)
    rng = np.random.default_rng(seed)
    n_all = max(COSINE_LANDINGS)
    ids = rng.permutation(n_all).astype(np.uint64) * np.uint64(3) + np.uint64(5)
    rows = rng.standard_normal((n_all, kit.dim), dtype=np.float32)
    rows *= np.exp2(rng.uniform(-2, 2, (n_all, 1))).astype(np.float32)
    for lo, hi in ((0, 1024), (1025, 2049), (2049, 131_071), (131_073, 262_143)):      # plants in old and in late batches
        p = rng.integers(lo, hi, 12)
        rows[p[1:4]] = rows[p[0]]
        rows[p[4:7]] = 0.0
        rows[p[7], int(rng.integers(0, kit.dim))] = np.nan
        rows[p[8]] = np.inf
        rows[p[9:12]] = rows[rng.integers(0, 1024, 3)]                                   # late copies of the oldest rows
    n0 = 0
    for n, shapes in COSINE_LANDINGS.items():
        yield ("upsert", 0, ids[n0:n], rows[n0:n])
        nq = max(q for q, _ in shapes)
        old = rows[rng.integers(0, 1024, (nq + 2) // 3)]
        new = rows[rng.integers(n0, n, (nq + 2) // 3)]
        src = [s for s in np.concatenate([old, new]) if np.isfinite(s).all() and np.any(s != 0)]
        q = rng.standard_normal((nq, kit.dim), dtype=np.float32)
        for j, s in enumerate(src[:nq]):
            q[j] = s * np.float32(3.0) if j % 2 == 0 else s + np.float32(0.05) * np.abs(s).max() * q[j]
        q = rng.permutation(q)
        if nq >= 3:
            q[2] = 0.0
        yield ("check", 0, q, shapes, "landing %d" % n)
        if n > 1 << 17:
            yield ("check", 0, q, shapes, "landing %d, f16 minima off" % n, NO_F16)
        n0 = n


def test_cosine_shard_grows_through_capacity_and_pass_switches(gpu_ctx):
    """(d) -- dim 64; capacities 1024 -> 2048 -> 4096 -> 131 072 -> 262 144 -> 524 288 with ids, rows and norms copied at each.
    Passes: below 2^17 the dense keys (row stream for up to 4 queries from 4096 rows on, LDS-resident kernel up to 48,
    GEMM above) with select_pruned or select + merge; from 2^17 on the f16 minima for 2 .. 64 queries a pass and k <= 64
    (65 and 300 queries: passes of 33 and 60); k = 65 keeps the dense passes.  At dim 64 the f16 minima pre-empt every
    shape the f32 chunk minima (cosine_prune_ok) and the thresholded GEMM pass (cosine_filter_ok) would take, so from
    131 073 rows on each check runs a second time with UCFP_COSINE_NO_F16: 5 and 48 queries then take the f32 chunk minima
    from 2^17 rows on, and (64, 10) and (300, 10) the thresholded pass at 262 145 rows but not at 262 143 (300: a pass of
    256 and a short dense one)."""
    from ucfp_amd import index
    model = IndexModel(np.float32, (COSINE_GROWTH_DIM,))
    ix = index.DeviceIndex(index.COSINE_F32, COSINE_GROWTH_DIM, ctx=gpu_ctx)
    run_events(cosine_growth_events(), model, ix, cosine_checker)
    ix.close()


# =====================================================================================================================
# scenario (e): append-only shard, two streams, growth between two searches
# =====================================================================================================================
def stream_case(kit, seed):
    """-> ids, rows, blocks ((0, a), (a, b)), queries.  Hamming: 200 000 + 100 000 codes out of a palette of 40 (heavy ties) under
    ascending ids; cosine: 3000 + 2000 rows."""
    rng = np.random.default_rng(seed)
    if kit.dim == 0:
        a, b = 200_000, 300_000
        palette = rng.integers(0, 2**64, 40, dtype=np.uint64)
        rows = palette[rng.integers(0, 40, b)]
        queries = palette[rng.integers(0, 40, 64)] ^ (np.uint64(1) << rng.integers(0, 64, 64).astype(np.uint64))
        queries[:8] = palette[:8]                                         # distance 0 to thousands of rows each
    else:
        a, b = 3000, 5000
        rows = kit.new_rows(rng, b, False)
        queries = rng.standard_normal((64, kit.dim), dtype=np.float32)
        src = [s for s in rows[rng.integers(0, b, 40)] if np.isfinite(s).all() and np.any(s != 0)]
        for j, s in enumerate(src):
            queries[j] = s * np.float32(3.0) if j % 2 else s + np.float32(0.05) * np.abs(s).max() * queries[j]
        queries = rng.permutation(queries)
    ids = np.cumsum(rng.integers(1, 5, b)).astype(np.uint64) + np.uint64(1_000_000)
    return ids, rows, ((0, a), (a, b)), queries


STREAM_K = 10


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).cuda()


def _outs(torch, nq, k):
    return (torch.full((nq, k), -1, dtype=torch.int64, device="cuda"), torch.zeros((nq, k), dtype=torch.float32, device="cuda"),
            torch.full((nq,), -1, dtype=torch.int32, device="cuda"))


def test_append_only_hamming_two_streams_growth_between_searches(gpu_ctx, oracle, torch_cuda):
    """(e) -- append_dev of 200 000 rows on stream A (capacity 262 144); searches of 64 and of 8 queries enqueued on stream B;
    append_dev of 100 000 more on A, which doubles the buffers and frees the ones the searches read; the same searches on B
    into other buffers; ONE synchronisation.  Ids ascend with the row: the single-launch search (8 queries) breaks ties
    by row before and after the growth, the staged search (64 queries) after it (300 000 rows: matrix filter, strict
    thresholds; before it the robust tier).  A third block whose ids start below the last id switches that off, and a fourth
    one, ascending again, must not switch it back on: rows of the third block win ties from behind."""
    torch = torch_cuda
    kit = HammingKit()
    ids, codes, blocks, queries = stream_case(kit, 5150)
    ix = open_index(kit, gpu_ctx, flags=1)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    d_ids, d_codes, d_q = _dev(torch, ids), _dev(torch, codes), _dev(torch, queries)
    torch.cuda.synchronize()
    answers = []

    def append(lo, hi, stream):
        ix.append_dev(0, d_ids[lo:].data_ptr(), d_codes[lo:].data_ptr(), hi - lo, stream.cuda_stream)

    def search(nq, stream):
        o = _outs(torch, nq, STREAM_K)
        d = torch.full((nq, STREAM_K), -1, dtype=torch.int32, device="cuda")
        ix.search_dev(0, d_q.data_ptr(), nq, STREAM_K, o[0].data_ptr(), 0, d.data_ptr(), o[2].data_ptr(), stream.cuda_stream)
        return o[0], d, o[2]

    torch.cuda.synchronize()
    append(*blocks[0], sa)
    answers.append((blocks[0][1], 64, search(64, sb)))
    answers.append((blocks[0][1], 8, search(8, sb)))
    append(*blocks[1], sa)
    answers.append((blocks[1][1], 64, search(64, sb)))
    answers.append((blocks[1][1], 8, search(8, sb)))
    torch.cuda.synchronize()
    assert ix.size(0) == blocks[1][1]
    for n, nq, (g_ids, g_d, g_c) in answers:
        o_ids, o_d, o_c = oracle.hamming_topk(ids[:n], codes[:n], queries[:nq], STREAM_K)
        assert np.array_equal(g_c.cpu().numpy().view(np.uint32), o_c), (n, nq)
        assert np.array_equal(g_d.cpu().numpy().view(np.uint32), o_d), (n, nq)
        assert np.array_equal(g_ids.cpu().numpy().view(np.uint64), o_ids), (n, nq)
    # third block: ids below everything so far, codes from the same palette -- its rows win every tie; fourth: ascending again
    rng = np.random.default_rng(5151)
    ids3 = np.arange(2000, dtype=np.uint64) * np.uint64(2) + np.uint64(10)
    codes3 = codes[rng.integers(0, len(codes), 2000)]
    ids4 = ids[-1] + np.uint64(1) + np.arange(3000, dtype=np.uint64)
    codes4 = codes[rng.integers(0, len(codes), 3000)]
    all_ids, all_codes = ids, codes
    for more_ids, more_codes in ((ids3, codes3), (ids4, codes4)):
        ix.upsert(0, more_ids, more_codes)
        all_ids, all_codes = np.concatenate([all_ids, more_ids]), np.concatenate([all_codes, more_codes])
        for nq in (64, 8):
            g_ids, _, g_d, g_c = ix.search(0, queries[:nq], STREAM_K)
            o_ids, o_d, o_c = oracle.hamming_topk(all_ids, all_codes, queries[:nq], STREAM_K)
            assert np.array_equal(g_c, o_c) and np.array_equal(g_d, o_d) and np.array_equal(g_ids, o_ids), (len(all_ids), nq)
            assert (g_ids[:8, 0] < 1_000_000).all()              # a row of the third block heads every palette query
    ix.close()


def test_append_only_cosine_two_streams_growth_between_searches(gpu_ctx, torch_cuda):
    """(e), cosine -- 3000 rows appended on stream A (capacity 4096), a search of 64 queries on B, 2000 more on A (capacity
    8192: ids, rows and norms move, the new norms land at norms + 3000 of the NEW buffer), the search again on B, one
    synchronisation."""
    torch = torch_cuda
    kit = CosineKit(64)
    ids, rows, blocks, queries = stream_case(kit, 6464)
    ix = open_index(kit, gpu_ctx, flags=1)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    d_ids, d_rows, d_q = _dev(torch, ids), _dev(torch, rows), _dev(torch, queries)
    torch.cuda.synchronize()
    answers = []
    for lo, hi in blocks:
        ix.append_dev(0, d_ids[lo:].data_ptr(), d_rows[lo:].data_ptr(), hi - lo, sa.cuda_stream)
        o = _outs(torch, 64, STREAM_K)
        ix.search_dev(0, d_q.data_ptr(), 64, STREAM_K, o[0].data_ptr(), o[1].data_ptr(), 0, o[2].data_ptr(), sb.cuda_stream)
        answers.append((hi, o))
    torch.cuda.synchronize()
    for n, (g_ids, g_sc, g_c) in answers:
        ref = CosineRef(ids[:n], rows[:n], queries, STREAM_K)
        ref.check(g_ids.cpu().numpy().view(np.uint64), g_sc.cpu().numpy(), g_c.cpu().numpy().view(np.uint32), STREAM_K, COS_TOL)
    ix.close()
