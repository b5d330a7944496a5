"""TLSH-distance search on the device (tlsh_index.hip): ids, distances, scores and counts equal the exact
top-k by (distance, id) of the restatement (tests/tlsh_ref.py) -- over random 35-byte rows with digests planted at known
distances from the queries, ties, header wrap-around, the distance cut, tenants, mutations, the pass loop, the device
entry point, and end to end from fingerprint_tlsh through GpuIndex.query."""
import numpy as np
import pytest

import tlsh_ref as ref

pytestmark = pytest.mark.gpu

INVALID_ID = 0xFFFFFFFFFFFFFFFF
N_BIG, N_SMALL, NQ_BIG, NQ_SMALL = 70_001, 1000, 65, 257


def _nudge(rng, dig: np.ndarray, steps: int) -> np.ndarray:
    """A copy of the digest at body distance `steps`: that many distinct bit pairs moved by one."""
    out = dig.copy()
    for p in rng.choice(128, steps, replace=False).tolist():
        byte, sh = 3 + p // 4, 2 * (p % 4)
        a = (int(out[byte]) >> sh) & 3
        b = a + 1 if a == 0 else a - 1
        out[byte] = (int(out[byte]) & ~(3 << sh)) | (b << sh)
    return out


@pytest.fixture(scope="module")
def pool():
    """Rows, ids and queries shared by the size cases, with the restatement's distances computed once: `big` is 65 queries
    over 70 001 rows, `small` 257 queries over the first 1000 rows.  The first 200 queries have copies planted at distances
    0, 3 and 17 (two of them): those of the first 15 queries among the first 60 rows, the others among rows 64 .. 803."""
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 256, (N_BIG, 35), dtype=np.uint8)
    queries = rng.integers(0, 256, (NQ_SMALL, 35), dtype=np.uint8)
    for q in range(200):
        for j, steps in enumerate((0, 3, 17, 17)):
            slot = q * 4 + j if q < 15 else 64 + (q - 15) * 4 + j
            rows[slot] = _nudge(rng, queries[q], steps)
    ids = rng.permutation(np.arange(1, N_BIG + 1, dtype=np.uint64) * np.uint64(0x9E3779B1))   # row order is not id order
    big = ref.distance_matrix(queries[:NQ_BIG], rows)
    small = ref.distance_matrix(queries, rows[:N_SMALL])
    return rows, ids, queries, big, small


def _check(got, want, k):
    g_ids, g_d, g_s, g_n = got
    w_ids, w_d, w_s, w_n = want
    assert g_ids.shape == g_d.shape == g_s.shape == (w_n.size, k)
    assert np.array_equal(g_n, w_n), (g_n[:8], w_n[:8])
    assert np.array_equal(g_d, w_d), np.argwhere(g_d != w_d)[:4]
    assert np.array_equal(g_ids, w_ids), np.argwhere(g_ids != w_ids)[:4]
    assert g_s.tobytes() == w_s.tobytes()


SIZES = [(1, 1, 1), (1, 3, 10), (1, 65, 128), (63, 1, 10), (63, 64, 128), (63, 257, 1), (64, 3, 128), (64, 65, 10), (64, 257, 128),
         (65, 1, 128), (65, 64, 1), (65, 257, 10), (1000, 1, 1), (1000, 3, 128), (1000, 64, 10), (1000, 65, 128), (1000, 257, 10),
         (70_001, 1, 10), (70_001, 3, 128), (70_001, 64, 1), (70_001, 65, 10)]


@pytest.mark.parametrize("n,nq,k", SIZES)
def test_sizes(gpu_ctx, pool, n, nq, k):
    from ucfp_amd.index import TlshIndex
    rows, ids, queries, big, small = pool
    dm = small[:nq, :n] if n <= N_SMALL else big[:nq, :n]
    ix = TlshIndex(ctx=gpu_ctx)
    ix.upsert(5, ids[:n], rows[:n])
    assert ix.size(5) == n
    got = ix.query(5, queries[:nq], k)
    want = ref.topk_from_distances(ids[:n], dm, k)
    _check(got, want, k)
    if n >= 64:
        assert (got[1][:min(nq, 15), 0] == 0).all()          # the planted exact copy comes first
    if k > n:
        assert (got[3] == n).all() and (got[0][:, n:] == INVALID_ID).all() and (got[2][:, n:] == -1.0).all()
    ix.close()


def test_pass_loop(gpu_ctx, pool, monkeypatch):
    """A key matrix smaller than the batch: 257 queries over 1000 rows in passes of 65, 65, 65 and 62."""
    from ucfp_amd.index import TlshIndex
    rows, ids, queries, big, small = pool
    monkeypatch.setenv("UCFP_TLSH_KEY_BYTES", str(65 * 4 * N_SMALL))
    ix = TlshIndex(ctx=gpu_ctx)
    monkeypatch.delenv("UCFP_TLSH_KEY_BYTES")
    ix.upsert(0, ids[:N_SMALL], rows[:N_SMALL])
    for k in (10, 128):
        _check(ix.query(0, queries, k), ref.topk_from_distances(ids[:N_SMALL], small, k), k)
    ix.close()


def test_short_last_pass(gpu_ctx, pool, monkeypatch):
    """A last pass that wants more slices than the partial lists were sized for: 65 queries over 33 000 rows in passes of
    64 and 1.  select_plan(33000, 64) asks for 4096 / 64 = 64 slices, 516 rows each, rounded up to 576: 58 slices, and the
    partial lists are reserved for those.  select_plan(33000, 1) is capped at ceil(33000 / 512) = 65 slices of 512 rows;
    65 > 58, so the pass loop has to bring the one-query pass back to 58 slices of 576 rows."""
    from ucfp_amd.index import TlshIndex
    rows, ids, queries, big, small = pool
    n, nq = 33_000, 65
    monkeypatch.setenv("UCFP_TLSH_KEY_BYTES", str(64 * 4 * n))
    ix = TlshIndex(ctx=gpu_ctx)
    monkeypatch.delenv("UCFP_TLSH_KEY_BYTES")
    ix.upsert(0, ids[:n], rows[:n])
    for k in (10, 128):
        _check(ix.query(0, queries[:nq], k), ref.topk_from_distances(ids[:n], big[:nq, :n], k), k)
    ix.close()


def test_identical_rows_return_the_smallest_ids(gpu_ctx):
    from ucfp_amd.index import TlshIndex
    rng = np.random.default_rng(12)
    row = rng.integers(0, 256, 35, dtype=np.uint8)
    ids = rng.permutation(np.arange(1000, dtype=np.uint64) * np.uint64(7) + np.uint64(3))    # inserted in shuffled order
    ix = TlshIndex(ctx=gpu_ctx)
    ix.upsert(0, ids, np.tile(row, (1000, 1)))
    g_ids, g_d, g_s, g_n = ix.query(0, [row.tobytes(), _nudge(rng, row, 5).tobytes()], 10)
    assert g_ids[0].tolist() == g_ids[1].tolist() == sorted(ids.tolist())[:10]
    assert g_d[0].tolist() == [0] * 10 and g_d[1].tolist() == [5] * 10 and g_n.tolist() == [10, 10]
    assert (g_s[0] == 1.0).all()
    ix.close()


def test_header_wrap_around(gpu_ctx):
    from ucfp_amd.index import TlshIndex
    body = bytes(range(32))
    sw = ref.swap
    rows = [bytes([0x11, sw(255), 0x00]) + body,      # id 1: L = 255
            bytes([0x11, sw(0), 0xF0]) + body,        # id 2: L = 0, Q1 = 15
            bytes([0x11, sw(128), 0x08]) + body,      # id 3: half a ring away in L and Q2
            bytes([0x22, sw(2), 0x02]) + body]        # id 4: another checksum, L two steps away, Q2 two steps away
    q = bytes([0x11, sw(0), 0x00]) + body
    want_d = [1, 1, 12 * 128 + 12 * 7, 1 + 24 + 12]
    assert [ref.distance(q, r) for r in rows] == want_d
    ix = TlshIndex(ctx=gpu_ctx)
    ix.upsert(0, np.array([1, 2, 3, 4], np.uint64), rows)
    got = ix.query(0, [q], 4)
    _check(got, ref.topk(np.array([1, 2, 3, 4], np.uint64), np.frombuffer(b"".join(rows), np.uint8), np.frombuffer(q, np.uint8), 4), 4)
    assert got[0][0].tolist() == [1, 2, 4, 3] and got[1][0].tolist() == [1, 1, 37, 1620]
    ix.close()


def test_max_distance(gpu_ctx, pool):
    from ucfp_amd.index import TlshIndex
    rows, ids, queries, big, small = pool
    ix = TlshIndex(ctx=gpu_ctx)
    ix.upsert(0, ids[:N_SMALL], rows[:N_SMALL])
    q = queries[20:23]
    for md, per_query in ((0, 1), (2, 1), (3, 2), (16, 2), (17, 4), (18, 4), (None, 10)):   # planted at 0, 3, 17, 17
        got = ix.query(0, q, 10, md)
        _check(got, ref.topk_from_distances(ids[:N_SMALL], small[20:23], 10, md), 10)
        assert got[3].tolist() == [per_query] * 3, md
    assert ix.query(0, rows[N_SMALL:N_SMALL + 1], 10, 0)[3].tolist() == [0]       # nothing within 0 of a stranger
    ix.close()


def test_tenants_mutations_and_empty_answers(gpu_ctx, pool):
    from ucfp_amd.index import TlshIndex
    rows, ids, queries, big, small = pool
    ix = TlshIndex(ctx=gpu_ctx)
    a_ids, b_ids = ids[:300], ids[300:500]
    ix.upsert(1, a_ids, rows[:300])
    ix.upsert(2, b_ids, rows[300:500])
    assert (ix.size(1), ix.size(2), ix.size(3)) == (300, 200, 0)
    q = queries[:5]
    dm_a, dm_b = small[:5, :300], small[:5, 300:500]
    _check(ix.query(1, q, 10), ref.topk_from_distances(a_ids, dm_a, 10), 10)
    _check(ix.query(2, q, 10), ref.topk_from_distances(b_ids, dm_b, 10), 10)
    # unknown tenant, k = 0, nq = 0
    e_ids, e_d, e_s, e_n = ix.query(9, q, 10)
    assert (e_ids == INVALID_ID).all() and (e_d == 0xFFFFFFFF).all() and (e_s == -1.0).all() and not e_n.any()
    assert not ix.query(1, q, 0)[3].any()
    assert ix.query(1, np.zeros((0, 35), np.uint8), 10)[3].shape == (0,)
    # upsert of a known id replaces its row: the nearest row of query 0 becomes a stranger's digest, and back
    first = int(ix.query(1, q[:1], 1)[0][0, 0])
    pos = int(np.flatnonzero(a_ids == np.uint64(first))[0])
    changed = rows[:300].copy()
    changed[pos] = rows[N_SMALL + 7]
    ix.upsert(1, a_ids[pos:pos + 1], changed[pos:pos + 1])
    assert ix.size(1) == 300
    _check(ix.query(1, q, 10), ref.topk(a_ids, changed, q, 10), 10)
    assert int(ix.query(1, q[:1], 1)[0][0, 0]) != first
    # delete: known ids go, unknown ones are not counted, the other tenant is untouched
    gone = a_ids[:50]
    assert ix.delete(1, np.concatenate([gone, np.array([1], np.uint64)])) == 50 and ix.delete(1, gone) == 0
    assert (ix.size(1), ix.size(2)) == (250, 200)
    ix.flush()
    _check(ix.query(1, q, 10), ref.topk(a_ids[50:], changed[50:], q, 10), 10)
    _check(ix.query(2, q, 10), ref.topk_from_distances(b_ids, dm_b, 10), 10)
    assert ix.delete(2, b_ids) == 200 and not ix.query(2, q, 10)[3].any()
    ix.close()


def test_device_entry_points(gpu_ctx, torch_cuda, pool):
    from ucfp_amd.index import TlshIndex
    torch = torch_cuda
    rows, ids, queries, big, small = pool
    n, nq, k = 777, 33, 10
    st = torch.cuda.current_stream().cuda_stream
    ix = TlshIndex(ctx=gpu_ctx)
    d_ids = torch.from_numpy(ids[:n].view(np.int64).copy()).cuda()
    d_rows = torch.from_numpy(rows[:n].copy()).cuda()
    ix.upsert_dev(0, d_ids.data_ptr(), d_rows.data_ptr(), n, st)
    assert ix.size(0) == n
    d_q = torch.from_numpy(queries[:nq].copy()).cuda()
    o_ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_d = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
    o_s = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_n = torch.zeros(nq, dtype=torch.int32, device="cuda")
    ix.query_dev(0, d_q.data_ptr(), nq, k, 0xFFFFFFFF, o_ids.data_ptr(), o_d.data_ptr(), o_s.data_ptr(), o_n.data_ptr(), st)
    torch.cuda.synchronize()
    got = (o_ids.cpu().numpy().view(np.uint64), o_d.cpu().numpy().view(np.uint32), o_s.cpu().numpy(), o_n.cpu().numpy().view(np.uint32))
    _check(got, ref.topk_from_distances(ids[:n], small[:nq, :n], k), k)
    _check(ix.query(0, queries[:nq], k), got, k)            # the host twin
    ix.close()


def test_gpu_index_end_to_end(gpu_ctx):
    """fingerprint_tlsh -> GpuIndex.upsert -> query with a `tlsh` body: every near-copy finds its original first."""
    import random
    from ucfp_amd import text
    from ucfp_amd.core import HitSource, Modality, QueryRequest
    from ucfp_amd.index import GpuIndex
    rnd = random.Random(13)

    def word():
        return "".join(rnd.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randrange(3, 10)))

    originals = []
    for _ in range(100):                      # about 1 KiB each, every document over a vocabulary of its own: in the
        vocab = [word() for _ in range(40)]   # restatement a copy is then within 91 of its original, strangers 157 and more apart
        originals.append(" ".join(rnd.choice(vocab) for _ in range(160)))
    copies = []
    for doc in originals:
        w = doc.split()
        w[rnd.randrange(len(w))] = "EDITED"
        copies.append(" ".join(w))
    opts = text.TextOpts()
    recs = [text.fingerprint_tlsh(d, opts, 3, 1000 + i) for i, d in enumerate(originals)]
    recs += [text.fingerprint_tlsh(d, opts, 4, 1000 + i) for i, d in enumerate(originals[:5])]      # another tenant
    for i, r in enumerate(recs[:100]):
        want = ref.digest(originals[i].casefold().encode())
        assert r.fingerprint == ref.hexdigest(want).encode() and r.algorithm == "tlsh-128-1" and r.text == originals[i]
    gi = GpuIndex(gpu_ctx)
    gi.upsert(recs)
    digs = np.stack([np.frombuffer(text.tlsh_digest_bytes(r.fingerprint), np.uint8) for r in recs[:100]])
    ids = np.arange(1000, 1100, dtype=np.uint64)
    for i, doc in enumerate(copies):
        c = text.fingerprint_tlsh(doc, opts, 3, 5000 + i)
        req = QueryRequest.from_json({"tenant_id": 3, "modality": "Text", "tlsh": c.fingerprint.decode(), "k": 3,
                                      "algorithm": "tlsh-128-1"})
        hits = gi.query(req)
        w_ids, w_d, w_s, _ = ref.topk(ids, digs, np.frombuffer(text.tlsh_digest_bytes(c.fingerprint), np.uint8), 3)
        assert [h.record_id for h in hits] == w_ids[0].tolist() and [h.distance for h in hits] == w_d[0].tolist()
        assert hits[0].record_id == 1000 + i and hits[0].source == HitSource.Tlsh and hits[0].tenant_id == 3, (i, hits[:2])
        assert np.float32(hits[0].score) == w_s[0, 0]
    # the same through nearest_tlsh with the raw bytes and a cut; the other tenant only sees its own five
    raw = text.tlsh_digest_bytes(recs[0].fingerprint)
    assert [h.record_id for h in gi.nearest_tlsh(3, raw, 5, max_distance=0)] == [1000]
    assert len(gi.nearest_tlsh(4, raw, 10)) == 5 and gi.nearest_tlsh(5, raw, 10) == []
    # a record re-ingested under another algorithm leaves the TLSH index; delete removes the rest
    gi.upsert([text.fingerprint_simhash_tf(originals[0], opts, 3, 1000)])
    assert 1000 not in [h.record_id for h in gi.nearest_tlsh(3, raw, 10)]
    gi.delete(3, range(1000, 1100))
    assert gi.nearest_tlsh(3, raw, 10) == []
    assert QueryRequest.from_json({"tenant_id": 3, "modality": "Text", "tlsh": list(raw)}).modality == Modality.Text
