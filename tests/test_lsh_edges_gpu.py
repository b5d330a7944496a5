"""GPU parity at the edges of the banded MinHash LSH shard (lsh.hip: band keys, build, query -- through the C ABI) vs the
numpy checker in oracle/ (spec: DESIGN.md "LSH" L1-L4).  Ids, scores and counts are compared bit for bit; there is no
tolerance.  The cases come from tests/lsh_cases.py; that each of them sits on the edge it names is proved on the CPU in
test_lsh_cases_spec.py."""
import threading

import numpy as np
import pytest

import lsh_cases as lc
from lsh_cases import RUN_CAPS, RUN_LENGTHS, SWEEP_SHAPES, SWEEP_SIZES

pytestmark = pytest.mark.gpu

INVALID = np.uint64(lc.M64)
TOPK_KS = [1, 2, 63, 64, 65, 127, 128]


def _same(got, want, what):
    """(ids, scores, counts) of the kernel and of the checker: same types, same bits; unused places as L4 says."""
    (g_ids, g_sc, g_ct), (o_ids, o_sc, o_ct) = got, want
    assert g_ids.dtype == np.uint64 and g_sc.dtype == np.float32 and g_ct.dtype == np.uint32
    assert g_ids.shape == o_ids.shape and g_sc.shape == o_sc.shape and g_ct.shape == o_ct.shape
    bad = np.flatnonzero(g_ct != o_ct)
    assert not bad.size, f"{what}: counts differ at query {bad[0]}: {g_ct[bad[0]]} != {o_ct[bad[0]]}"
    bad = np.argwhere(g_ids != o_ids)
    assert not bad.size, f"{what}: ids differ at {bad[0].tolist()}: {g_ids[tuple(bad[0])]} != {o_ids[tuple(bad[0])]}"
    bad = np.argwhere(g_sc.view(np.uint32) != o_sc.view(np.uint32))
    assert not bad.size, f"{what}: scores differ at {bad[0].tolist()}: {g_sc[tuple(bad[0])]} != {o_sc[tuple(bad[0])]}"
    unused = np.arange(g_ids.shape[1])[None, :] >= g_ct[:, None]
    assert (g_ids[unused] == INVALID).all() and (g_sc[unused] == -1).all() and (g_sc[~unused] >= 0).all()


def _check_case(text, oracle, case, ks, what, cand_per_band=None):
    """Build the case on a fresh handle and compare a query per k with the checker.  -> results of the last k."""
    ids, corpus, queries, p, _ = case
    cap = cand_per_band or p["cand_per_band"]
    crec, qrec = lc.records(corpus), lc.records(queries)
    idx = text.LshIndex(p["bands"], p["rows"], cap)
    try:
        idx.build(ids, crec)
        for k in ks:
            got = idx.query(qrec, k)
            _same(got, oracle.lsh_query(ids, crec, qrec, k, p["bands"], p["rows"], cap), f"{what} cap={cap} k={k}")
    finally:
        idx.close()
    return got


# ---- band keys (L1) ----

def _key_records(n, seed):
    """Random slots with the values that break a careless fold in the first rows: 0, 2^64-1, and pairs of rows that
    differ only in bit 0 / only in bit 63, of every slot (rows 2-5) or of some slots (rows 6-9)."""
    rng = lc._rng("keys", n, seed)
    slots = lc._slots(rng, n)
    slots[0] = 0
    if n > 1:
        slots[1] = lc.M64
    if n > 5:
        slots[3] = slots[2] ^ np.uint64(1)                  # every slot differs in bit 0 only
        slots[5] = slots[4] ^ np.uint64(1 << 63)            # ... in bit 63 only
    if n > 9:
        slots[7], slots[9] = slots[6], slots[8]
        slots[7, ::5] ^= np.uint64(1)                       # some slots do, the others are equal
        slots[9, 3::7] ^= np.uint64(1 << 63)
    return slots


def _band_key_check(text, oracle, bands, rows, n):
    slots = _key_records(n, rows)
    rec = lc.records(slots)
    want = oracle.lsh_band_keys(rec, bands, rows)
    got = text.lsh_band_keys(rec, bands, rows)
    assert got.shape == (n, bands) and got.dtype == np.uint64
    assert np.array_equal(got, want), (bands, rows, n)
    if n > 9:
        band = [np.arange(b * rows, (b + 1) * rows) for b in range(bands)]
        assert (got[2] != got[3]).all()                                     # bit 0 of a slot moves the key
        assert np.array_equal(got[6] != got[7], np.array([(i % 5 == 0).any() for i in band]))
        # bit 63 reaches the key as a parity over the band (2^63 * odd = 2^63 mod 2^64): an odd number of
        # flipped slots moves the key, an even number leaves it
        assert ((got[4] != got[5]) == (rows % 2 == 1)).all()
        assert np.array_equal(got[8] != got[9], np.array([(i % 7 == 3).sum() % 2 == 1 for i in band]))
    # neither the header nor a slot behind bands * rows takes part
    rng = lc._rng("junk", bands, rows, n)
    rec2 = rec.copy()
    rec2[:, :8] = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    rec2[:, 8 + 8 * bands * rows:] = rng.integers(0, 256, size=(n, 1024 - 8 * bands * rows), dtype=np.uint8)
    assert (rec2[:, :8] != rec[:, :8]).any()
    assert np.array_equal(text.lsh_band_keys(rec2, bands, rows), want), (bands, rows, n)


def test_band_keys_every_legal_rows(gpu_ctx, oracle):
    from ucfp_amd import text
    for rows in range(1, 65):
        for bands in sorted({128 // rows, 1}):
            _band_key_check(text, oracle, bands, rows, 257)


@pytest.mark.parametrize("n", [1, 255, 256])
def test_band_keys_block_edges(gpu_ctx, oracle, n):
    from ucfp_amd import text
    _band_key_check(text, oracle, 16, 8, n)


# ---- every band shape through build + query ----

@pytest.mark.parametrize("n", SWEEP_SIZES)
@pytest.mark.parametrize("bands,rows", SWEEP_SHAPES)
def test_shape_sweep(gpu_ctx, oracle, bands, rows, n):
    from ucfp_amd import text
    case = lc.one_band_matches(bands, rows, n)
    g_ids, g_sc, g_ct = _check_case(text, oracle, case, (1, 128), f"one_band {bands}x{rows} n={n}")
    src = case[4]["band_src"]
    assert (g_ct == 1).all() and np.array_equal(g_ids[:bands, 0], case[0][src])      # band b found its row, for every b
    assert (g_sc[:bands, 0] == np.float32(rows / 128)).all()
    if bands * rows < 128:
        case = lc.uncovered_slots(bands, rows, n)
        g_ids, g_sc, g_ct = _check_case(text, oracle, case, (1, 128), f"uncovered {bands}x{rows} n={n}")
        for j, (kind, s, agree) in enumerate(case[4]["kinds"]):
            if kind == "U":
                assert g_ct[j] == 0
            elif kind != "P":
                assert g_ct[j] == 1 and g_ids[j, 0] == case[0][s] and g_sc[j, 0] == np.float32(agree / 128)


# ---- run length against cand_per_band, at every position of the table ----

@pytest.mark.parametrize("L", RUN_LENGTHS)
@pytest.mark.parametrize("position", lc.POSITIONS)
def test_runs_against_the_per_band_cap(gpu_ctx, oracle, position, L):
    from ucfp_amd import text
    case = lc.run_at(position, L)
    ids, f = case[0], case[4]
    for cap in RUN_CAPS:
        g_ids, g_sc, g_ct = _check_case(text, oracle, case, (128,), f"run {position} L={L}", cand_per_band=cap)
        assert g_ct[0] == min(L, cap, 128) and g_ct[2] == 0
        if min(L, cap) <= 128:                              # the first `cap` rows of the run, whatever their ids
            assert set(g_ids[0, :g_ct[0]].tolist()) == set(ids[f["run_rows"][:cap]].tolist())


# ---- the cut at 1024 ----

@pytest.mark.parametrize("variant", lc.CUT_VARIANTS)
def test_cut_at_1024(gpu_ctx, oracle, variant):
    from ucfp_amd import text
    case = lc.cut_at_1024(variant)
    ids, f = case[0], case[4]
    present = f["x_entry"] is not None and f["x_entry"] < lc.MAX_CAND
    g_ids, g_sc, g_ct = _check_case(text, oracle, case, (1, 128), f"cut {variant}")
    if f["x"] is not None:
        assert (ids[f["x"]] in g_ids[0]) == present
    if variant == "inside":
        assert g_ids[0, 0] == ids[f["x"]] and g_sc[0, 0] == np.float32(0.8828125)
    if variant in ("outside_cut", "outside_cap"):
        assert g_sc[0, 0] == np.float32(0.0625)


# ---- the top-k list: lanes, the 63 -> 64 seam, arrival orders, ids at the top of the range ----

@pytest.mark.parametrize("order,mixed_ids", [(o, False) for o in lc.ORDERS] + [("random", True)])
def test_topk_lanes(gpu_ctx, oracle, order, mixed_ids):
    from ucfp_amd import text
    case = lc.graded(order, mixed_ids=mixed_ids)
    ids, corpus, queries, p, f = case
    crec, qrec = lc.records(corpus), lc.records(queries)
    idx = text.LshIndex(p["bands"], p["rows"], p["cand_per_band"])
    try:
        idx.build(ids, crec)
        for k in TOPK_KS:
            g_ids, g_sc, g_ct = got = idx.query(qrec, k)
            _same(got, oracle.lsh_query(ids, crec, qrec, k, 16, 8, 1024), f"graded {order} mixed={mixed_ids} k={k}")
            assert g_ct[0] == k                                             # more graded candidates than places
            assert (np.diff(g_sc[0]) <= 0).all()
            # query 1: `counts` tells the row whose id is 2^64-1 from a place that nobody took
            c1 = int(g_ct[1])
            if c1 < k:
                assert g_ids[1, c1 - 1] == INVALID and g_sc[1, c1 - 1] == np.float32(8 / 128)
                assert (g_ids[1, c1:] == INVALID).all() and (g_sc[1, c1:] == -1).all()
    finally:
        idx.close()


# ---- rebuilds on one handle ----

def test_rebuilds_to_other_sizes(gpu_ctx, oracle):
    from ucfp_amd import text
    other = lc.one_band_matches(32, 4, 257)
    o_rec, o_q = lc.records(other[1]), lc.records(other[2])
    o_want = oracle.lsh_query(other[0], o_rec, o_q, 3, 32, 4)
    idx, idx2 = text.LshIndex(16, 8), text.LshIndex(32, 4)
    try:
        idx2.build(other[0], o_rec)
        for ids, corpus, queries, p, f in lc.resize_sequence():
            crec, qrec = lc.records(corpus), lc.records(queries)
            idx.build(ids, crec)
            assert idx.n == corpus.shape[0]
            g_ids, g_sc, g_ct = got = idx.query(qrec, 4)
            _same(got, oracle.lsh_query(ids, crec, qrec, 4, 16, 8), f"rebuild step {f['step']}")
            assert (g_ct[:f["n_own"]] == 1).all() and not g_ct[f["n_own"]:].any()    # rows of earlier builds are gone
            found = g_ids[g_ids != INVALID]
            assert (found >> np.uint64(32) == np.uint64(f["step"])).all()
            _same(idx2.query(o_q, 3), o_want, f"the other handle after step {f['step']}")
    finally:
        idx.close()
        idx2.close()


# ---- the device entries with the caller's own buffers ----

GUARD = 64          # bytes behind every output
FILL = 0x5A


def _dev_bytes(torch, arr, offset=0):
    """The bytes of `arr` on the device, `offset` bytes behind an 8-byte-aligned address.  -> (tensor, pointer)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    host = np.full(offset + raw.size + 8, FILL, np.uint8)
    host[offset:offset + raw.size] = raw
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 8 == 0
    return t, t.data_ptr() + offset


def _out(torch, nbytes):
    t = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 8 == 0
    return t


def _read(t, nbytes, dtype, shape):
    """-> (the first nbytes as dtype, True if every byte behind them is still FILL)"""
    h = t.cpu().numpy()
    return h[:nbytes].view(dtype).reshape(shape).copy(), bool((h[nbytes:] == FILL).all())


def _query_dev(torch, idx, q_ptr, nq, k, stream):
    """query_dev into guarded buffers on `stream` (a raw handle); the caller synchronises.  -> reader()"""
    o_ids, o_sc, o_ct = _out(torch, nq * k * 8), _out(torch, nq * k * 4), _out(torch, nq * 4)
    torch.cuda.current_stream().synchronize()                   # the fills are done before another stream writes
    idx.query_dev(q_ptr, nq, k, o_ids.data_ptr(), o_sc.data_ptr(), o_ct.data_ptr(), stream)

    def reader():
        a, ga = _read(o_ids, nq * k * 8, np.uint64, (nq, k))
        b, gb = _read(o_sc, nq * k * 4, np.float32, (nq, k))
        c, gc = _read(o_ct, nq * 4, np.uint32, (nq,))
        assert ga and gb and gc, "bytes behind an output were written"
        return a, b, c
    return reader


@pytest.mark.parametrize("bands,rows,n,k", [(16, 8, 257, 5), (20, 6, 65, 128), (128, 1, 64, 1)])
def test_dev_entries_own_stream_and_4_byte_aligned_records(gpu_ctx, oracle, torch_cuda, bands, rows, n, k):
    """build_dev / query_dev / ucfp_text_lsh_band_keys_dev with the caller's tensors, on a stream that is not torch's
    current one, the records 4 bytes off an 8-byte boundary (all the header promises), the outputs guarded."""
    from ucfp_amd import _lib, text
    torch = torch_cuda
    ids, corpus, queries, p, _ = lc.one_band_matches(bands, rows, n)
    crec, qrec = lc.records(corpus), lc.records(queries)
    nq = qrec.shape[0]
    d_ids, ids_ptr = _dev_bytes(torch, ids)
    d_c, c_ptr = _dev_bytes(torch, crec, 4)
    d_q, q_ptr = _dev_bytes(torch, qrec, 4)
    assert c_ptr % 8 == 4 and q_ptr % 8 == 4
    d_keys = _out(torch, bands * n * 8)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream and s.cuda_stream != torch.cuda.current_stream().cuda_stream
    idx = text.LshIndex(bands, rows)
    try:
        _lib.check(_lib.load().ucfp_text_lsh_band_keys_dev(gpu_ctx.handle, c_ptr, n, bands, rows, d_keys.data_ptr(),
                                                           s.cuda_stream))
        idx.build_dev(ids_ptr, c_ptr, n, s.cuda_stream)
        reader = _query_dev(torch, idx, q_ptr, nq, k, s.cuda_stream)
        s.synchronize()
        _same(reader(), oracle.lsh_query(ids, crec, qrec, k, bands, rows), f"dev {bands}x{rows}")
        keys, guard = _read(d_keys, bands * n * 8, np.uint64, (bands, n))
        assert guard and np.array_equal(keys.T, oracle.lsh_band_keys(crec, bands, rows))
        # nq = 0: success, and nothing is written
        o = _out(torch, 64)
        torch.cuda.synchronize()
        rc = _lib.load().ucfp_lsh_query_dev(idx.handle, q_ptr, 0, k, o.data_ptr(), o.data_ptr(), o.data_ptr(),
                                            s.cuda_stream)
        s.synchronize()
        assert rc == 0 and (o.cpu().numpy() == FILL).all()
    finally:
        idx.close()


def test_two_threads_two_streams_one_handle(gpu_ctx, oracle, torch_cuda):
    """Two host threads, a stream each, 8 queries each (one call per query, k varies) against one handle."""
    from ucfp_amd import text
    torch = torch_cuda
    ids, corpus, queries, p, _ = lc.one_band_matches(16, 8, 4097)
    crec = lc.records(corpus)
    near = corpus[100:108].copy()
    near[:, 40:] = lc._slots(lc._rng("threads"), 8)[:, 40:]         # bands 0..4 of rows 100..107
    qsets = [lc.records(np.concatenate([queries[:4], near[:4]])), lc.records(np.concatenate([near[4:], queries[12:16]]))]
    ks = [1, 2, 63, 64, 65, 127, 128, 10]
    idx = text.LshIndex(16, 8)
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def worker(t):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                d_q, q_ptr = _dev_bytes(torch, qsets[t])
                gate.wait(timeout=60)
                readers = [_query_dev(torch, idx, q_ptr + 1032 * i, 1, ks[i], s.cuda_stream) for i in range(8)]
                s.synchronize()
                results[t] = [r() for r in readers]
        except BaseException as e:       # noqa: BLE001 -- handed to the main thread
            errors.append(e)
            gate.abort()

    try:
        idx.build(ids, crec)
        threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        if errors:
            raise errors[0]
        for t in range(2):
            for i in range(8):
                want = oracle.lsh_query(ids, crec, qsets[t][i:i + 1], ks[i], 16, 8)
                assert want[2][0] == 1
                _same(results[t][i], want, f"thread {t} query {i}")
    finally:
        idx.close()
