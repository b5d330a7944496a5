"""TLSH 128/1 digests on the device (tlsh.hip): every digest and status is compared bit for bit with the
restatement (tests/tlsh_ref.py) -- lengths around the 64-byte steps and 256-byte stages of a wave, all byte values, the
refusal boundary, a skewed document, a ragged batch, and the host and device entry points against each other."""
import numpy as np
import pytest

import tlsh_ref as ref

pytestmark = pytest.mark.gpu

REFUSED_64 = b"acabacbaacacababaaccbcabccababcbcabcacabacacaaacbaaaaccbbbaaabcbcabcbaaca"
ACCEPTED_65 = b"cabaabbaaacbabbaacabbccbcbbbbcaababcaacbbccabbccaabaaccabaacaaacbcbcbaaacc"


def _rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _agree(gpu_ctx, docs):
    from ucfp_amd import text
    got, st = text.tlsh_batch(docs, ctx=gpu_ctx)
    want, wst = ref.digest_batch(docs)
    assert got.shape == (len(docs), 35) and st.shape == (len(docs),)
    bad = [i for i in range(len(docs)) if st[i] != wst[i] or got[i].tobytes() != want[i].tobytes()]
    assert not bad, [(i, len(docs[i]), int(st[i]), int(wst[i]), got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad[:4]]
    return got, st


def test_short_lengths(gpu_ctx):
    rng = np.random.default_rng(1)
    docs = [_rand(rng, n) for n in (0, 1, 4, 5, 49, 50, 51)]
    got, st = _agree(gpu_ctx, docs)
    assert st.tolist() == [-1, -1, -1, -1, -1, 0, 0]
    assert not got[:5].any() and got[5].any() and got[6].any()


def test_step_and_stage_boundaries(gpu_ctx):
    rng = np.random.default_rng(2)
    lengths = list(range(60, 71)) + list(range(124, 134)) + list(range(252, 262)) + [4095, 4096, 4097, 65_539]
    _, st = _agree(gpu_ctx, [_rand(rng, n) for n in lengths])
    assert not st.any()


def test_one_mebibyte_document(gpu_ctx):
    rng = np.random.default_rng(3)
    _, st = _agree(gpu_ctx, [_rand(rng, 1 << 20)])
    assert st[0] == 0


def test_all_byte_values(gpu_ctx):
    rng = np.random.default_rng(4)
    body = _rand(rng, 700)
    docs = [bytes(range(256)) * 2, b"\0" + body, body + b"\0", b"\0" * 5 + body + b"\0" * 5, b"\xff" + body + b"\xff",
            bytes(range(255, -1, -1)) + body, b"\0" * 300 + body]
    assert len(set(b"".join(docs))) == 256 and len(set(body)) > 200
    _, st = _agree(gpu_ctx, docs)
    assert not st.any()


def test_refusal_boundary(gpu_ctx):
    assert ref.nonzero_buckets(REFUSED_64) == 64 and ref.nonzero_buckets(ACCEPTED_65) == 65   # from the restatement alone
    assert len(REFUSED_64) >= 50 and len(ACCEPTED_65) >= 50
    got, st = _agree(gpu_ctx, [REFUSED_64, ACCEPTED_65, b"a" * 100])
    assert st.tolist() == [-1, 0, -1]
    assert not got[0].any() and got[1].any() and not got[2].any()


def test_skewed_document(gpu_ctx):
    rng = np.random.default_rng(5)
    doc = _rand(rng, 300) + b"abcdefg" * 200_000        # hot buckets, large counts, same-address conflicts
    _, st = _agree(gpu_ctx, [doc])
    assert st[0] == 0


def test_ragged_batch(gpu_ctx):
    from ucfp_amd import text
    rng = np.random.default_rng(6)
    docs = []
    for i in range(300):
        if i % 7 == 3:
            docs.append(b"")
        elif i % 7 == 5:
            docs.append(b"ab" * int(rng.integers(25, 200)))           # long enough, too few buckets
        elif i % 11 == 0:
            docs.append(_rand(rng, int(rng.integers(1, 50))))         # too short
        else:
            docs.append(_rand(rng, int(rng.integers(50, 1200))))
    starts = np.cumsum([0] + [len(d) for d in docs[:-1]])
    assert set((starts % 16).tolist()) == set(range(16))
    got, st = _agree(gpu_ctx, docs)
    refused = st != 0
    assert 80 < refused.sum() < 200 and not got[refused].any() and got[~refused].any(axis=1).all()
    # a document's record does not depend on its neighbours
    alone, ast = text.tlsh_batch([docs[1], docs[150], docs[299]], ctx=gpu_ctx)
    assert np.array_equal(alone, got[[1, 150, 299]]) and np.array_equal(ast, st[[1, 150, 299]])
    # n = 0
    e, es = text.tlsh_batch([], ctx=gpu_ctx)
    assert e.shape == (0, 35) and es.shape == (0,)
    from ucfp_amd import _lib
    assert _lib.load().ucfp_text_tlsh_batch(gpu_ctx.handle, None, None, 0, None, None) == 0
    assert _lib.load().ucfp_text_tlsh_batch_dev(gpu_ctx.handle, None, None, 0, None, None, None) == 0


def test_host_and_device_twins_agree(gpu_ctx, torch_cuda):
    from ucfp_amd import _lib, text
    torch = torch_cuda
    rng = np.random.default_rng(7)
    docs = [_rand(rng, n) for n in (50, 63, 64, 65, 257, 1000, 3, 4099)] + [REFUSED_64, b""]
    host, hst = text.tlsh_batch(docs, ctx=gpu_ctx)
    want, wst = ref.digest_batch(docs)
    assert np.array_equal(host, want) and np.array_equal(hst, wst)
    for lead in (0, 1, 3):                                 # the blob at every alignment of its first byte
        blob = np.frombuffer(b"\xaa" * lead + b"".join(docs) + b"\xbb" * 16, np.uint8).copy()
        offs = (np.cumsum([0] + [len(d) for d in docs]) + lead).astype(np.uint64)
        d_blob = torch.from_numpy(blob).cuda()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        d_out = torch.full((len(docs) * 35 + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.full((len(docs),), 99, dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().ucfp_text_tlsh_batch_dev(gpu_ctx.handle, d_blob.data_ptr(), d_offs.data_ptr(), len(docs),
                                                        d_out.data_ptr(), d_st.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream or None))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert np.array_equal(out[:len(docs) * 35].reshape(-1, 35), host), lead
        assert (out[len(docs) * 35:] == 0x5A).all()        # nothing written behind the last record
        assert np.array_equal(d_st.cpu().numpy(), hst), lead
