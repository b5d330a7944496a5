"""The slot rules every stream set shares (ucfp_amd/csrc/stream_slots.h, stream_set.h), through each of the four kinds:
Wang (A9), Panako (A19), Haitsma (A18) and MinHash text (T7).  `open` hands out the lowest free slot; a call that names
a slot twice, a closed slot, a slot out of range or more entries than the set has slots is refused with the same words
everywhere, and a refused call leaves nothing behind: the same slots push in the next call."""
import numpy as np
import pytest

from ucfp_amd.errors import InvalidArgument

pytestmark = pytest.mark.gpu

KINDS = ("wang", "panako", "haitsma", "text")
CHUNK = 2000                     # samples of an audio entry; a text entry has 10 bytes
ROWS = 4096                      # output rows: above what three such chunks can emit under any of the configs here


def _make(kind, ctx, window_frames=0):
    from ucfp_amd import audio, text
    if kind == "wang":
        return audio.WangStreams(3, ctx=ctx)
    if kind == "panako":
        return audio.PanakoStreams(3, audio.PanakoConfig(target_zone_t=16), window_frames=window_frames, ctx=ctx)
    if kind == "haitsma":
        return audio.HaitsmaStreams(3, 8000, block_frames=4, ctx=ctx)
    return text.MinHashStreams(3, ctx=ctx)


class _Pusher:
    """push_dev of one kind with buffers allocated once; a push that is accepted is also waited for."""

    def __init__(self, kind, s, torch):
        self.kind, self.s, self.torch = kind, s, torch
        rng = np.random.default_rng(5)
        if kind == "text":
            self.data = torch.from_numpy(np.frombuffer(b"some words" * 4, np.uint8).copy()).cuda()
            self.out = torch.zeros((4, 1032), dtype=torch.uint8, device="cuda")
            self.aux = torch.zeros(4, dtype=torch.int32, device="cuda")
        else:
            self.data = torch.from_numpy((0.2 * rng.standard_normal(4 * CHUNK)).astype(np.float32)).cuda()
            shape = {"wang": (ROWS, 2), "panako": (ROWS, 4), "haitsma": (ROWS,)}[kind]
            self.out = torch.zeros(shape, dtype=torch.int32, device="cuda")
            self.aux = torch.zeros(5, dtype=torch.int64, device="cuda")

    def __call__(self, slots, final=()):
        if self.kind == "text":
            self.s.push_dev(slots, [10] * len(slots), self.data, self.out, self.aux, final)
        else:
            self.s.push_dev(slots, [CHUNK] * len(slots), self.data, self.out, self.aux, final)
        self.torch.cuda.synchronize()
        if self.kind != "text":
            oo = self.aux.cpu().numpy()[: len(slots) + 1]
            assert oo[0] == 0 and np.all(np.diff(oo) >= 0) and oo[-1] <= ROWS


def _list_rules(call, valid):
    """`call(slots)` is one table-filling entry of a 3-slot set whose slots 0, 1, 2 are open; `valid` a list it takes."""
    a, b = valid[0], valid[-1]
    for bad in ([a, a], [a, b, a] if a != b else [a, a, a]):
        with pytest.raises(InvalidArgument, match="twice"):
            call(bad)
        call(valid)                                  # `seen` was cleared: the same slots pass
    for bad in ([a, 7], [7, a], [0xFFFFFFFF, a, 3]):
        with pytest.raises(InvalidArgument, match="out of range"):
            call(bad)
        call([a])
    with pytest.raises(InvalidArgument, match="in one"):
        call([0, 1, 2, 0])
    call(valid)


@pytest.mark.parametrize("kind", KINDS)
def test_slot_rules(gpu_ctx, torch_cuda, kind):
    s = _make(kind, gpu_ctx)
    assert [s.open(), s.open(), s.open()] == [0, 1, 2]
    with pytest.raises(InvalidArgument, match="slots are open"):
        s.open()
    s.close(1)
    assert s.open() == 1
    push = _Pusher(kind, s, torch_cuda)
    _list_rules(push, [0, 2])
    with pytest.raises(InvalidArgument, match="out of range"):      # the valid slot after the bad one is un-marked too
        push([1, 7])
    push([1])
    # a final push frees its slot
    push([0, 1], final={1})
    with pytest.raises(InvalidArgument, match="not open"):
        push([1])
    with pytest.raises(InvalidArgument, match="not open"):
        push([0, 1])
    push([0])
    assert s.open() == 1
    push([2, 1, 0])
    s.close(2)
    with pytest.raises(InvalidArgument, match="not open"):
        s.close(2)
    with pytest.raises(InvalidArgument, match="not open"):
        s.close(3)
    assert s.open() == 2
    s.destroy()


def test_haitsma_blocks_slot_rules(gpu_ctx, torch_cuda):
    torch = torch_cuda
    hs = _make("haitsma", gpu_ctx)
    assert [hs.open(), hs.open(), hs.open()] == [0, 1, 2]
    push = _Pusher("haitsma", hs, torch)
    d_out = torch.zeros(3 * 4, dtype=torch.int32, device="cuda")
    d_oo = torch.zeros(4, dtype=torch.int64, device="cuda")

    def blocks(slots):
        hs.blocks_dev(slots, d_out, d_oo)
        torch.cuda.synchronize()

    _list_rules(blocks, [0, 2])
    push([0, 2])                                     # the pushes share the tables and `seen` with the blocks calls
    _list_rules(blocks, [2, 1])
    hs.close(1)
    with pytest.raises(InvalidArgument, match="not open"):
        blocks([0, 1])
    blocks([0])
    hs.destroy()


def test_panako_windows_slot_rules_and_shared_tables(gpu_ctx, torch_cuda):
    """The windows calls and the pushes of a set fill the same two pinned tables in turn.  Each round below makes three
    table-filling calls (a push, two windows calls), so over four rounds either table is filled by either kind of call;
    the windows must still be the ring the pushes imply."""
    from ucfp_amd import audio
    torch = torch_cuda
    W = 64
    ps = _make("panako", gpu_ctx, window_frames=W)
    assert [ps.open(), ps.open(), ps.open()] == [0, 1, 2]
    d_rec = torch.zeros((3 * ps.window_cap, 4), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(4, dtype=torch.int64, device="cuda")

    def windows(slots):
        ps.windows_dev(slots, d_rec, d_off)
        torch.cuda.synchronize()

    _list_rules(windows, [0, 2])
    ps.close(1)
    with pytest.raises(InvalidArgument, match="not open"):
        windows([0, 1])
    windows([0])

    rng = np.random.default_rng(9)
    x = np.clip(0.2 * rng.standard_normal(4 * 8000), -0.9, 0.9).astype(np.float32)
    cfg = audio.PanakoConfig(target_zone_t=16)
    full = audio.panako_hashes(x, 8000, cfg, ctx=gpu_ctx)
    ta = full[:, 1].astype(np.int64)
    slot, other, n, nonempty = 2, 0, 0, 0
    for _ in range(4):
        got = ps.push({slot: x[n:n + 8000]})[slot]
        n += 8000
        F = ps.frontier(n)
        w0 = max(0, F - W)
        want = full[(ta >= w0) & (ta < F)].copy()
        want[:, 1:] -= np.uint32(w0)
        assert np.array_equal(got, full[(ta >= ps.frontier(n - 8000)) & (ta < F)])
        both = ps.windows([other, slot])
        assert both[slot][1] == w0 and np.array_equal(both[slot][0], want), (n, w0)
        assert both[other][0].shape == (0, 4) and both[other][1] == 0
        one = ps.windows([slot])[slot]
        assert one[1] == w0 and np.array_equal(one[0], want), (n, w0)
        nonempty += want.shape[0] > 0
    assert nonempty >= 2 and w0 > 0                  # the window moved and held records
    ps.destroy()
