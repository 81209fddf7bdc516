"""getNeighborPairsFrames: a batch of frames, every frame in its own box (neighbor_pairs_frames.h), against the single-system op by
bits and against the float64 restatement of pairs_frames_float64.  The two tests at the top need no GPU."""
import pytest
import torch

import pairs_frames_float64 as f64

DEV = torch.device("cuda:0")
C = f64.CUTOFF
DTYPES = [torch.float32, torch.float64]


def test_seeded_batches_keep_every_distance_clear_of_the_cutoff():
    for periodic in (True, False):
        assert f64.reference(*f64.batch(periodic))[4] > 1e-4


def test_frame_table_cuts_triangles_into_segments():
    from nnpops_amd import capi
    rows = capi.neighbor_pairs_frames_table([0, 0, 1, 3, 68, 68, 72]).tolist()
    P = f64.PART_PAIRS
    assert rows == [[2, 1, 2, 0, 1], [3, 3, 65, 0, P], [3, 3, 65, P, 1], [5, 68, 4, 0, 6]]
    for bad, word in (([1, 2], "start at 0"), ([0, 3, 2], "ascending"), ([], "at least one")):
        with pytest.raises((RuntimeError, ValueError), match=word):
            capi.neighbor_pairs_frames_table(bad)


@pytest.fixture(scope="module")
def ops():
    import NNPOps  # noqa: F401
    from NNPOps.neighbors import frame_table, getNeighborPairs, getNeighborPairsFrames
    return frame_table, getNeighborPairs, getNeighborPairsFrames


@pytest.fixture(scope="module", params=[True, False], ids=["boxes", "molecules"])
def case(request):
    """The seeded batch and its float64 list, computed once (and checked: pair sets have to agree exactly)."""
    pos, offsets, boxes = f64.batch(request.param)
    ref = f64.reference(pos, offsets, boxes)
    assert ref[4] > 1e-4
    return pos, offsets, boxes, ref


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _inputs(case, dtype, grad=False):
    pos, offsets, boxes, _ = case
    p = pos.to(DEV, dtype).requires_grad_(grad)
    b = None if boxes is None else boxes.to(DEV, dtype).requires_grad_(grad)
    return p, b


def _frame_slots(nb, a, b):
    return ((nb[0] >= a) & (nb[0] < b)).nonzero().flatten()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_frame_has_the_bits_of_the_single_system_op(ops, case, dtype):
    frame_table, single, frames = ops
    _, offsets, _, ref = case
    pos, boxes = _inputs(case, dtype)
    table, true = frame_table(offsets, DEV), ref[0].numel()
    full = frames(pos, C, table, -1, boxes)
    tight = frames(pos, C, table, true, boxes)
    short = frames(pos, C, table, true - 1, boxes)
    assert int(full[3]) == int(tight[3]) == int(short[3]) == true
    assert (tight[0] >= 0).all() and torch.equal(tight[0][0].cpu().long(), ref[0]) and torch.equal(tight[0][1].cpu().long(), ref[1])
    # the surplus pair is the last one: dropped, and nothing else moves
    assert torch.equal(short[0], tight[0][:, :-1]) and _same(short[1], tight[1][:-1]) and _same(short[2], tight[2][:-1])
    base = 0
    for m, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b == a:
            continue
        box = None if boxes is None else boxes[m]
        tri = (b - a) * (b - a - 1) // 2
        nb, dl, ds, cnt = single(pos[a:b], C, -1, box)
        got = full[0][:, base:base + tri]
        assert torch.equal(torch.where(got >= 0, got - a, got), nb) and _same(full[1][base:base + tri], dl) and _same(full[2][base:base + tri], ds)
        base += tri
        k = _frame_slots(tight[0], a, b)
        assert k.numel() == int(cnt)
        if k.numel():
            nb, dl, ds, _ = single(pos[a:b], C, k.numel(), box)
            assert torch.equal(tight[0][:, k] - a, nb) and _same(tight[1][k], dl) and _same(tight[2][k], ds)
    # the batch reversed, and frames given alone: a frame's bits stay
    order = list(range(len(offsets) - 1))[::-1]
    rpos = torch.cat([pos[offsets[m]:offsets[m + 1]] for m in order])
    roff = [0]
    for m in order:
        roff.append(roff[-1] + offsets[m + 1] - offsets[m])
    rev = frames(rpos, C, frame_table(roff, DEV), true, None if boxes is None else boxes[order].contiguous())
    for q, m in enumerate(order):
        a, b = offsets[m], offsets[m + 1]
        k, kr = _frame_slots(tight[0], a, b), _frame_slots(rev[0], roff[q], roff[q + 1])
        assert torch.equal(tight[0][:, k] - a, rev[0][:, kr] - roff[q]) and _same(tight[1][k], rev[1][kr]) and _same(tight[2][k], rev[2][kr])
        if b - a in (65, f64.LDS_ATOMS + 1):
            alone = frames(pos[a:b].contiguous(), C, frame_table([0, b - a], DEV), k.numel(), None if boxes is None else boxes[m:m + 1])
            assert torch.equal(tight[0][:, k] - a, alone[0]) and _same(tight[1][k], alone[1]) and _same(tight[2][k], alone[2])


def _step(frames, pos, table, slots, boxes):
    _, dl, ds, _ = frames(pos, C, table, slots, boxes)
    keep = ds == ds
    return f64.energy(dl[keep], ds[keep])


def _close(got, want, tol=1e-4):
    return float((got.detach().cpu().double() - want).abs().max()) <= tol * float(want.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [-1, 0], ids=["all-slots", "compacted"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_values_and_gradients_against_float64(ops, case, dtype, slots):
    frame_table, single, frames = ops
    pos64, offsets, boxes64, ref = case
    table = frame_table(offsets, DEV)
    slots = slots if slots else ref[0].numel() + 5
    pos, boxes = _inputs(case, dtype, grad=True)
    nb, dl, ds, cnt = frames(pos, C, table, slots, boxes)
    k = (nb[0] >= 0).nonzero().flatten()
    assert int(cnt) == ref[0].numel() and torch.equal(nb[0][k].cpu().long(), ref[0]) and torch.equal(nb[1][k].cpu().long(), ref[1])
    # float32: the bars of tests/test_neighbor_pairs_gpu.py (test_periodic with boxes, test_values without)
    rtol = 1e-12 if dtype == torch.float64 else (2e-5 if boxes is not None else 1e-6)
    atol = 1e-5 if dtype == torch.float32 and boxes is not None else 0.0
    torch.testing.assert_close(ds[k].detach().cpu().double(), ref[3], rtol=rtol, atol=0.0)
    torch.testing.assert_close(dl[k].detach().cpu().double(), ref[2], rtol=rtol, atol=max(atol, 1e-12 * float(ref[2].abs().max())))
    # first derivatives of a smooth scalar, float64 autograd through the restatement as the judge
    p64 = pos64.clone().requires_grad_()
    b64 = None if boxes64 is None else boxes64.clone().requires_grad_()
    r = f64.reference(p64, offsets, b64)
    want = torch.autograd.grad(f64.energy(r[2], r[3]), [p64] if b64 is None else [p64, b64])
    leaves = [pos] if boxes is None else [pos, boxes]
    got = torch.autograd.grad(_step(frames, pos, table, slots, boxes), leaves)
    again = torch.autograd.grad(_step(frames, pos, table, slots, boxes), leaves)
    assert all(_same(x, y) for x, y in zip(got, again))                     # repeated backward calls: equal bits
    assert all(_close(x, y) for x, y in zip(got, want))
    if boxes is not None:
        # Against the single-system op's box gradient of the frame alone: within the bar, not by bits -- both add the same terms in
        # float64, but the single-system pass strides its whole list over fixed blocks while a frame's segments are added one by one.
        assert got[1].shape == (len(offsets) - 1, 3, 3) and got[1].dtype == dtype
        for m in (3, 6, 7):
            a, b = offsets[m], offsets[m + 1]
            p1, b1 = pos[a:b].detach().requires_grad_(), boxes[m].detach().requires_grad_()
            _, d1, r1, _ = single(p1, C, -1 if slots < 0 else (b - a) * (b - a - 1) // 2, b1)
            keep = r1 == r1
            alone = torch.autograd.grad(f64.energy(d1[keep], r1[keep]), b1)[0]
            assert _close(got[1][m], alone.detach().cpu().double())
    # a force-loss step: the box does not require a gradient
    fixed = None if boxes is None else boxes.detach()
    force = torch.autograd.grad(_step(frames, pos, table, slots, fixed), pos, create_graph=True)[0]
    got2 = torch.autograd.grad((force ** 2).sum(), pos)[0]
    fixed64 = None if b64 is None else b64.detach()
    r = f64.reference(p64, offsets, fixed64)
    force64 = torch.autograd.grad(f64.energy(r[2], r[3]), p64, create_graph=True)[0]
    assert _close(force, force64.detach()) and _close(got2, torch.autograd.grad((force64 ** 2).sum(), p64)[0])
    if boxes is not None:
        with pytest.raises(RuntimeError, match="second derivatives that involve the box are not available for frames"):
            torch.autograd.grad(_step(frames, pos, table, slots, boxes), leaves, create_graph=True)


@pytest.mark.gpu
def test_forward_and_backward_replay_in_a_captured_graph(ops, case):
    frame_table, _, frames = ops
    _, offsets, _, ref = case
    table = frame_table(offsets, DEV)
    static_pos, boxes = _inputs(case, torch.float32, grad=True)
    leaves = [static_pos] if boxes is None else [static_pos, boxes]

    def step(lv):
        _, dl, ds, _ = frames(lv[0], C, table, ref[0].numel() + 64, lv[1] if len(lv) > 1 else None)
        keep = ds == ds                                                     # (no boolean indexing: it would read the mask back)
        far = torch.full_like(ds, 1e3)
        return torch.autograd.grad(f64.energy(torch.where(keep[:, None], dl, torch.zeros_like(dl)), torch.where(keep, ds, far)), lv)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(leaves)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(leaves)
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        with torch.no_grad():
            static_pos.add_((0.01 * torch.randn(static_pos.shape, generator=g)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        eager = step([t.detach().clone().requires_grad_() for t in leaves])
        assert all(_same(x, y) for x, y in zip(captured, eager)) and float(eager[0].abs().max()) > 0


@pytest.mark.gpu
def test_refusals(ops, case):
    frame_table, _, frames = ops
    _, offsets, _, ref = case
    pos, boxes = _inputs(case, torch.float32)
    table = frame_table(offsets, DEV)
    with pytest.raises(RuntimeError, match="Too many neighbor pairs found"):
        frames(pos, C, table, ref[0].numel() - 1, boxes, check_errors=True)
    big = torch.zeros(2 * 46342, 3, device=DEV)                             # two triangles of 46342 atoms: more than 2^31 - 1 slots
    refused = [
        (pos, table[:, :4].contiguous(), boxes, r'Expected "table" to have shape'),
        (pos, table.long(), boxes, r'Expected "table" to be int32'),
        (pos, table.clone(), boxes, r'Expected "table" to be a tensor that frame_table returned'),
        (pos[:-1].contiguous(), table, boxes, r'Expected the last offset of "table" \(\d+\) to be the 1st dimension size of "positions"'),
        (big, frame_table([0, 46342, 2 * 46342], DEV), None, "Too many pair slots"),
    ]
    if boxes is not None:
        refused.append((pos, table, boxes[:-1].contiguous(), r'Expected the 1st dimension size of "box_vectors" \(8\) to be the number of frames'))
    for p, t, b, message in refused:
        with pytest.raises(RuntimeError, match=message):
            frames(p, C, t, -1, b)
    with pytest.raises(RuntimeError, match="Too many atoms"):
        frame_table([0, 2 ** 31], DEV)
