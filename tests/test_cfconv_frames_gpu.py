"""CFConv periodic batches on the device: B periodic frames behind one neighbour list, every frame in its own box
(nnpops_cfconv_neighbors_set_frames / Holder.set_frames / CFConvNeighbors.set_frames).

Batches and judge: tests/cfconv_frames_float64.py (pinned by tests/test_cfconv_frames_reference_cpu.py).  The judge evaluates one frame
at a time in that frame's box; no intra-frame distance is within 1e-4 A of the cutoff (3 A), so the exact list comparisons are
unambiguous.
    ragged    frames of 1, 2, 21, 64, 65 and 7 atoms on top of each other, boxes from 2.12 to 3.9 cutoffs wide, one triclinic, one frame
              wrapped, one a box vector outside its box
    many      70 frames of 1 ... 9 atoms
    crowded   a 190-atom frame whose rows outgrow the first capacity of 64 (check() grows, build again)
    long      257 and 300 atoms: the per-frame stride of the box pass (256 atoms) goes round a second time
Bars: OUT_RTOL / OUT_ATOL_FRAC / FORCE_RTOL of tests/cfconv_float64.py for compute and backprop; the box gradient by
box_gradient_judge.judge frame by frame at FORCE_RTOL = 1e-4 of the frame's largest entry, as tests/test_cfconv_box_gradient_gpu.py
(the antisymmetric part of every frame's stress to the same bar); 1e-4 of an array's largest entry for the second derivatives, the
weight gradients and the force-loss steps (the project's bar for CFConv gradients, cfconv_weights_float64.BAR).  Distances of the
exported list: float32 rounding of three differences and three image shifts at the magnitude of the coordinates and the box,
8 eps32 (|x|max + |B|max).  Every evaluation prints its measured figures (pytest -s).

Layers (the kernels behind them asserted through nnpops_cfconv_describe):
    split-registers   W 32, G 16   both layers split-fp16, register-fed; pair slots, box pass ROW_S = false
    split-planes      W 32, G 70   layer 2 through LDS planes
    valu              W 32, G 16, NNPOPS_CFCONV_VALU=1: the vector kernel and its second walk; box pass ROW_S = true

Measured on an MI355X: see docs/LAB_NOTEBOOK_cfconv_frames.md.
"""
import numpy as np
import pytest
import torch

import cfconv_force_weights_float64 as ff
import cfconv_frames_float64 as frames
import cfconv_weights_float64 as wf
from box_gradient_judge import clean_env, judge as judge_box
from cfconv_float64 import FORCE_RTOL, OUT_ATOL_FRAC, OUT_RTOL, SecondOrder, sigma_of, weights

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 1e-4
CUTOFF = frames.CUTOFF

LAYERS = {                     # name: (W, G, activation, environment, path of nnpops_cfconv_describe)
    "split-registers": (32, 16, "ssp", {}, "split_registers"),
    "split-planes": (32, 70, "tanh", {}, "split_planes"),
    "valu": (32, 16, "ssp", {"NNPOPS_CFCONV_VALU": "1"}, "vector"),
}


def _env(monkeypatch, name):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    for k, v in LAYERS[name][3].items():
        monkeypatch.setenv(k, v)


def _dev(*arrays):
    out = [None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV) for a in arrays]
    return out if len(out) > 1 else out[0]


def _list(n, offsets=None, cutoff=CUTOFF):
    from nnpops_amd.capi import CFConvNeighbors
    nb = CFConvNeighbors(n, cutoff, True)
    if offsets is not None:
        nb.set_frames(offsets)
    return nb


def _conv(tag, name, n=None):
    from nnpops_amd.capi import CFConv
    W, G, act, _, path = LAYERS[name]
    w1, b1, w2, b2 = frames.batch_layer(tag, W, G)[:4]
    cf = CFConv(len(frames.batch(tag)[0]) if n is None else n, W, G, CUTOFF, sigma_of(G), act, w1, b1, w2, b2, periodic=True)
    assert cf.describe()["path"] == path, cf.describe()
    return cf


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _run(nb, cf, pos, boxes, x, gy):
    """build, compute, backprop_box -> [out, gx, gp, gbox] (clones)"""
    tpos, tbox, tx, tg = _dev(pos, boxes, x, gy)
    nb.build(tpos, tbox)
    res = [cf.compute(nb, tpos, tx, tbox).clone(), *[t.clone() for t in cf.backprop_box(nb, tpos, tx, tg, tbox)]]
    torch.cuda.synchronize()
    return res


# ---------------------------------------------------------------------------------------------- the list
@pytest.mark.parametrize("tag", frames.TAGS)
def test_list_is_the_judges(tag):
    pos, boxes, offsets, _ = frames.batch(tag)
    nb = _list(len(pos), offsets)
    nb.build(*_dev(pos, boxes))
    atoms, dist = nb.export()
    i, j, d, _ = frames.half_pairs(pos, boxes, offsets)
    assert nb.num_pairs() == len(i)
    assert np.array_equal(atoms[0], i) and np.array_equal(atoms[1], j)
    r = np.sqrt((d * d).sum(axis=1))
    tol = 8 * float(np.finfo(np.float32).eps) * (float(np.abs(pos).max()) + float(np.abs(boxes).max()))
    err = float(np.abs(dist.astype(np.float64) - r).max())
    print(f"\n[cfconv-frames] {tag}: {len(i)} pairs, distances within {err:.2e} A of float64 (bound {tol:.2e})")
    assert err <= tol


# ---------------------------------------------------------------------------------------------- values
def _check_first(out, gx, gp, ref):
    out, gx, gp = (t.cpu().numpy().astype(np.float64) for t in (out, gx, gp))
    errs = [np.abs(a - ref[k]).max() / np.abs(ref[k]).max() for a, k in ((out, "out"), (gx, "gx"), (gp, "g"))]
    print(f"  out {errs[0]:.2e} gx {errs[1]:.2e} gp {errs[2]:.2e} of max")
    np.testing.assert_allclose(out, ref["out"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(ref["out"]).max())
    np.testing.assert_allclose(gx, ref["gx"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(ref["gx"]).max())
    assert np.abs(gp - ref["g"]).max() <= FORCE_RTOL * np.abs(ref["g"]).max()
    return errs


def _check_box(label, pos, boxes, offsets, ref, gp, gbox):
    """every frame's nine entries by box_gradient_judge.judge; exact zeros where float64 has them"""
    gp, gbox = gp.cpu().numpy().astype(np.float64), gbox.cpu().numpy().astype(np.float64)
    assert gbox.shape == ref["gbox"].shape
    zeros = ref["gbox"] == 0
    assert not gbox[zeros].any(), "an entry that is an exact zero in float64 is not one here"
    judged = 0
    for m, (lo, hi) in enumerate(frames.segments(offsets)):
        if not ref["gbox"][m].any():
            continue                                         # a lone atom, or no pair through a face: exact zeros, asserted above
        sub = dict(g=ref["g"][lo:hi], gbox=ref["gbox"][m])
        judge_box("cfconv-frames", f"{label} frame {m} ({hi - lo} atoms)", pos[lo:hi], boxes[m], sub, gp[lo:hi], gbox[m], FORCE_RTOL)
        judged += 1
    return judged


VALUE_CASES = [(name, tag) for name in LAYERS for tag in ("ragged", "many", "long")] + [("split-registers", "crowded")]


@pytest.mark.parametrize("name,tag", VALUE_CASES, ids=[f"{n}-{t}" for n, t in VALUE_CASES])
def test_values_against_float64(monkeypatch, name, tag):
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    pos, boxes, offsets, _ = frames.batch(tag)
    x, gy = frames.batch_layer(tag, W, G)[4:6]
    ref = frames.reference(tag, W, G, act)
    nb, cf = _list(len(pos), offsets), _conv(tag, name)
    out, gx, gp, gbox = _run(nb, cf, pos, boxes, x, gy)
    atoms, _ = nb.export()
    assert np.array_equal(atoms[0], ref["i"]) and np.array_equal(atoms[1], ref["j"])
    tpos, tbox, tx, tg = _dev(pos, boxes, x, gy)
    plain = cf.backprop(nb, tpos, tx, tg, tbox)
    again = [cf.compute(nb, tpos, tx, tbox), *cf.backprop_box(nb, tpos, tx, tg, tbox)]
    torch.cuda.synchronize()
    for a, b in zip([out, gx, gp, gbox], again):
        assert _same_bits(a, b), "two calls give different bits"
    assert _same_bits(gx, plain[0]) and _same_bits(gp, plain[1]), "backprop_box does not return the plain backprop()'s gradients"
    print(f"\n[cfconv-frames] {name} W={W} G={G} {act} {tag}:")
    _check_first(out, gx, gp, ref)
    assert gbox.shape == (len(offsets) - 1, 3, 3) and gbox.dtype == torch.float32
    assert _check_box(f"{name} {tag}", pos, boxes, offsets, ref, gp, gbox) >= 2
    for m, (lo, hi) in enumerate(frames.segments(offsets)):
        if hi - lo == 1:                                     # a lone atom: exact zeros everywhere
            assert not out[lo].any() and not gx[lo].any() and not gp[lo].any() and not gbox[m].any()


# ---------------------------------------------------------------------------------------------- bit-equality
BITS = ["split-registers", "valu"]


@pytest.mark.parametrize("name", BITS)
def test_a_frame_alone_and_in_company(monkeypatch, name):
    """the 21-, 64- and 65-atom frames of `ragged`, each behind a list of its own with set_frames([0, n]): output, both gradients and
    the nine box entries have the bits they have in the batch; and against a plain single-system periodic list (all-pairs build) the
    output and both gradients keep their bits, the box gradient -- summed in another order -- agrees to the bar"""
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    pos, boxes, offsets, _ = frames.batch("ragged")
    x, gy = frames.batch_layer("ragged", W, G)[4:6]
    whole = _run(_list(len(pos), offsets), _conv("ragged", name), pos, boxes, x, gy)
    for m in (2, 3, 4):
        lo, hi = frames.segments(offsets)[m]
        n = hi - lo
        alone = _run(_list(n, [0, n]), _conv("ragged", name, n=n), pos[lo:hi], boxes[m:m + 1], x[lo:hi], gy[lo:hi])
        for k in range(3):
            assert _same_bits(whole[k][lo:hi], alone[k]), (m, k)
        assert _same_bits(whole[3][m], alone[3][0]), m
        plain = _run(_list(n), _conv("ragged", name, n=n), pos[lo:hi], boxes[m], x[lo:hi], gy[lo:hi])
        for k in range(3):
            assert _same_bits(alone[k], plain[k]), (m, k)
        assert plain[3].shape == (3, 3)
        a, b = alone[3][0].cpu().numpy().astype(np.float64), plain[3].cpu().numpy().astype(np.float64)
        assert np.abs(a - b).max() <= FORCE_RTOL * np.abs(b).max() and np.abs(b).max() > 0


@pytest.mark.parametrize("name", BITS)
def test_many_in_reversed_order(monkeypatch, name):
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    pos, boxes, offsets, _ = frames.batch("many")
    x, gy = frames.batch_layer("many", W, G)[4:6]
    base = _run(_list(len(pos), offsets), _conv("many", name), pos, boxes, x, gy)
    order = list(range(len(offsets) - 1))[::-1]
    rpos, rboxes, roffsets, rows, rx, rgy = frames.reorder(pos, boxes, offsets, order, x, gy)
    got = _run(_list(len(pos), roffsets), _conv("many", name), rpos, rboxes, rx, rgy)
    at = torch.tensor(rows, device=DEV)
    for k in range(3):
        assert _same_bits(base[k][at], got[k]), k
    assert _same_bits(base[3][torch.tensor(order, device=DEV)], got[3])
    assert float(base[3].abs().max()) > 0


# ---------------------------------------------------------------------------------------------- handles
def test_a_handle_partitioned_again_gives_the_bits_of_a_fresh_one(monkeypatch):
    """70 -> 35 -> 70 frames, then back to one system: every time what a fresh handle gives.  (35: neighbouring frames two by two under
    the box of the first; one system: all the atoms under the first frame's box -- compared with fresh handles, not judged)"""
    name = "split-registers"
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    pos, boxes, offsets, _ = frames.batch("many")
    x, gy = frames.batch_layer("many", W, G)[4:6]
    n = len(pos)
    half_boxes, half_offsets = np.ascontiguousarray(boxes[0::2]), np.ascontiguousarray(offsets[0::2])
    assert len(half_offsets) == 36 and half_offsets[-1] == n
    nb, cf = _list(n), _conv("many", name)
    seen = []
    for off, bx in ((offsets, boxes), (half_offsets, half_boxes), (offsets, boxes), (None, boxes[0])):
        nb.set_frames(off)
        assert nb.build_count() == 0                         # the call invalidates the current build
        got = _run(nb, cf, pos, bx, x, gy)
        fresh = _run(_list(n, off), _conv("many", name), pos, bx, x, gy)
        assert got[3].shape == fresh[3].shape == ((len(off) - 1, 3, 3) if off is not None else (3, 3))
        for a, b in zip(got, fresh):
            assert _same_bits(a, b)
        seen.append(got)
    assert all(_same_bits(a, b) for a, b in zip(seen[0], seen[2]))
    assert not _same_bits(seen[0][0], seen[1][0]) and not _same_bits(seen[0][0], seen[3][0])       # (the partitions do differ)


def test_crowded_grows_through_check(monkeypatch):
    from nnpops_amd.capi import NNPOpsHipError
    name = "split-registers"
    _env(monkeypatch, name)
    pos, boxes, offsets, _ = frames.batch("crowded")
    nb = _list(len(pos), offsets)
    tpos, tbox = _dev(pos, boxes)
    nb.build(tpos, tbox, check=False)
    with pytest.raises(NNPOpsHipError, match="neighbour rows overflowed"):
        nb.num_pairs()
    nb.build(tpos, tbox)
    i, j, _, _ = frames.half_pairs(pos, boxes, offsets)
    atoms, _ = nb.export()
    assert np.array_equal(atoms[0], i) and np.array_equal(atoms[1], j)
    assert int(np.bincount(np.concatenate([i, j])).max()) > 64


# ---------------------------------------------------------------------------------------------- the kernels that work from the rows
def _rel(got, ref):
    top = float(np.abs(ref).max())
    assert top > 0
    return float(np.abs(got.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref).max()) / top


@pytest.mark.parametrize("name", ["split-registers", "valu"])
def test_unchanged_kernels_on_a_periodic_batch(monkeypatch, name):
    """double_backward, backprop_weights and double_backward_weights on `ragged` against their float64 judges, frame by frame"""
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    tag = "ragged"
    pos, boxes, offsets, _ = frames.batch(tag)
    x, gy, V, Q = frames.batch_layer(tag, W, G)[4:]
    J = frames.judge_of(tag, W, G, act)
    nb, cf = _list(len(pos), offsets), _conv(tag, name)
    tpos, tbox, tx, tg, tV, tQ = _dev(pos, boxes, x, gy, V, Q)
    nb.build(tpos, tbox)
    cf.compute(nb, tpos, tx, tbox)
    ref2 = frames.second(J, pos, boxes, offsets, x, gy, V, Q)
    e2 = [_rel(t, ref2[k]) for t, k in zip(cf.double_backward(nb, tpos, tx, tg, tV, tQ), ("dg", "dx", "dp"))]
    i, j, d, _ = frames.half_pairs(pos, boxes, offsets)
    refw = wf.judge(J, i, j, np.sqrt((d * d).sum(axis=1)), x, gy)
    ew = [_rel(t, refw[k]) for t, k in zip(cf.backprop_weights(nb, tx, tg), wf.NAMES)]
    reffw = ff.judge(J, i, j, d, x, gy, V, Q)
    efw = [_rel(t, reffw[k]) for t, k in zip(cf.double_backward_weights(nb, tx, tg, tV, tQ), ff.NAMES)]
    print(f"\n[cfconv-frames] {name} ragged: double backward {max(e2):.2e}, weight gradients {max(ew):.2e}, force-loss weight gradients "
          f"{max(efw):.2e} of max")
    assert max(e2) <= BAR and max(ew) <= BAR and max(efw) <= BAR


# ---------------------------------------------------------------------------------------------- the C ABI's refusals
def test_c_abi_refusals():
    from nnpops_amd.capi import CFConvNeighbors, NNPOpsHipError
    pos, boxes, offsets, _ = frames.batch("ragged")
    n = len(pos)
    tpos, tbox = _dev(pos, boxes)
    with pytest.raises(NNPOpsHipError, match="created non-periodic"):
        CFConvNeighbors(n, CUTOFF, False).set_frames(offsets)
    nb = _list(n)
    with pytest.raises(NNPOpsHipError, match="start at 0 and end at num_atoms"):
        nb.set_frames([1, 50, n])
    with pytest.raises(NNPOpsHipError, match="start at 0 and end at num_atoms"):
        nb.set_frames([0, 50, n - 1])
    with pytest.raises(NNPOpsHipError, match="empty or offsets are not increasing"):
        nb.set_frames([0, 50, 50, n])
    with pytest.raises(NNPOpsHipError, match="empty or offsets are not increasing"):
        nb.set_frames([0, 90, 50, n])
    with pytest.raises(NNPOpsHipError, match="empty or offsets are not increasing"):
        nb.set_frames([0, n + 5, n])                         # (never indexes beyond the table)
    # a refused call changed nothing: still one system
    nb.build(tpos, tbox[4])
    fresh = _list(n)
    fresh.build(tpos, tbox[4])
    assert np.array_equal(nb.export()[0], fresh.export()[0])
    nb.set_frames(offsets)
    with pytest.raises(NNPOpsHipError, match="needs the box vectors of every frame"):
        nb.build(tpos, None)
    with pytest.raises(ValueError, match="shape"):
        nb.build(tpos, tbox[0])                              # capi: a (3, 3) box on a list of frames
    # frames together with molecules: a handle is periodic or not for life, and each call refuses the other kind
    with pytest.raises(NNPOpsHipError, match="non-periodic"):
        nb.set_molecules(offsets)
    with pytest.raises(NNPOpsHipError, match="non-periodic"):
        CFConvNeighbors(n, CUTOFF, True).set_molecules(offsets)          # ... as it always did
    batched = CFConvNeighbors(n, CUTOFF, False)
    batched.set_molecules(offsets)
    with pytest.raises(NNPOpsHipError, match="created non-periodic"):
        batched.set_frames(offsets)
    nb.build(tpos, tbox)                                     # the handle is still good
    assert nb.num_pairs() == len(frames.half_pairs(pos, boxes, offsets)[0])


# ---------------------------------------------------------------------------------------------- the torch surface
def _module(name, weights4, **kw):
    from NNPOps.CFConv import CFConv
    W, G, act = LAYERS[name][:3]
    w1, b1, w2, b2 = (torch.tensor(w) for w in weights4)
    return CFConv(sigma_of(G), act, w1.reshape(G, W), b1, w2, b2, **kw)      # weights1: the core's [W][G] buffer seen as [G, W]


def _neighbors(offsets):
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    nb = CFConvNeighbors(CUTOFF)
    nb.set_frames([int(v) for v in offsets])
    return nb


def _leaf(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV, requires_grad=True)


@pytest.mark.parametrize("name", ["split-registers", "valu"])
def test_module_gives_the_bits_of_the_c_abi(monkeypatch, name):
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    tag = "ragged"
    pos, boxes, offsets, _ = frames.batch(tag)
    w1, b1, w2, b2, x, gy = frames.batch_layer(tag, W, G)[:6]
    ref = frames.reference(tag, W, G, act)
    abi = _run(_list(len(pos), offsets), _conv(tag, name), pos, boxes, x, gy)
    nb, conv = _neighbors(offsets), _module(name, (w1, b1, w2, b2))
    tpos, tx, tbox = _leaf(pos), _leaf(x), _leaf(boxes)
    nb.build(tpos, tbox)
    out = conv(nb, tpos, tx, tbox)
    (out * _dev(gy)).sum().backward()
    assert tbox.grad is not None and tbox.grad.shape == (len(offsets) - 1, 3, 3) and tbox.grad.dtype == torch.float32
    for a, b in zip(abi, (out, tx.grad, tpos.grad, tbox.grad)):
        assert _same_bits(a, b)
    print(f"\n[cfconv-frames] torch {name} {tag}:")
    _check_first(out.detach(), tx.grad, tpos.grad, ref)
    _check_box(f"torch {name} {tag}", pos, boxes, offsets, ref, tpos.grad, tbox.grad)
    # every frame's stress (x^T dL/dx + B^T dL/dB) / V is symmetric to the bar
    for m, (anti, top) in enumerate(frames.stress_antisymmetry(pos, boxes, offsets, tpos.grad.cpu().numpy(), tbox.grad.cpu().numpy())):
        assert anti <= FORCE_RTOL * top or top == 0, (m, anti, top)
    # a box that does not require a gradient gets none, and the other results keep their bits
    tpos2, tx2 = _leaf(pos), _leaf(x)
    plain_box = _dev(boxes)
    out2 = conv(nb, tpos2, tx2, plain_box)
    (out2 * _dev(gy)).sum().backward()
    assert plain_box.grad is None and _same_bits(out2, out) and _same_bits(tpos2.grad, tpos.grad) and _same_bits(tx2.grad, tx.grad)


def _frozen_lists(J, pos, boxes, offsets):
    i, j, d, _ = frames.half_pairs(pos, boxes, offsets)
    p64 = pos.astype(np.float64)
    return i, j, d - (p64[j] - p64[i])


@pytest.mark.parametrize("name", ["split-registers", "valu"])
def test_force_loss_step_through_two_twice_differentiable_layers(monkeypatch, name):
    """two stacked layers behind a linear layer on one list of frames: the gradients of |F - F0|^2 in the linear weight, the positions
    and the input against float64 over the frames' own pair lists with frozen shifts"""
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    tag = "ragged"
    pos, boxes, offsets, _ = frames.batch(tag)
    x, gy, _, Q = frames.batch_layer(tag, W, G)[4:]
    readout, f_ref = (0.1 * gy).astype(np.float32), (0.1 * Q).astype(np.float32)
    la, lb = weights(W, G, 1, 41)[:4], weights(W, G, 1, 42)[:4]
    conv1, conv2 = _module(name, la, twice_differentiable=True), _module(name, lb, twice_differentiable=True)
    torch.manual_seed(5)
    linear = torch.nn.Linear(W, W, bias=False).to(DEV)
    nb = _neighbors(offsets)
    tpos, tx, tbox = _leaf(pos), _leaf(x), _dev(boxes)
    nb.build(tpos, tbox)
    energy = (conv2(nb, tpos, 0.1 * conv1(nb, tpos, linear(tx), tbox), tbox) * _dev(readout)).sum()
    force, = torch.autograd.grad(energy, tpos, create_graph=True)
    gw, gp, gx = torch.autograd.grad(((force - _dev(f_ref)) ** 2).sum(), [linear.weight, tpos, tx])
    # float64
    wide = lambda a: torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))
    from cfconv_float64 import Restatement
    j1, j2 = Restatement(W, G, CUTOFF, sigma_of(G), act, *la), Restatement(W, G, CUTOFF, sigma_of(G), act, *lb)
    i, j, shift = _frozen_lists(j1, pos, boxes, offsets)
    so1, so2 = SecondOrder(j1, i, j, shift), SecondOrder(j2, i, j, shift)
    w = wide(linear.weight.detach().cpu().numpy()).requires_grad_(True)
    p, xin = wide(pos).requires_grad_(True), wide(x).requires_grad_(True)
    e64 = (so2.forward(p, 0.1 * so1.forward(p, xin @ w.T)) * wide(readout)).sum()
    f64, = torch.autograd.grad(e64, p, create_graph=True)
    rw, rp, rx = torch.autograd.grad(((f64 - wide(f_ref)) ** 2).sum(), [w, p, xin])
    errs = [_rel(force.detach(), f64.detach().numpy()), _rel(gw, rw.numpy()), _rel(gp, rp.numpy()), _rel(gx, rx.numpy())]
    print(f"\n[cfconv-frames] force-loss step {name}: force {errs[0]:.2e}, d/dweight {errs[1]:.2e}, d/dpositions {errs[2]:.2e}, "
          f"d/dinput {errs[3]:.2e} of max")
    assert max(errs) <= BAR


def _param_grads(conv, W, G):
    return dict(w1=conv.weights1.grad.cpu().numpy().reshape(W, G), b1=conv.biases1.grad.cpu().numpy(),
                w2=conv.weights2.grad.cpu().numpy(), b2=conv.biases2.grad.cpu().numpy())


def test_force_loss_step_with_force_trainable(monkeypatch):
    """(E - E0)^2 + |F - F0|^2 through one force_trainable layer on a list of frames: every parameter gradient against float64"""
    name = "split-registers"
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    tag = "ragged"
    pos, boxes, offsets, _ = frames.batch(tag)
    w1, b1, w2, b2, x, gy = frames.batch_layer(tag, W, G)[:6]
    readout = (0.1 * gy).astype(np.float32)
    J = frames.judge_of(tag, W, G, act)
    i, j, shift = _frozen_lists(J, pos, boxes, offsets)
    start = [wf._wide(a) for a in (w1, b1, w2, b2)]
    _, E, F = ff.force_loss(J, start, i, j, pos, x, readout, 0.0, np.zeros((len(pos), 3), np.float32), shift)
    E0, F0 = float(np.float32(0.5 * float(E.detach()))), (0.5 * F.detach().numpy()).astype(np.float32)
    params = [p.clone().requires_grad_(True) for p in start]
    ref = torch.autograd.grad(ff.force_loss(J, params, i, j, pos, x, readout, E0, F0, shift)[0], params)
    conv = _module(name, (w1, b1, w2, b2), force_trainable=True).to(DEV)
    nb = _neighbors(offsets)
    tpos, tbox = _leaf(pos), _dev(boxes)
    nb.build(tpos, tbox)
    Eg = (conv(nb, tpos, _dev(x), tbox) * _dev(readout)).sum()
    Fg = -torch.autograd.grad(Eg, tpos, create_graph=True)[0]
    ((Eg - E0) ** 2 + ((Fg - _dev(F0)) ** 2).sum()).backward()
    err = ff.errors(_param_grads(conv, W, G), {n: v.numpy() for n, v in zip(ff.NAMES, ref)})
    print(f"\n[cfconv-frames] force_trainable step: {ff.figures(err)}")
    assert max(err.values()) <= BAR


def test_trainable_parameter_gradients_with_the_box_gradient_in_one_backward(monkeypatch):
    name = "split-registers"
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    tag = "ragged"
    pos, boxes, offsets, _ = frames.batch(tag)
    w1, b1, w2, b2, x, gy = frames.batch_layer(tag, W, G)[:6]
    ref = frames.reference(tag, W, G, act)
    J = frames.judge_of(tag, W, G, act)
    i, j, d, _ = frames.half_pairs(pos, boxes, offsets)
    refw = wf.judge(J, i, j, np.sqrt((d * d).sum(axis=1)), x, gy)
    conv = _module(name, (w1, b1, w2, b2), trainable=True).to(DEV)
    nb = _neighbors(offsets)
    tpos, tx, tbox = _leaf(pos), _leaf(x), _leaf(boxes)
    nb.build(tpos, tbox)
    (conv(nb, tpos, tx, tbox) * _dev(gy)).sum().backward()
    err = wf.errors(_param_grads(conv, W, G), refw)
    print(f"\n[cfconv-frames] trainable: {wf.figures(err)}")
    assert max(err.values()) <= BAR
    assert tbox.grad.shape == (len(offsets) - 1, 3, 3)
    _check_box("trainable ragged", pos, boxes, offsets, ref, tpos.grad, tbox.grad)


def test_step_with_the_box_gradient_replays_in_a_captured_graph(monkeypatch):
    """build + forward + backward with box.grad captured after warm-up steps (they settle the row capacity and size the scratch) and
    replayed on moved positions: the eager result, bit for bit"""
    name = "split-registers"
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    tag = "long"
    pos, boxes, offsets, _ = frames.batch(tag)
    w1, b1, w2, b2, x, gy = frames.batch_layer(tag, W, G)[:6]
    nb, conv = _neighbors(offsets), _module(name, (w1, b1, w2, b2))
    tbox, tx, tg = _leaf(boxes), _leaf(x), _dev(gy)
    static_pos = _leaf(pos)

    def step(p):
        nb.build(p, tbox)
        return torch.autograd.grad((conv(nb, p, tx, tbox) * tg).sum(), [p, tx, tbox])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(static_pos)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_pos, g_x, g_box = step(static_pos)
    rng = np.random.default_rng(1)
    for _ in range(2):
        new = (pos + rng.normal(0, 0.02, pos.shape)).astype(np.float32)
        with torch.no_grad():
            static_pos.copy_(torch.tensor(new, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        e_pos, e_x, e_box = step(static_pos.detach().clone().requires_grad_(True))
        assert _same_bits(g_box, e_box) and _same_bits(g_pos, e_pos) and _same_bits(g_x, e_x)
        assert g_box.shape == (len(offsets) - 1, 3, 3) and float(e_box.abs().max()) > 0


def test_scripted_saved_and_reloaded_module_still_batches(monkeypatch, tmp_path):
    name = "valu"
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    tag = "ragged"
    pos, boxes, offsets, _ = frames.batch(tag)
    w1, b1, w2, b2, x, _ = frames.batch_layer(tag, W, G)[:6]
    nb = _neighbors(offsets)
    path = str(tmp_path / "neighbors.pt")
    torch.jit.script(nb).save(path)
    loaded = torch.jit.load(path)
    assert loaded.holder.frames() == []
    tpos, tbox, tx = _dev(pos, boxes, x)
    loaded.build(tpos, tbox)
    assert loaded.holder.frames() == [int(v) for v in offsets]
    nb.build(tpos, tbox)
    conv = _module(name, (w1, b1, w2, b2))
    a = torch.ops.NNPOpsCFConv.operation_periodic(conv.holder, loaded.holder, tpos, tbox, tx)
    b = torch.ops.NNPOpsCFConv.operation_periodic(conv.holder, nb.holder, tpos, tbox, tx)
    assert _same_bits(a, b) and not a[0].any() and bool(a[1:].abs().sum() > 0)          # (the lone atom: an empty row)
    ref = frames.reference(tag, W, G, act)
    assert np.abs(a.cpu().numpy() - ref["out"]).max() <= 1e-4 * np.abs(ref["out"]).max()


def test_torch_refusals(monkeypatch):
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    name = "valu"
    _env(monkeypatch, name)
    W, G, act = LAYERS[name][:3]
    pos, boxes, offsets, _ = frames.batch("ragged")
    w1, b1, w2, b2, x, _ = frames.batch_layer("ragged", W, G)[:6]
    B = len(offsets) - 1
    tpos, tbox, tx = _dev(pos, boxes, x)
    listed = [int(v) for v in offsets]
    nb = _neighbors(offsets)
    with pytest.raises(RuntimeError, match="set_frames"):
        nb.build(tpos, tbox[0])                              # a (3, 3) box on a list of frames
    with pytest.raises(RuntimeError, match="set_frames"):
        nb.holder.build_periodic(tpos, tbox[0])
    with pytest.raises(RuntimeError, match=f"\\[{B}, 3, 3\\]"):
        nb.build(tpos, tbox[:B - 1])
    with pytest.raises(RuntimeError, match=f"\\[{B}, 3, 3\\]"):
        nb.build(tpos, torch.cat([tbox, tbox[:1]]))
    with pytest.raises(RuntimeError, match="set_frames"):
        nb.build(tpos, None)
    nb.build(tpos, tbox)
    for kw in (dict(), dict(twice_differentiable=True), dict(trainable=True), dict(force_trainable=True)):
        conv = _module(name, (w1, b1, w2, b2), **kw).to(DEV)
        with pytest.raises(RuntimeError, match=f"\\[{B}, 3, 3\\]"):
            conv(nb, tpos, tx, tbox[0])
        with pytest.raises(RuntimeError, match=f"\\[{B}, 3, 3\\]"):
            conv(nb, tpos, tx, tbox[:B - 1])
        assert bool(torch.isfinite(conv(nb, tpos, tx, tbox)).all())
        if "twice_differentiable" in kw or "force_trainable" in kw:
            with pytest.raises(RuntimeError, match="box gradients need the default op|no box gradient"):
                conv(nb, tpos, tx, tbox.clone().requires_grad_(True))
    # a (3, 3) box on a list without frames keeps its message
    single = CFConvNeighbors(CUTOFF)
    with pytest.raises(RuntimeError, match="\\(3, 3\\)"):
        single.build(tpos, tbox)
    # set_frames after a non-periodic build
    built = CFConvNeighbors(CUTOFF)
    built.build(tpos)
    with pytest.raises(RuntimeError, match="built without a box"):
        built.set_frames(listed)
    # frames and molecules exclude each other
    with pytest.raises(RuntimeError, match="set_frames"):
        nb.set_molecules(listed)
    batched = CFConvNeighbors(CUTOFF)
    batched.set_molecules(listed)
    with pytest.raises(RuntimeError, match="set_molecules"):
        batched.set_frames(listed)
    # offsets that do not fit the positions: refused at the first build, no half-made handle stays behind
    odd = CFConvNeighbors(CUTOFF)
    odd.set_frames([0, 100, len(pos) + 1])
    with pytest.raises(RuntimeError, match="start at 0 and end at num_atoms"):
        odd.build(tpos, tbox[:2])
    odd.set_frames(listed)
    odd.build(tpos, tbox)
