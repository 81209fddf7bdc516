"""Periodic batches of the ANI symmetry functions -- every frame of a batch in its own box: nnpops_ani_set_molecules on a periodic
handle, the per-molecule box gradient, and the torch surface above them up to OptimizedTorchANI.

The judge is tests/ani_periodic_batch_float64.py (ani_float64.Restatement per molecule with its own box, pinned by
tests/test_ani_periodic_batch_reference_cpu.py); every float64 reference is computed once per module run and not changed.

Bars: the AEV at AEV_RTOL / AEV_ATOL of test_ani_dispatch_gpu.py (2e-5 / 2e-6); backprop and backprop_box at the project's FORCE_RTOL,
1e-4 of each array's largest entry, judged PER MOLECULE for box_deriv; the tangent at the bar of test_ani_tangent_gpu.py (1e-4 of the
largest entry of each block, the adjoint identity to 1e-4 of the sum of the absolute terms); energies and gradients through the modules
at the bars of test_ani_batch_energy_gpu.py (energy 5e-6 |e| + 1e-4, gradients 1e-4 of the largest entry); parameter gradients at G_BAR
of mlp_weights_float64 / mlp_force_weights_float64.  Every evaluation prints its measured figures (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import ani_members_float64 as AJ
import ani_periodic_batch_float64 as pb
import mlp_force_weights_float64 as TF
import mlp_weights_float64 as W
from ani_tangent_float64 import block_errors, functions
from box_gradient_judge import clean_env, moved_frames
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
AEV_RTOL, AEV_ATOL, FORCE_RTOL = 2e-5, 2e-6, 1e-4
ENERGY_RTOL, ENERGY_ATOL = 5e-6, 1e-4
TANGENT_BAR = 1e-4


def _clean_env(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_ANI_")


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


# ---------------------------------------------------------------------------------------------- the C ABI
@functools.lru_cache(maxsize=None)
def _reference(fset, torchani):
    """float64 judge of the four-frame batch: dict(r, a, g, gbox, L, wr, wa), once per (function list, angle convention)"""
    species, pos, boxes, offsets = pb.batch()
    fn = functions(fset)
    wr, wa = pb.weights(len(species), 7 + int(torchani), n_angular=len(np.asarray(fn[1]).reshape(-1, 4)))
    out = pb.judge(species, pos, boxes, offsets, fn, torchani, wr, wa)
    out.update(wr=wr, wa=wa)
    return out


def _handle(parts, fset="ani2x", torchani=True, periodic=True):
    """-> (handle with the frames `parts` as molecules, device positions, device boxes, offsets)"""
    from nnpops_amd.capi import AniSymmetryFunctions
    species, pos, boxes, offsets = pb.assemble(parts)
    sym = AniSymmetryFunctions(pb.N_SPECIES, pb.RCR, pb.RCA, species, *functions(fset), periodic=periodic, torchani=torchani)
    sym.set_molecules(offsets)
    return sym, _t(pos), _t(boxes), offsets


def _run(sym, tpos, tboxes, wr, wa):
    """compute, backprop_box -> clones of (radial, angular, position gradient, box gradient)"""
    radial, angular = sym.compute(tpos, tboxes)
    g, gbox = sym.backprop_box(tpos, tboxes, wr, wa)
    torch.cuda.synchronize()
    return radial.clone(), angular.clone(), g.clone(), gbox.clone()


def _check_aev(label, radial, angular, ref, rows=slice(None)):
    r, a = radial.cpu().numpy().astype(np.float64), angular.cpu().numpy().astype(np.float64)
    er, ea = float(np.abs(r - ref["r"][rows]).max()), float(np.abs(a - ref["a"][rows]).max())
    print(f"\n[ani-pbatch] {label}: AEV off by up to {er:.2e} (radial) {ea:.2e} (angular)", end="")
    np.testing.assert_allclose(r, ref["r"][rows], rtol=AEV_RTOL, atol=AEV_ATOL)
    np.testing.assert_allclose(a, ref["a"][rows], rtol=AEV_RTOL, atol=AEV_ATOL)


def _check_gradients(label, g, gbox, ref, pos, boxes, offsets):
    g, gbox = g.cpu().numpy().astype(np.float64), gbox.cpu().numpy().astype(np.float64)
    assert gbox.shape == ref["gbox"].shape and np.isfinite(gbox).all() and np.isfinite(g).all()
    err_g = float(np.abs(g - ref["g"]).max() / np.abs(ref["g"]).max())
    errs = [float(np.abs(gbox[m] - ref["gbox"][m]).max() / np.abs(ref["gbox"][m]).max()) for m in range(len(gbox))]
    anti = pb.stress_antisymmetry(pos, boxes, offsets, g, gbox)
    print(f"\n[ani-pbatch] {label}: position gradient {err_g:.2e} of max, box gradient per molecule {['%.2e' % e for e in errs]} of the "
          f"molecule's max, antisymmetric stress {['%.2e' % (a / w) for a, w in anti]} of the molecule's largest entry", end="")
    assert err_g <= FORCE_RTOL, (label, err_g)
    assert max(errs) <= FORCE_RTOL, (label, errs)
    for a, w in anti:                                  # rotation invariance, molecule by molecule
        assert a <= FORCE_RTOL * w, (label, a, w)


CASES = [("ani2x", True), ("ani2x", False), ("no_grid", True)]


@pytest.mark.parametrize("fset,torchani", CASES, ids=["torchani", "paper", "generic"])
def test_c_abi_against_float64(monkeypatch, fset, torchani):
    _clean_env(monkeypatch)
    ref = _reference(fset, torchani)
    species, pos, boxes, offsets = pb.batch()
    sym, tpos, tboxes, _ = _handle(pb.frames(), fset, torchani)
    assert sym.describe().get("batch_boxes") == "1"
    wr, wa = _t(ref["wr"]), _t(ref["wa"])
    radial, angular, g, gbox = _run(sym, tpos, tboxes, wr, wa)
    what = sym.describe()
    assert what["batch_boxes"] == "1" and what["fused_build"] == "0" and what["cells"] == "0", what
    assert what["generic"] == ("1" if fset == "no_grid" else "0"), what
    assert gbox.shape == (4, 3, 3) and gbox.dtype == torch.float32
    _check_aev(f"{fset} torchani={torchani}", radial, angular, ref)
    _check_gradients(f"{fset} torchani={torchani}", g, gbox, ref, pos, boxes, offsets)
    # repeated calls agree bit for bit, the position gradient is the plain backprop()'s
    again = _run(sym, tpos, tboxes, wr, wa)
    assert all(torch.equal(a, b) for a, b in zip(again, (radial, angular, g, gbox))), "two calls give different bits"
    assert torch.equal(sym.backprop(wr, wa), g), "the position gradient is not the plain backprop()'s"


def test_calls_around_the_box_gradient_keep_their_bits(monkeypatch):
    _clean_env(monkeypatch)
    ref = _reference("ani2x", True)
    sym, tpos, tboxes, _ = _handle(pb.frames())
    wr, wa = _t(ref["wr"]), _t(ref["wa"])
    tv = _t(np.random.default_rng(3).standard_normal((547, 3)).astype(np.float32))
    radial, angular = (t.clone() for t in sym.compute(tpos, tboxes))
    plain = sym.backprop(wr, wa).clone()
    tangent = tuple(t.clone() for t in sym.tangent(tv))
    g, gbox = (t.clone() for t in sym.backprop_box(tpos, tboxes, wr, wa))
    assert torch.equal(g, plain)
    after = sym.tangent(tv)
    assert torch.equal(after[0], tangent[0]) and torch.equal(after[1], tangent[1]), "tangent() after backprop_box() changed"
    assert torch.equal(sym.backprop(wr, wa), plain), "backprop() after backprop_box() changed"
    again = sym.compute(tpos, tboxes)
    assert torch.equal(again[0], radial) and torch.equal(again[1], angular), "compute() after backprop_box() changed"
    g2, gbox2 = sym.backprop_box(tpos, tboxes, wr, wa)
    assert torch.equal(g2, g) and torch.equal(gbox2, gbox)


# ---------------------------------------------------------------------------------------------- isolation and invariance
@pytest.mark.parametrize("move", ["box_vector", "shifted"])
def test_moving_one_molecule_leaves_the_others_their_bits(monkeypatch, move):
    """molecule 1 (triclinic): every other atom by its third box vector, the one with two off-diagonal entries; or molecule 0 as a
    whole by 0.37 box lengths along x, a third of it outside its box.  No displacement changes, so the moved molecule's AEV stays
    inside the bar; nothing of the other molecules may change at all."""
    _clean_env(monkeypatch)
    ref = _reference("ani2x", True)
    species, pos, boxes, offsets = pb.batch()
    moved = pos.copy()
    if move == "box_vector":
        which, lo, hi = 1, 130, 330
        moved[lo:hi:2] += boxes[1][2]
    else:
        which, lo, hi = 0, 0, 130
        moved[lo:hi] = moved_frames(pos[lo:hi], boxes[0])[0]
    sym, tpos, tboxes, _ = _handle(pb.frames())
    wr, wa = _t(ref["wr"]), _t(ref["wa"])
    base = _run(sym, tpos, tboxes, wr, wa)
    got = _run(sym, _t(moved), tboxes, wr, wa)
    others = np.ones(547, dtype=bool)
    others[lo:hi] = False
    rows = torch.tensor(others, device=DEV)
    for name, a, b in zip(("radial", "angular", "forces"), base[:3], got[:3]):
        assert torch.equal(a[rows], b[rows]), f"{name} of the other molecules changed"
    keep = [m for m in range(4) if m != which]
    assert torch.equal(base[3][keep], got[3][keep]), "box gradients of the other molecules changed"
    _check_aev(f"molecule {which} moved ({move})", got[0][lo:hi], got[1][lo:hi], ref, slice(lo, hi))
    err = float((got[2][lo:hi] - base[2][lo:hi]).abs().max() / base[2][lo:hi].abs().max())
    print(f"; its forces move by {err:.2e} of max", end="")
    assert err <= FORCE_RTOL


def test_a_molecule_is_the_same_bits_wherever_it_stands(monkeypatch):
    """the water frame at slot 0 of one batch and at slot 2 of another, other companions and other boxes around it"""
    _clean_env(monkeypatch)
    f = pb.frames()
    wr, wa = pb.weights(150, 11)
    out, words = [], []
    for parts, slot in (((f[2], f[0]), 0), ((f[3], f[1], f[2]), 2)):
        sym, tpos, tboxes, offsets = _handle(parts)
        lo, hi = int(offsets[slot]), int(offsets[slot + 1])
        n = int(offsets[-1])
        rng = np.random.default_rng(n)
        full_r, full_a = rng.standard_normal((n, 112)).astype(np.float32), rng.standard_normal((n, 896)).astype(np.float32)
        full_r[lo:hi], full_a[lo:hi] = wr, wa
        radial, angular, g, gbox = _run(sym, tpos, tboxes, _t(full_r), _t(full_a))
        out.append((radial[lo:hi], angular[lo:hi], g[lo:hi], gbox[slot]))
        what = sym.describe()
        words.append({k: what[k] for k in ("forward", "backward", "uniform", "literal", "dynamic_quads", "fused_build", "cap_angular", "chunk", "bwd_mode",
                                           "radial_bwd", "batch_boxes")})          # (batch_boxes: only periodic batches carry the word)
    assert words[0] == words[1], words                 # (both handles run the same kernels: the comparison is one of bits)
    for name, a, b in zip(("radial", "angular", "forces", "box gradient"), *out):
        assert torch.equal(a, b), f"{name} depends on the slot or on the companions"
    assert float(out[0][3].abs().max()) > 0


def test_overlaid_molecules_never_become_neighbours(monkeypatch):
    _clean_env(monkeypatch)
    f = pb.frames()
    wr, wa = pb.weights(67, 12)
    sym1, tpos1, tboxes1, _ = _handle((f[3],))
    one = _run(sym1, tpos1, tboxes1, _t(wr), _t(wa))
    sym2, tpos2, tboxes2, _ = _handle((f[3], f[3]))
    two = _run(sym2, tpos2, tboxes2, _t(np.concatenate([wr, wr])), _t(np.concatenate([wa, wa])))
    for name, a, b in zip(("radial", "angular", "forces"), one[:3], two[:3]):
        assert torch.equal(b[:67], a) and torch.equal(b[67:], a), f"{name}: the two copies on the same coordinates see each other"
    assert torch.equal(two[3][0], one[3][0]) and torch.equal(two[3][1], one[3][0])


# ---------------------------------------------------------------------------------------------- against a single handle
@pytest.mark.parametrize("fuse", [None, "0"], ids=["default", "two-launch"])
def test_batch_of_one_against_a_single_periodic_handle(monkeypatch, fuse):
    from nnpops_amd.capi import AniSymmetryFunctions
    _clean_env(monkeypatch)
    if fuse is not None:
        monkeypatch.setenv("NNPOPS_ANI_FUSE", fuse)
    species, pos, box = pb.frames()[2]
    fn = workloads.ani2x_functions()
    wr, wa = pb.weights(150, 13)
    ref = pb.judge(species, pos, box[None], np.array([0, 150]), fn, True, wr, wa)
    sym, tpos, tboxes, offsets = _handle((pb.frames()[2],))
    batch = _run(sym, tpos, tboxes, _t(wr), _t(wa))
    single = AniSymmetryFunctions(pb.N_SPECIES, pb.RCR, pb.RCA, species, *fn, periodic=True)
    single.set_neighbor_algorithm(1)
    alone = _run(single, tpos, _t(box), _t(wr), _t(wa))
    assert alone[3].shape == (3, 3) and batch[3].shape == (1, 3, 3)
    for label, out in (("batch of one", batch), ("single handle", alone)):
        _check_aev(label, out[0], out[1], ref)
        _check_gradients(label, out[2], out[3].reshape(1, 3, 3), ref, pos, box[None], offsets)
    a, b = sym.describe(), single.describe()
    assert a.get("batch_boxes") == "1" and "batch_boxes" not in b and a["fused_build"] == "0"
    if fuse == "0":
        assert b["fused_build"] == "0", b
    if a["fused_build"] == b["fused_build"] and a["forward"] == b["forward"] and a["chunk"] == b["chunk"] and a["cap_angular"] == b["cap_angular"]:
        assert torch.equal(batch[0], alone[0]) and torch.equal(batch[1], alone[1]), "the same forward kernel gives other bits"
        assert torch.equal(batch[2], alone[2])


# ---------------------------------------------------------------------------------------------- exact cases
def test_wide_boxes_give_a_zero_box_gradient_and_the_vacuum_aev(monkeypatch):
    """every box 50 A wide around frames of ~11 A: no pair is shifted, box_deriv is exactly zero and the AEV is the non-periodic batch's"""
    _clean_env(monkeypatch)
    species, pos, _, offsets = pb.batch()
    wide = np.stack([np.eye(3, dtype=np.float32) * 50.0] * 4)
    wr, wa = (_t(w) for w in pb.weights(547, 14))
    sym, tpos, _, _ = _handle(pb.frames())
    radial, angular, g, gbox = _run(sym, tpos, _t(wide), wr, wa)
    assert torch.equal(gbox, torch.zeros_like(gbox)), gbox
    vac, _, _, _ = _handle(pb.frames(), periodic=False)
    r0, a0 = vac.compute(tpos, None)
    g0 = vac.backprop(wr, wa)
    assert "batch_boxes" not in vac.describe()
    np.testing.assert_allclose(radial.cpu().numpy(), r0.cpu().numpy(), rtol=AEV_RTOL, atol=AEV_ATOL)
    np.testing.assert_allclose(angular.cpu().numpy(), a0.cpu().numpy(), rtol=AEV_RTOL, atol=AEV_ATOL)
    assert float((g - g0).abs().max()) <= FORCE_RTOL * float(g0.abs().max())
    assert float(a0.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- the tangent
def test_tangent_on_a_periodic_batch(monkeypatch):
    _clean_env(monkeypatch)
    ref = _reference("ani2x", True)
    species, pos, boxes, offsets = pb.batch()
    v = np.random.default_rng([547, 4]).standard_normal((547, 3)).astype(np.float32)
    want = pb.tangent(species, pos, boxes, offsets, workloads.ani2x_functions(), v)
    sym, tpos, tboxes, _ = _handle(pb.frames())
    wr, wa, tv = _t(ref["wr"]), _t(ref["wa"]), _t(v)
    sym.compute(tpos, tboxes)
    force = sym.backprop(wr, wa).clone()
    first = tuple(t.clone() for t in sym.tangent(tv))
    second = sym.tangent(tv)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    er, ea = block_errors(tuple(t.cpu().numpy() for t in first), want)
    left = float((wr.double() * first[0].double()).sum() + (wa.double() * first[1].double()).sum())
    right = float((force.double() * tv.double()).sum())
    size = float((wr * first[0]).abs().double().sum() + (wa * first[1]).abs().double().sum() + (force * tv).abs().double().sum())
    print(f"\n[ani-pbatch] tangent: radial {er:.2e} angular {ea:.2e} of the largest entry; <w, Jv> - <J^T w, v> = {abs(left - right) / size:.2e} "
          f"of the terms", end="")
    assert er <= TANGENT_BAR and ea <= TANGENT_BAR, (er, ea)
    assert abs(left - right) <= TANGENT_BAR * size, (left, right, size)


# ---------------------------------------------------------------------------------------------- capacity
def test_overflowing_rows_are_regrown(monkeypatch):
    from nnpops_amd import capi
    _clean_env(monkeypatch)
    monkeypatch.setenv("NNPOPS_ANI_CAP", "16")          # rows of 16 entries: every atom of these frames has more neighbours
    ref = _reference("ani2x", True)
    species, pos, boxes, offsets = pb.batch()
    sym, tpos, tboxes, _ = _handle(pb.frames())
    sym.compute(tpos, tboxes, check=False)
    assert capi.lib().nnpops_ani_check(sym._h, None, None) == capi.ERR_CAPACITY, "the first compute() did not overflow"
    radial, angular, g, gbox = _run(sym, tpos, tboxes, _t(ref["wr"]), _t(ref["wa"]))
    assert int(sym.describe()["cap"]) > 16
    _check_aev("regrown", radial, angular, ref)
    _check_gradients("regrown", g, gbox, ref, pos, boxes, offsets)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_and_the_way_back_to_one_box(monkeypatch):
    from nnpops_amd.capi import AniSymmetryFunctions, NNPOpsHipError
    _clean_env(monkeypatch)
    species, pos, box = pb.frames()[2]
    fn = workloads.ani2x_functions()
    tpos, tbox = _t(pos), _t(box)
    wr, wa = (_t(w) for w in pb.weights(150, 15))
    # a non-periodic handle with molecules has no box to differentiate
    vac = AniSymmetryFunctions(pb.N_SPECIES, pb.RCR, pb.RCA, species, *fn, periodic=False)
    vac.set_molecules([0, 75, 150])
    vac.compute(tpos, None)
    with pytest.raises(NNPOpsHipError, match="periodic"):
        vac.backprop_box(tpos, tbox, wr, wa)
    # a periodic handle with molecules takes one box per molecule ...
    sym = AniSymmetryFunctions(pb.N_SPECIES, pb.RCR, pb.RCA, species, *fn, periodic=True)
    sym.set_neighbor_algorithm(1)
    alone = _run(sym, tpos, tbox, wr, wa)
    sym.set_molecules([0, 75, 150])
    assert sym.describe().get("batch_boxes") == "1"
    with pytest.raises(ValueError, match="box"):
        sym.compute(tpos, tbox)
    with pytest.raises(ValueError, match="box"):
        sym.compute(tpos, torch.stack([tbox] * 3))
    two = _run(sym, tpos, torch.stack([tbox, tbox]).contiguous(), wr, wa)
    assert two[3].shape == (2, 3, 3) and not torch.equal(two[0], alone[0])
    sym.set_molecules([0, 100, 150])
    with pytest.raises(NNPOpsHipError, match="compute"):             # (set_molecules invalidates the lists)
        sym.backprop(wr, wa)
    # ... and set_molecules(None) returns to one box: the bits of before
    sym.set_molecules(None)
    assert "batch_boxes" not in sym.describe()
    with pytest.raises(ValueError, match="box"):
        sym.compute(tpos, torch.stack([tbox, tbox]))
    back = _run(sym, tpos, tbox, wr, wa)
    assert all(torch.equal(a, b) for a, b in zip(back, alone))


# ---------------------------------------------------------------------------------------------- the torch surface: aev / operation
@functools.lru_cache(maxsize=None)
def _model():
    return AJ.model_of(3)


def _numbers(species):
    return torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=DEV)


def _batched_holder(species, offsets):
    from NNPOps.SymmetryFunctions import TorchANISymmetryFunctions
    model = _model()
    ctor = TorchANISymmetryFunctions(model.species_converter, model.aev_computer, _numbers(species[:2]).cpu())._ctor
    holder = torch.classes.NNPOpsANISymmetryFunctions.Holder(*ctor, [int(s) for s in species])
    holder.set_molecules([int(o) for o in offsets])
    return holder


@pytest.mark.parametrize("op", ["aev", "operation"])
def test_ops_with_a_batched_holder_and_one_cell_per_frame(monkeypatch, op):
    _clean_env(monkeypatch)
    ref = _reference("ani2x", True)
    species, pos, boxes, offsets = pb.batch()
    w = _t(np.concatenate([ref["wr"], ref["wa"]], axis=1))

    def run(cell_grad, create_graph=False):
        holder = _batched_holder(species, offsets)
        x, cell = _t(pos).requires_grad_(True), _t(boxes).requires_grad_(cell_grad)
        if op == "aev":
            aev = torch.ops.NNPOpsANISymmetryFunctions.aev(holder, x, cell)
        else:
            aev = torch.cat(torch.ops.NNPOpsANISymmetryFunctions.operation(holder, x, cell), dim=1)
        loss = (aev * w).sum()
        if create_graph:
            return torch.autograd.grad(loss, [x, cell], create_graph=True)
        loss.backward()
        return aev.detach(), x.grad, cell.grad

    aev, gx, gcell = run(True)
    aev0, gx0, none = run(False)
    assert none is None and gcell.shape == (4, 3, 3)
    assert torch.equal(aev, aev0) and torch.equal(gx, gx0), "the position gradient depends on whether the cell wants one"
    _check_aev(f"torch.ops {op}", aev[:, :112], aev[:, 112:], ref)
    _check_gradients(f"torch.ops {op}", gx, gcell, ref, pos, boxes, offsets)
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        run(True, create_graph=True)
    # the shapes a batched holder refuses, by name
    holder = _batched_holder(species, offsets)
    for bad in (_t(boxes[0]), _t(boxes[:3])):
        with pytest.raises(RuntimeError, match=r"\[4, 3, 3\]"):
            torch.ops.NNPOpsANISymmetryFunctions.aev(holder, _t(pos), bad)


def test_a_holder_without_molecules_keeps_its_messages(monkeypatch):
    from NNPOps.SymmetryFunctions import TorchANISymmetryFunctions
    _clean_env(monkeypatch)
    species, coords, cells = pb.module_frames()
    model = _model()
    module = TorchANISymmetryFunctions(model.species_converter, model.aev_computer, _numbers(species).cpu()).to(DEV)
    with pytest.raises(RuntimeError, match='The shape of "cell" has to have 2 dimensions'):
        torch.ops.NNPOpsANISymmetryFunctions.aev(module.holder, _t(coords[0]), _t(cells))


def test_capture_and_replay_of_the_batched_aev(monkeypatch):
    """forward and backward (with the box gradient) of the three-frame water batch, 450 atoms, captured once and replayed on new
    positions: the eager bits.  Evaluated before the capture (capacities fitted, allocator warm); no stream split at this size."""
    _clean_env(monkeypatch)
    species, coords, cells = pb.module_frames()
    holder = _batched_holder(np.tile(species, 3), [0, 150, 300, 450])
    cell = _t(cells).requires_grad_(True)
    static = _t(coords.reshape(450, 3)).requires_grad_(True)
    w = torch.randn((450, 1008), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))

    def step(p):
        aev = torch.ops.NNPOpsANISymmetryFunctions.aev(holder, p, cell)
        return (aev.detach(),) + torch.autograd.grad((aev * w).sum(), [p, cell])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(static)
    rng = np.random.default_rng(1)
    for _ in range(2):
        new = (coords.reshape(450, 3) + rng.normal(0, 0.03, (450, 3))).astype(np.float32)
        with torch.no_grad():
            static.copy_(_t(new))
        graph.replay()
        torch.cuda.synchronize()
        eager = step(static.detach().clone().requires_grad_(True))
        for name, a, b in zip(("aev", "position gradient", "cell gradient"), captured, eager):
            assert torch.equal(a, b), f"replayed {name} differs from the eager one"
        assert eager[2].shape == (3, 3, 3) and float(eager[2].abs().max()) > 0


# ---------------------------------------------------------------------------------------------- the torch surface: the modules
@functools.lru_cache(maxsize=None)
def _module_judge():
    """float64: member energies E [3 frames][M] (no self energy), and per frame and member dE_m/dpositions [3][M][150][3] and
    dE_m/dcell [3][M][3][3] -- the networks of _model() per species in float64 on the judge's AEV, its backward by the judge"""
    species, coords, cells = pb.module_frames()
    model = _model()
    fn = workloads.ani2x_functions()
    nets = [{sym: net.double() for sym, net in member.items()} for member in model.neural_networks]
    M = len(nets)
    E, G, C = np.empty((3, M)), np.empty((3, M, 150, 3)), np.empty((3, M, 3, 3))
    try:
        for b in range(3):
            one = (species, coords[b], cells[b][None], np.array([0, 150]))
            out = pb.judge(*one, fn)
            aev = torch.tensor(np.concatenate([out["r"], out["a"]], axis=1), requires_grad=True)
            e = AJ.member_energies(nets, species, aev)
            E[b] = e.detach().numpy()
            for m in range(M):
                d = torch.autograd.grad(e[m], aev, retain_graph=True)[0].numpy()
                back = pb.judge(*one, fn, True, np.ascontiguousarray(d[:, :112]), np.ascontiguousarray(d[:, 112:]))
                G[b, m], C[b, m] = back["g"], back["gbox"][0]
    finally:
        for member in model.neural_networks:
            member.float()
    for a in (E, G, C):
        a.setflags(write=False)
    return E, G, C


def _optimized(**kwargs):
    from NNPOps import OptimizedTorchANI
    species, _, _ = pb.module_frames()
    numbers = _numbers(species)
    return OptimizedTorchANI(_model(), numbers.cpu(), **kwargs).to(DEV), numbers


PBC = torch.tensor([True, True, True])


def _inputs():
    species, coords, cells = pb.module_frames()
    return _t(coords).requires_grad_(True), _t(cells).requires_grad_(True)


def _check_energy_step(label, e, gx, gcell, w, E_ref, G_ref, C_ref):
    """e [B] float64, gradients of sum_b w_b e_b against the judge's mean over the members"""
    species, _, _ = pb.module_frames()
    e, gx, gcell = e.detach().cpu().numpy(), gx.cpu().numpy().astype(np.float64), gcell.cpu().numpy().astype(np.float64)
    assert e.dtype == np.float64 and gcell.shape == (3, 3, 3)
    worst = [0.0, 0.0, 0.0]
    for b in range(3):
        e_ref = E_ref[b].mean() + AJ.self_energy(species)
        g_ref, c_ref = w[b] * G_ref[b].mean(0), w[b] * C_ref[b].mean(0)
        errs = (abs(e[b] - e_ref), np.abs(gx[b] - g_ref).max() / np.abs(g_ref).max(), np.abs(gcell[b] - c_ref).max() / np.abs(c_ref).max())
        worst = [max(a, float(x)) for a, x in zip(worst, errs)]
        assert errs[0] <= ENERGY_RTOL * abs(e_ref) + ENERGY_ATOL, (label, b, e[b], e_ref)
        assert errs[1] <= FORCE_RTOL and errs[2] <= FORCE_RTOL, (label, b, errs)
    print(f"\n[ani-pbatch] {label}: energy off by up to {worst[0]:.2e}, coordinate gradient {worst[1]:.2e}, cell gradient {worst[2]:.2e} of the "
          f"frame's largest entry", end="")


@pytest.mark.parametrize("fused_step", [True, False], ids=["fused", "composition"])
def test_forward_batch_with_a_cell_per_frame(monkeypatch, fused_step):
    _clean_env(monkeypatch)
    module, numbers = _optimized(fused_step=fused_step)
    assert type(module).__name__ == ("FusedOptimizedTorchANI" if fused_step else "OptimizedTorchANI")
    x, cell = _inputs()
    w = np.array([0.7, -1.3, 1.1])
    e = module.forward_batch((numbers.expand(3, -1), x), cell, PBC).energies
    (e * _t(w)).sum().backward()
    _check_energy_step(f"forward_batch fused_step={fused_step}", e, x.grad, cell.grad, w, *_module_judge())
    # ... and against the loop of single-frame calls it replaces
    for b in range(3):
        xb, cb = x[b:b + 1].detach().clone().requires_grad_(True), cell[b].detach().clone().requires_grad_(True)
        one = module((numbers, xb), cb, PBC).energies
        (one * float(w[b])).sum().backward()
        assert abs(float(one) - float(e[b])) <= ENERGY_RTOL * abs(float(one)) + ENERGY_ATOL
        assert float((xb.grad[0] - x.grad[b]).abs().max()) <= FORCE_RTOL * float(xb.grad.abs().max())
        assert float((cb.grad - cell.grad[b]).abs().max()) <= FORCE_RTOL * float(cb.grad.abs().max())
    # without a cell gradient: the same energies and coordinate gradient, bit for bit
    x2, cell2 = _inputs()
    e2 = module.forward_batch((numbers.expand(3, -1), x2), cell2.detach(), PBC).energies
    (e2 * _t(w)).sum().backward()
    assert torch.equal(e2, e) and torch.equal(x2.grad, x.grad)
    if fused_step:
        with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
            x3, cell3 = _inputs()
            e3 = module.forward_batch((numbers.expand(3, -1), x3), cell3, PBC).energies
            torch.autograd.grad(e3.sum(), [x3, cell3], create_graph=True)


def test_aev_module_forward_batch_against_the_loop(monkeypatch):
    from NNPOps.SymmetryFunctions import TorchANISymmetryFunctions
    _clean_env(monkeypatch)
    species, coords, cells = pb.module_frames()
    model = _model()
    numbers = _numbers(species)
    module = TorchANISymmetryFunctions(model.species_converter, model.aev_computer, numbers.cpu()).to(DEV)
    sp = torch.tensor(species, device=DEV).unsqueeze(0)
    w = torch.randn((3, 150, 1008), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    x, cell = _inputs()
    aev = module.forward_batch((sp.expand(3, -1), x), cell, PBC)[1]
    assert aev.shape == (3, 150, 1008)
    (aev * w).sum().backward()
    assert cell.grad.shape == (3, 3, 3)
    for b in range(3):
        xb, cb = x[b:b + 1].detach().clone().requires_grad_(True), cell[b].detach().clone().requires_grad_(True)
        one = module((sp, xb), cb, PBC)[1]
        (one * w[b:b + 1]).sum().backward()
        np.testing.assert_allclose(aev[b].detach().cpu().numpy(), one[0].detach().cpu().numpy(), rtol=AEV_RTOL, atol=AEV_ATOL)
        assert float((xb.grad[0] - x.grad[b]).abs().max()) <= FORCE_RTOL * float(xb.grad.abs().max())
        assert float((cb.grad - cell.grad[b]).abs().max()) <= FORCE_RTOL * float(cb.grad.abs().max())
    # the periodic holder is an entry of its own: the non-periodic batch of the same size still runs, and gives other numbers
    vac = module.forward_batch((sp.expand(3, -1), x.detach()))[1]
    assert not torch.equal(vac, aev.detach())
    assert module.batch_holder(3, True) is not module.batch_holder(3)


def test_members_qbcs_and_energy_and_forces_with_a_cell(monkeypatch):
    _clean_env(monkeypatch)
    module, numbers = _optimized()
    E_ref, G_ref, C_ref = _module_judge()
    species, _, _ = pb.module_frames()
    sae = AJ.self_energy(species)
    sp = numbers.expand(3, -1)
    # member energies [M, B] and the gradient of a weighted sum of them
    x, cell = _inputs()
    wm = AJ.random_weights(3, 3, seed=9)                                  # [B][M]
    members = module.members_energies_batch((sp, x), cell, PBC).energies
    assert members.shape == (3, 3) and members.dtype == torch.float64
    (members * _t(wm.T.copy())).sum().backward()
    for b in range(3):
        for m in range(3):
            assert abs(float(members[m, b]) - (E_ref[b, m] + sae)) <= ENERGY_RTOL * abs(E_ref[b, m] + sae) + ENERGY_ATOL
        g_ref, c_ref = AJ.combine(wm[b], G_ref[b]), np.einsum("m,mij->ij", wm[b], C_ref[b])
        top_g, top_c = AJ.magnitude(wm[b], G_ref[b]), float(np.einsum("m,mij->ij", np.abs(wm[b]), np.abs(C_ref[b])).max())
        assert np.abs(x.grad[b].cpu().numpy() - g_ref).max() <= FORCE_RTOL * top_g
        assert np.abs(cell.grad[b].cpu().numpy() - c_ref).max() <= FORCE_RTOL * top_c
    # energies_qbcs_batch: mean and QBC factor of the same member energies
    _, mean, qbcs = module.energies_qbcs_batch((sp, x.detach()), cell.detach(), PBC)
    assert torch.allclose(mean, members.detach().mean(0), rtol=0, atol=1e-12)
    want_q = AJ.sigma(E_ref) / 150 ** 0.5
    assert np.abs(qbcs.cpu().numpy() - want_q).max() <= ENERGY_RTOL * np.abs(E_ref + sae).max() + ENERGY_ATOL
    # energy_and_forces_batch: forward_batch's energies and negated gradients, bit for bit, outside autograd, no virial
    x2, cell2 = _inputs()
    e = module.forward_batch((sp, x2), cell2.detach(), PBC).energies
    e.sum().backward()
    out = module.energy_and_forces_batch((sp, x2.detach()), cell2.detach(), PBC)
    assert len(out) == 2 and out[0].grad_fn is None and out[1].shape == (3, 150, 3)
    assert torch.equal(out[0], e.detach()) and torch.equal(out[1], -x2.grad)


def test_trainable_energy_loss_over_a_periodic_batch(monkeypatch):
    _clean_env(monkeypatch)
    module, numbers = _optimized(trainable=True)
    assert type(module).__name__ == "TrainableOptimizedTorchANI"
    nets = module.neural_networks[0]
    species, coords, cells = pb.module_frames()
    fn = workloads.ani2x_functions()
    c = np.array([0.7, -1.3, 1.1])
    module.zero_grad()
    x, cell = _inputs()
    e = module.forward_batch((numbers.expand(3, -1), x), cell.detach(), PBC).energies
    (e * _t(c)).sum().backward()
    got = W.gradients_of_module(nets)
    # the judge: sum_b c_b mean_m E_m(frame b) over the float64 AEV of every frame in its own box
    kinds = W.kinds_of_module(nets)
    M = nets.num_models
    want = None
    for b in range(3):
        out = pb.judge(species, coords[b], cells[b][None], np.array([0, 150]), fn)
        aev = torch.tensor(np.concatenate([out["r"], out["a"]], axis=1))
        part, _ = W.autograd(kinds, aev, np.full(M, c[b] / M))
        want = part if want is None else [{g: kd[g] + pd[g] for g in W.NAMES} for kd, pd in zip(want, part)]
    err, where = W.worst(got, want)
    print(f"\n[ani-pbatch] trainable=True, energy loss over three periodic frames: parameter gradients {err:.2e} of the largest entry at {where}", end="")
    assert err <= W.G_BAR, (err, where)
    # the energies are the default module's bits at equal weights, on a periodic batch as elsewhere; the coordinate gradient of a
    # WEIGHTED sum is formed in another order there (the default step scales its kept forces), so it is compared at the force bar
    default, _ = _optimized()
    x0, _ = _inputs()
    e0 = default.forward_batch((numbers.expand(3, -1), x0), cell.detach(), PBC).energies
    (e0 * _t(c)).sum().backward()
    assert torch.equal(e0, e.detach())
    assert float((x0.grad - x.grad).abs().max()) <= FORCE_RTOL * float(x0.grad.abs().max())


def test_force_trainable_force_loss_over_a_periodic_batch(monkeypatch):
    _clean_env(monkeypatch)
    module, numbers = _optimized(force_trainable=True)
    assert type(module).__name__ == "ForceTrainableOptimizedTorchANI"
    nets = module.neural_networks[0]
    species, coords, cells = pb.module_frames()
    kinds = W.kinds_of_module(nets, torch.float64)
    want, e0, f0, loss64 = None, [], [], 0.0
    for b in range(3):                                  # the loss is a sum over the frames: frame by frame, each in its own box
        part, e0_b, f0_b, loss_b = TF.force_loss_float64(kinds, species, coords[b:b + 1], cells[b])
        want = part if want is None else [{g: kd[g] + pd[g] for g in W.NAMES} for kd, pd in zip(want, part)]
        e0.append(e0_b[0]); f0.append(f0_b[0]); loss64 += loss_b
    params = list(module.neural_networks.parameters())
    module.zero_grad()
    x = _t(coords).requires_grad_(True)
    cell = _t(cells)
    energies = module.forward_batch((numbers.expand(3, -1), x), cell, PBC).energies
    force = -torch.autograd.grad(energies.sum(), x, create_graph=True)[0]
    assert force.requires_grad, "the force carries no graph: the backward was not recorded"
    loss = ((energies - _t(np.array(e0))) ** 2).sum() + ((force - _t(np.stack(f0)).to(force.dtype)) ** 2).sum()
    loss.backward(inputs=params)
    got = W.gradients_of_module(nets)
    err, where = W.worst(got, want)
    print(f"\n[ani-pbatch] force_trainable=True, force loss over three periodic frames: loss {float(loss.detach()):.6e} (float64 {loss64:.6e}), "
          f"parameter gradients {err:.2e} of the largest entry at {where}", end="")
    assert err <= TF.G_BAR, (err, where)
    # a cell that requires a gradient is refused under create_graph
    x2, cell2 = _inputs()
    e2 = module.forward_batch((numbers.expand(3, -1), x2), cell2, PBC).energies
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(e2.sum(), [x2, cell2], create_graph=True)


def test_pinned_refusals_still_raise(monkeypatch):
    _clean_env(monkeypatch)
    module, numbers = _optimized()
    x, cell = _inputs()
    sp = numbers.expand(3, -1)
    for method in (module.forward_batch, module.members_energies_batch, module.energy_and_forces_batch):
        with pytest.raises(ValueError, match="non-periodic"):
            method((sp, x.detach()), cell[0].detach(), PBC)
        with pytest.raises(ValueError, match="non-periodic"):
            method((sp, x.detach()), None, PBC)
        with pytest.raises(ValueError, match="Only fully periodic"):
            method((sp, x.detach()), cell.detach(), torch.tensor([True, False, True]))
    nets = module.neural_networks[0]
    holder = module.aev_computer.batch_holder(3)
    with pytest.raises(RuntimeError, match="batches of molecules are non-periodic: a cell is not supported"):
        nets.fused_energy_batch(holder, x.detach(), None, cell[0].detach())
    with pytest.raises(RuntimeError, match=r"\[3, 3, 3\]"):
        nets.fused_energy_batch(module.aev_computer.batch_holder(3, True), x.detach(), None, cell[:2].detach())
