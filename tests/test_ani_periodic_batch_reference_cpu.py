"""Periodic batches of the ANI symmetry functions: what pins the float64 judge of tests/ani_periodic_batch_float64.py and what exists
without a GPU (CPU only).

What pins the judge (Restatement.evaluate per molecule, each with its own box):
    the float32 oracle per molecule   at the project's AEV bars (rtol 2e-5, atol 2e-6: AEV_RTOL / AEV_ATOL of test_ani_dispatch_gpu.py);
        its position gradient against the oracle in double precision, 1e-10 of the largest entry
    dL/dB of one molecule, all nine entries   against central differences of the judge's own L, Richardson-extrapolated from the steps
        h = 2^-13 and 2^-14 Angstrom (the procedure of test_ani_box_gradient_reference_cpu.py: the judge rounds its box to float32, so
        the steps are powers of two, exact next to an ~11 Angstrom entry).  The judge recomputes its shifts from the moved box, so the
        difference quotient is the formal derivative only on a frame where no shift changes across the step: the test
        asserts, for the four moved boxes of every entry, that every pair inside the radial cutoff + 0.01 Angstrom keeps the shift it
        has at the centre (a pair that crosses a cutoff inside the step does so with value and slope zero, as discussed there).  Bar
        1e-6 of the largest entry, as there.
    the frames   every box at least 2 x 5.1 wide on every diagonal entry, shifted pairs on every axis, the offsets the issue states.
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import ani_periodic_batch_float64 as pb
from ani_float64 import Restatement
from nnpops_amd import workloads
from oracle import AniOracle, AniOracle64

AEV_RTOL, AEV_ATOL = 2e-5, 2e-6
FD_RTOL = 1e-6
PIN_RTOL = 1e-10


def test_frames_are_wide_enough_and_wrap_on_every_axis():
    species, pos, boxes, offsets = pb.batch()
    assert offsets.tolist() == [0, 130, 330, 480, 547]
    assert all(int(o) % 64 for o in offsets[1:])
    counts = []
    for m, (sp, x, box) in enumerate(pb.frames()):
        c = pb.census(sp, x, box)
        counts.append(c)
        print(f"\n[ani-pbatch-reference] frame {m}: {len(sp)} atoms, widths {c['width']}, pairs {c['pairs']}, shifted {c['shifted']} "
              f"(per axis {c['per_axis']}), triples {c['triples']}")
        assert min(c["width"]) >= 2 * pb.RCR, c
        assert all(n > 0 for n in c["per_axis"]), c
    assert [c["pairs"] for c in counts] == [6998, 11100, 8290, 1846]
    assert [c["shifted"] for c in counts] == [3068, 4286, 3156, 808]
    assert counts[2]["triples"] == 22713
    assert np.count_nonzero(pb.frames()[1][2] - np.diag(np.diag(pb.frames()[1][2]))) == 3          # (the triclinic frame's off-diagonals)
    species, coords, cells = pb.module_frames()
    assert coords.shape == (3, 150, 3) and cells.shape == (3, 3, 3)
    for b in range(3):
        c = pb.census(species, coords[b], cells[b])
        assert min(c["width"]) >= 2 * pb.RCR and all(n > 0 for n in c["per_axis"]), c
    assert min(float(cells[b, a, a]) for b in range(3) for a in range(3)) > 11.0


@pytest.mark.parametrize("torchani", [True, False], ids=["torchani", "paper"])
def test_judge_is_the_float32_oracle_per_molecule(torchani):
    species, pos, boxes, offsets = pb.batch()
    functions = workloads.ani2x_functions()
    wr, wa = pb.weights(len(species), 5)
    out = pb.judge(species, pos, boxes, offsets, functions, torchani, wr, wa)
    assert out["r"].shape == wr.shape and out["a"].shape == wa.shape and out["gbox"].shape == (4, 3, 3) and out["g"].shape == (547, 3)
    assert abs(out["L"] - float((out["r"] * wr).sum() + (out["a"] * wa).sum())) <= 1e-9 * float(np.abs(out["Lm"]).sum())
    for m in range(4):
        lo, hi = int(offsets[m]), int(offsets[m + 1])
        oracle = AniOracle(pb.N_SPECIES, pb.RCR, pb.RCA, species[lo:hi], *functions, periodic=True, torchani=torchani)
        r_ref, a_ref = oracle.forward(pos[lo:hi], boxes[m])
        np.testing.assert_allclose(out["r"][lo:hi], r_ref, rtol=AEV_RTOL, atol=AEV_ATOL)
        np.testing.assert_allclose(out["a"][lo:hi], a_ref, rtol=AEV_RTOL, atol=AEV_ATOL)
        # the position gradient against the oracle in double precision (both sides float64: the bar of test_ani_box_gradient_reference_cpu.py)
        oracle64 = AniOracle64(pb.N_SPECIES, pb.RCR, pb.RCA, species[lo:hi], *functions, periodic=True, torchani=torchani)
        oracle64.forward(pos[lo:hi], boxes[m])
        g_ref = oracle64.backward(wr[lo:hi], wa[lo:hi])
        err = float(np.abs(out["g"][lo:hi] - g_ref).max() / np.abs(g_ref).max())
        print(f"\n[ani-pbatch-reference] molecule {m} torchani={torchani}: position gradient {err:.2e} of max against the float64 oracle")
        assert err <= PIN_RTOL, (m, err)
        assert np.abs(out["gbox"][m]).max() > 0


def test_cell_gradient_of_one_molecule_against_central_differences():
    species, pos, box = pb.frames()[1]                 # the triclinic frame: every one of the nine entries moves a displacement
    functions = workloads.ani2x_functions()
    rest = Restatement(pb.N_SPECIES, pb.RCR, pb.RCA, species, *functions)
    wr, wa = pb.weights(len(species), 6)
    centre = rest.evaluate(pos, box, wr, wa)
    box64 = box.astype(np.float64)
    pos64 = pos.astype(np.float64)

    # every pair that is, or within the step could become, a neighbour: inside the radial cutoff + 0.01 A at the centre box
    n0 = rest.shifts(pos64, box64)
    d0 = pos64[None, :, :] - pos64[:, None, :] + n0 @ box64
    near = np.einsum("ijk,ijk->ij", d0, d0) < (pb.RCR + 0.01) ** 2
    assert (n0[near] != 0).any(axis=0).all()

    worst, top = 0.0, float(np.abs(centre["gbox"]).max())
    for k in range(3):
        for c in range(3):
            def central(h):
                plus, minus = box64.copy(), box64.copy()
                plus[k, c] += h; minus[k, c] -= h
                for moved in (plus, minus):
                    assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)
                    assert np.array_equal(rest.shifts(pos64, moved)[near], n0[near]), "a shift changes across the step"
                return (rest.evaluate(pos, plus, wr, wa)["L"] - rest.evaluate(pos, minus, wr, wa)["L"]) / (2 * h)
            fd = (4.0 * central(2.0 ** -14) - central(2.0 ** -13)) / 3.0
            worst = max(worst, abs(fd - centre["gbox"][k, c]))
    print(f"\n[ani-pbatch-reference] cell gradient of the triclinic molecule vs central differences: {worst / top:.2e} of max {top:.3e}")
    assert worst <= FD_RTOL * top, (worst, top)
    # ... and it is the entry of the batch judge for that molecule
    sp, x, boxes, offsets = pb.batch()
    wr_b, wa_b = np.zeros((547, wr.shape[1]), np.float32), np.zeros((547, wa.shape[1]), np.float32)
    wr_b[130:330], wa_b[130:330] = wr, wa
    out = pb.judge(sp, x, boxes, offsets, functions, True, wr_b, wa_b)
    assert np.array_equal(out["gbox"][1], centre["gbox"]) and not out["gbox"][[0, 2, 3]].any()


def test_library_and_capi_surface():
    from nnpops_amd import capi
    L = capi.lib()
    for name in ("nnpops_ani_set_molecules", "nnpops_ani_backprop_box_strided", "nnpops_ani_tangent_strided", "nnpops_ani_describe"):
        assert hasattr(L, name) and name in capi.SIGNATURES
    assert L.nnpops_ani_set_molecules(ctypes.c_void_p(), 2, ctypes.c_void_p()) < 0 and b"NULL" in L.nnpops_last_error()
    sym = capi.AniSymmetryFunctions
    assert "box" in inspect.signature(sym.compute).parameters and "box_grad" in inspect.signature(sym.backprop_box).parameters
    assert "[M,3,3]" in sym.compute.__doc__ and "[M,3,3]" in sym.backprop_box.__doc__ and "[M,3,3]" in sym.set_molecules.__doc__
    header = open(capi.__file__.replace("nnpops_amd/capi.py", "include/nnpops_hip.h")).read()
    assert "[num_molecules][3][3]" in header and "batch_boxes=1" in header


def test_python_argument_errors_without_a_gpu():
    from NNPOps import OptimizedTorchANI
    from NNPOps.SymmetryFunctions import TorchANISymmetryFunctions
    model = workloads.torchani_like_model(n_models=2, seed=3)
    species, coords, cells = pb.module_frames()
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]])
    x, cell = torch.tensor(coords), torch.tensor(cells)
    yes, partly = torch.tensor([True, True, True]), torch.tensor([True, True, False])
    aev = TorchANISymmetryFunctions(model.species_converter, model.aev_computer, numbers)
    assert "cell" in inspect.signature(aev.forward_batch).parameters and "pbc" in inspect.signature(aev.forward_batch).parameters
    assert aev.check_batch_arguments(x, cell, yes) == 3 and aev.check_batch_arguments(x) == 3
    assert aev.batch_holder(3, True) is aev.batch_holder(3, True) and aev.batch_holder(3, True) is not aev.batch_holder(3)
    modules = [OptimizedTorchANI(model, numbers), OptimizedTorchANI(model, numbers, fused_step=False),
               OptimizedTorchANI(model, numbers, trainable=True), OptimizedTorchANI(model, numbers, force_trainable=True)]
    for module in modules:
        methods = [module.forward_batch, module.members_energies_batch, module.energies_qbcs_batch]
        if hasattr(module, "energy_and_forces_batch"):
            methods.append(module.energy_and_forces_batch)
        for method in methods:
            with pytest.raises(ValueError, match="non-periodic"):          # a single frame's cell
                method((numbers, x), cell[0], yes)
            with pytest.raises(ValueError, match="non-periodic"):          # pbc without a cell
                method((numbers, x), None, yes)
            with pytest.raises(ValueError, match=r"\[3, 3, 3\]"):          # a wrong leading size
                method((numbers, x), cell[:2], yes)
            with pytest.raises(ValueError, match='"pbc" has to be defined'):
                method((numbers, x), cell, None)
            with pytest.raises(ValueError, match="Only fully periodic systems are supported"):
                method((numbers, x), cell, partly)
    for module in modules[:2]:                       # forward and the scripted modules are unchanged
        torch.jit.script(module)
