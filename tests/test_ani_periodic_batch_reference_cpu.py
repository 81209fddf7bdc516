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
import functools
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


def _cell_gradient_against_central_differences(species, pos, box, seed):
    """-> (the judge's evaluation at the centre, largest |central difference - gbox| over the nine entries, largest |gbox|, weights)"""
    functions = workloads.ani2x_functions()
    rest = Restatement(pb.N_SPECIES, pb.RCR, pb.RCA, species, *functions)
    wr, wa = pb.weights(len(species), seed)
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
    return centre, worst, top, (wr, wa)


def test_cell_gradient_of_one_molecule_against_central_differences():
    species, pos, box = pb.frames()[1]                 # the triclinic frame: every one of the nine entries moves a displacement
    functions = workloads.ani2x_functions()
    centre, worst, top, (wr, wa) = _cell_gradient_against_central_differences(species, pos, box, 6)
    print(f"\n[ani-pbatch-reference] cell gradient of the triclinic molecule vs central differences: {worst / top:.2e} of max {top:.3e}")
    assert worst <= FD_RTOL * top, (worst, top)
    # ... and it is the entry of the batch judge for that molecule
    sp, x, boxes, offsets = pb.batch()
    wr_b, wa_b = np.zeros((547, wr.shape[1]), np.float32), np.zeros((547, wa.shape[1]), np.float32)
    wr_b[130:330], wa_b[130:330] = wr, wa
    out = pb.judge(sp, x, boxes, offsets, functions, True, wr_b, wa_b)
    assert np.array_equal(out["gbox"][1], centre["gbox"]) and not out["gbox"][[0, 2, 3]].any()


# ---------------------------------------------------------------------------------------------- the edge batches
# (tests/test_ani_periodic_batch_edges_gpu.py runs them; here: every frame reaches the edge it is named for, by the reference alone)
def _census_line(name, m, frame, c):
    print(f"\n[ani-pbatch-reference] {name} molecule {m}: {len(frame[0])} atoms, widths {['%.2f' % w for w in c['width']]}, pairs {c['pairs']}, "
          f"shifted {c['shifted']} (per axis {c['per_axis']}), triples {c['triples']}", end="")


@functools.lru_cache(maxsize=None)
def _edge_census(name):
    frames = dict(size_edges=pb.size_edge_frames, many_molecules=pb.many_molecule_frames, dense_pair=pb.dense_pair_frames)[name]()
    return [pb.census(*frame) for frame in frames]


@pytest.mark.parametrize("name", ["size_edges", "many_molecules", "dense_pair"])
def test_edge_batches_keep_the_contract_of_two_cutoffs(name):
    frames = dict(size_edges=pb.size_edge_frames, many_molecules=pb.many_molecule_frames, dense_pair=pb.dense_pair_frames)[name]()
    boxes = [f[2] for f in frames]
    for m, (frame, c) in enumerate(zip(frames, _edge_census(name))):
        _census_line(name, m, frame, c)
        assert min(c["width"]) >= 2 * pb.RCR, (name, m, c)
        assert np.array_equal(np.triu(frame[2], 1), np.zeros((3, 3), np.float32))          # (rows = box vectors, reduced form)
        if len(frame[0]) >= 2:
            assert all(n > 0 for n in c["per_axis"]), (name, m, c)
    assert len({b.tobytes() for b in boxes}) == len(boxes), "two molecules share a box"
    triclinic = sum(bool(np.count_nonzero(b - np.diag(np.diag(b)))) for b in boxes)
    if name == "size_edges":
        assert [len(f[0]) for f in frames] == list(pb.SIZE_EDGES) and pb.size_edges()[3].tolist()[-1] == 957
        assert triclinic == 4 and all(np.count_nonzero(frames[m][2] - np.diag(np.diag(frames[m][2]))) == 3 for m in (4, 5, 6, 9))
    elif name == "many_molecules":
        assert [len(f[0]) for f in frames] == [1 + m % 9 for m in range(70)] and pb.many_molecules()[3].tolist()[-1] == 343
        assert 23 <= triclinic <= 24                                                       # a third of the boxes
    else:
        assert [len(f[0]) for f in frames] == [230, 300]
    # the slots128 batch has cutoffs of its own: 2 x 5.2
    for sp, x, box in pb.slots128_frames():
        assert min(float(box[a, a]) for a in range(3)) >= 2 * pb.SLOTS128[1], box
    assert [len(f[0]) for f in pb.slots128_frames()] == [400, 300]
    from ani_float64 import system
    assert np.array_equal(pb.slots128_frames()[0][1], system("slots128")[4]) and pb.SLOTS128 == system("slots128")[:3]


def test_tiny_molecules_have_the_pairs_and_triples_they_are_named_for():
    frames, counts = pb.size_edge_frames(), _edge_census("size_edges")
    one, two, three, four, five = (counts[m] for m in (1, 3, 5, 7, 9))
    assert one["pairs"] == 0 and one["triples"] == 0
    assert two["pairs"] == 2 and two["triples"] == 0 and two["shifted"] == 2 and two["per_axis"] == [2, 2, 2]
    assert three["pairs"] == 6 and three["triples"] == 1
    # the 3-atom molecule: one centre with two angular neighbours, two with a lone leg whose partner is radial only
    species, pos, box = frames[5]
    assert pb.angular_counts(species, pos, box).tolist() == [2, 1, 1]
    rest = Restatement(pb.N_SPECIES, pb.RCR, pb.RCA, species, *workloads.ani2x_functions())
    p, b = pos.astype(np.float64), box.astype(np.float64)
    n = rest.shifts(p, b)
    d12 = p[2] - p[1] + n[1, 2] @ b
    assert pb.RCA < float(np.linalg.norm(d12)) < pb.RCR
    u, v = p[1] - p[0] + n[0, 1] @ b, p[2] - p[0] + n[0, 2] @ b
    angle = np.degrees(np.arccos(u @ v / np.linalg.norm(u) / np.linalg.norm(v)))
    assert 140.0 < angle < 150.0, angle          # (bent: at 180 degrees the angle of the paper's convention has no derivative)
    # the 5-atom molecule: its first atom has no neighbour inside the radial cutoff, the other four -- the last of them the one
    # atom of the molecule's second workgroup -- see one another
    species, pos, box = frames[9]
    (pi, pj, pn), _ = Restatement(pb.N_SPECIES, pb.RCR, pb.RCA, species, *workloads.ani2x_functions()).lists(pos.astype(np.float64), box.astype(np.float64))
    assert 0 not in pi and 0 not in pj and five["pairs"] == 12 and (pn[pi == 4] != 0).any(axis=0).all()
    out = pb.judge(species, pos, box[None], np.array([0, 5]), workloads.ani2x_functions())
    assert not out["r"][0].any() and not out["a"][0].any() and out["r"][1:].any(axis=1).all()
    assert four["pairs"] == 12
    # the last atom of the 257- and of the 65-atom liquids (the second round's, the 17th workgroup's only atom) has shifted pairs
    # on every axis, inside the angular cutoff too: dropping it or counting it twice moves every row of the molecule's dL/dB
    for m in (0, 6):
        species, pos, box = frames[m]
        rest = Restatement(pb.N_SPECIES, pb.RCR, pb.RCA, species, *workloads.ani2x_functions())
        (pi, pj, pn), _ = rest.lists(pos.astype(np.float64), box.astype(np.float64))
        mine = pn[pi == len(species) - 1]
        print(f"\n[ani-pbatch-reference] size_edges molecule {m}: its last atom at {pos[-1]} has {len(mine)} pairs, shifted per axis "
              f"{(mine != 0).sum(axis=0).tolist()}", end="")
        assert (mine != 0).sum(axis=0).min() >= 5, (m, mine)
    # a tiny box is more than 1.5 times as wide as the first molecule's on some axis (and the first is the widest nowhere): a shift
    # recovered against the wrong molecule's box is another integer
    first = float(frames[0][2][0, 0])
    assert max(float(frames[m][2][a, a]) for m in (1, 3, 5, 7, 9) for a in range(3)) > 1.5 * first
    widths = np.array([[float(f[2][a, a]) for a in range(3)] for f in pb.many_molecule_frames()])
    assert (widths.max(axis=0) > 1.5 * widths[0]).all() and (widths.max(axis=0) > 1.5 * widths[-1]).all()
    # spacings inside the clusters: no two atoms closer than 0.9 A
    for m in (3, 5, 7, 9):
        species, pos, box = frames[m]
        p, b = pos.astype(np.float64), box.astype(np.float64)
        rest = Restatement(pb.N_SPECIES, pb.RCR, pb.RCA, species, *workloads.ani2x_functions())
        d = p[None] - p[:, None] + rest.shifts(p, b) @ b
        r = np.linalg.norm(d, axis=2)[np.triu_indices(len(p), 1)]
        assert r.min() >= 0.9 - 1e-5, (m, r.min())


def test_workgroup_counts_of_the_box_gradient_pass():
    sizes = [len(f[0]) for f in pb.size_edge_frames()]
    assert [pb.molecule_blocks(n) for n in sizes] == [64, 1, 16, 1, 64, 1, 17, 1, 64, 2]
    assert [n > 64 * 4 for n in sizes] == [True, False, False, False, True, False, False, False, False, False]      # a second round of the stride loop
    assert pb.molecule_blocks(0) == 1 and pb.molecule_blocks(4) == 1 and pb.molecule_blocks(5) == 2 and pb.molecule_blocks(10 ** 6) == 64
    many = [pb.molecule_blocks(len(f[0])) for f in pb.many_molecule_frames()]
    assert len(many) == 70 and sorted(set(many)) == [1, 2, 3] and sum(many) == 7 * 15 + 10
    # the re-partition of test_repartitioning_a_live_handle: 35 molecules, other table lengths, records that never grow
    _, _, boxes, offsets = pb.many_molecules()
    boxes2, offsets2 = pb.paired(boxes, offsets)
    assert len(offsets2) == 36 and boxes2.shape == (35, 3, 3) and int(offsets2[-1]) == 343 and set(offsets2.tolist()) < set(offsets.tolist())
    sizes2 = np.diff(offsets2)
    assert sizes2.max() <= 17 and sum(pb.molecule_blocks(n) for n in sizes2) != sum(many)


def test_dense_frames_reach_the_scattered_backward_and_the_wide_records():
    total = 0
    for m, (frame, c) in enumerate(zip(pb.dense_pair_frames(), _edge_census("dense_pair"))):
        na = pb.angular_counts(*frame)
        total += c["triples"]
        print(f"\n[ani-pbatch-reference] dense_pair molecule {m}: {c['triples'] / len(frame[0]):.1f} triples per atom, angular neighbours "
              f"{na.min()} .. {na.max()}", end="")
        assert c["triples"] == int((na * (na - 1) // 2).sum())
        assert c["triples"] / len(frame[0]) >= 200.0          # (the threshold of $NNPOPS_ANI_SCATTER's default: two waves per atom)
        assert 32 < na.max() <= 64                             # records of 64 slots
    assert total / 530 >= 200.0                                # (what the handle sees: the mean over the batch)
    n_species, rcr, rca = pb.SLOTS128
    for m, frame in enumerate(pb.slots128_frames()):
        na = pb.angular_counts(*frame, rcr=rcr, rca=rca)
        print(f"\n[ani-pbatch-reference] slots128 molecule {m}: angular neighbours {na.min()} .. {na.max()}", end="")
        assert 64 < na.max() <= 128 and int(frame[0].max()) == n_species - 1


def test_judge_is_the_float32_oracle_on_the_edge_frames():
    functions = workloads.ani2x_functions()
    for name, frame in (("257 atoms", pb.size_edge_frames()[0]), ("230 atoms", pb.dense_pair_frames()[0])):
        species, pos, box = frame
        out = pb.judge(species, pos, box[None], np.array([0, len(species)]), functions)
        oracle = AniOracle(pb.N_SPECIES, pb.RCR, pb.RCA, species, *functions, periodic=True, torchani=True)
        r_ref, a_ref = oracle.forward(pos, box)
        print(f"\n[ani-pbatch-reference] {name}: judge against the float32 oracle, radial {np.abs(out['r'] - r_ref).max():.2e} angular "
              f"{np.abs(out['a'] - a_ref).max():.2e}", end="")
        np.testing.assert_allclose(out["r"], r_ref, rtol=AEV_RTOL, atol=AEV_ATOL)
        np.testing.assert_allclose(out["a"], a_ref, rtol=AEV_RTOL, atol=AEV_ATOL)


@pytest.mark.parametrize("which", [3, 5], ids=["two_atoms", "three_atoms"])
def test_cell_gradient_of_the_tiny_molecules_against_central_differences(which):
    species, pos, box = pb.size_edge_frames()[which]
    centre, worst, top, _ = _cell_gradient_against_central_differences(species, pos, box, 20 + which)
    print(f"\n[ani-pbatch-reference] cell gradient of the {len(species)}-atom molecule vs central differences: {worst / top:.2e} of max {top:.3e}")
    assert top > 0 and np.count_nonzero(centre["gbox"]) == 9
    assert worst <= FD_RTOL * top, (worst, top)


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
