"""Periodic batches of the ANI symmetry functions at the edges of molecule size and of the backward dispatch: the C ABI
(nnpops_ani_set_molecules on a periodic handle, compute, backprop, backprop_box, tangent, describe) against float64.

The batches and the judge are those of tests/ani_periodic_batch_float64.py, pinned by tests/test_ani_periodic_batch_reference_cpu.py:
    size_edges()       molecules of 257, 1, 64, 2, 300, 3, 65, 4, 256, 5 atoms: a second round of the stride loop of
                       ani_box_partials_molecules (more than 64 workgroups x 4 waves), one workgroup, waves without an atom, a centre
                       with a lone angular leg, an atom without a neighbour, the remainders around 64 and 256
    many_molecules()   70 molecules of 1 .. 9 atoms: more molecules than a finishing workgroup has waves, workgroup counts 1, 2, 3
    dense_pair()       230 + 300 atoms at density 0.2: records of 64 slots, the two-wave backward, leg forces in the receivers' rows
    slots128_pair()    400 + 300 atoms, 3 species, cutoffs 5.2 / 4.8: records of 128 slots
Every float64 reference is computed once per module run and not changed.

Bars (those of test_ani_periodic_batch_gpu.py): the AEV at rtol 2e-5 + atol 2e-6; gradients and tangents at 1e-4 of the largest
entry, the box gradient PER MOLECULE against that molecule's largest float64 entry, the adjoint identity to 1e-4 of the sum of the
absolute terms.  Where the float64 entries are exactly zero -- everything of the 1-atom molecule, the rows of the atom without a
neighbour -- the device's must be exactly zero.  Every evaluation prints its measured figures (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import ani_periodic_batch_float64 as pb
from ani_float64 import system
from ani_tangent_float64 import block_errors, functions
from box_gradient_judge import clean_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
AEV_RTOL, AEV_ATOL, FORCE_RTOL = 2e-5, 2e-6, 1e-4
TANGENT_BAR = 1e-4
ANI2X = (pb.N_SPECIES, pb.RCR, pb.RCA)


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


BATCHES = dict(size_edges=pb.size_edges, many_molecules=pb.many_molecules, dense_pair=pb.dense_pair, slots128=pb.slots128_pair)


@functools.lru_cache(maxsize=None)
def _reference(name, fset="ani2x", torchani=True):
    """float64 judge of a whole batch: dict(r, a, g, gbox, L, Lm, wr, wa), once per (batch, function list, angle convention)"""
    species, pos, boxes, offsets = BATCHES[name]()
    n_species, rcr, rca = pb.SLOTS128 if name == "slots128" else ANI2X
    fn = functions(fset)
    wr, wa = pb.weights(len(species), 31 + int(torchani), n_angular=len(np.asarray(fn[1]).reshape(-1, 4)), n_species=n_species)
    out = pb.judge(species, pos, boxes, offsets, fn, torchani, wr, wa, n_species=n_species, rcr=rcr, rca=rca)
    out.update(wr=wr, wa=wa)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _handle(species, offsets, fset="ani2x", torchani=True, config=ANI2X):
    from nnpops_amd.capi import AniSymmetryFunctions
    sym = AniSymmetryFunctions(*config, species, *functions(fset), periodic=True, torchani=torchani)
    sym.set_molecules(offsets)
    return sym


def _run(sym, tpos, tboxes, wr, wa):
    """compute, backprop_box -> clones of (radial, angular, position gradient, box gradient)"""
    radial, angular = sym.compute(tpos, tboxes)
    g, gbox = sym.backprop_box(tpos, tboxes, wr, wa)
    torch.cuda.synchronize()
    return radial.clone(), angular.clone(), g.clone(), gbox.clone()


def _zero_rows(ref):
    """atoms whose float64 AEV is exactly zero (no neighbour inside the radial cutoff)"""
    return np.nonzero(~(ref["r"].any(axis=1) | ref["a"].any(axis=1)))[0]


def _check_aev(label, radial, angular, ref):
    r, a = radial.cpu().numpy().astype(np.float64), angular.cpu().numpy().astype(np.float64)
    er, ea = float(np.abs(r - ref["r"]).max()), float(np.abs(a - ref["a"]).max())
    lone = _zero_rows(ref)
    print(f"\n[ani-pbatch-edges] {label}: AEV off by up to {er:.2e} (radial) {ea:.2e} (angular); {len(lone)} atoms without a neighbour: "
          f"largest entry of their rows {max(float(np.abs(r[lone]).max(initial=0)), float(np.abs(a[lone]).max(initial=0))):.1e}", end="")
    np.testing.assert_allclose(r, ref["r"], rtol=AEV_RTOL, atol=AEV_ATOL)
    np.testing.assert_allclose(a, ref["a"], rtol=AEV_RTOL, atol=AEV_ATOL)
    assert not r[lone].any() and not a[lone].any(), (label, "the AEV of an atom without a neighbour is not exactly zero")


def _check_gradients(label, g, gbox, ref, pos, boxes, offsets):
    g, gbox = g.cpu().numpy().astype(np.float64), gbox.cpu().numpy().astype(np.float64)
    assert gbox.shape == ref["gbox"].shape and np.isfinite(gbox).all() and np.isfinite(g).all()
    err_g = float(np.abs(g - ref["g"]).max() / np.abs(ref["g"]).max())
    tops = [float(np.abs(ref["gbox"][m]).max()) for m in range(len(gbox))]
    errs = [float(np.abs(gbox[m] - ref["gbox"][m]).max()) / (tops[m] if tops[m] > 0 else 1.0) for m in range(len(gbox))]
    worst = int(np.argmax(errs))
    anti = pb.stress_antisymmetry(pos, boxes, offsets, g, gbox)
    ratios = [a / w if w > 0 else a for a, w in anti]
    print(f"\n[ani-pbatch-edges] {label}: position gradient {err_g:.2e} of max; box gradient per molecule, worst {errs[worst]:.2e} of the "
          f"molecule's max (molecule {worst}, {int(offsets[worst + 1] - offsets[worst])} atoms){'' if len(errs) > 10 else ' ' + str(['%.1e' % e for e in errs])}; "
          f"antisymmetric stress up to {max(ratios):.2e} of the molecule's largest entry", end="")
    assert err_g <= FORCE_RTOL, (label, err_g)
    for m, (e, top) in enumerate(zip(errs, tops)):
        if top > 0:
            assert e <= FORCE_RTOL, (label, m, errs)
        else:                                          # (no shifted pair in the molecule: nothing to sum)
            assert not gbox[m].any(), (label, m, gbox[m])
    for m, (a, w) in enumerate(anti):                  # rotation invariance, molecule by molecule
        assert a <= FORCE_RTOL * w, (label, m, a, w)
    lone = _zero_rows(ref)
    assert not ref["g"][lone].any() and not g[lone].any(), (label, "the gradient of an atom without a neighbour is not exactly zero")


# ---------------------------------------------------------------------------------------------- molecule sizes
CASES = [("ani2x", True), ("ani2x", False), ("no_grid", True)]


@pytest.mark.parametrize("fset,torchani", CASES, ids=["torchani", "paper", "generic"])
def test_size_edges_against_float64(monkeypatch, fset, torchani):
    clean_env(monkeypatch, "NNPOPS_ANI_")
    ref = _reference("size_edges", fset, torchani)
    species, pos, boxes, offsets = pb.size_edges()
    assert len(species) == 957 and not ref["gbox"][1].any() and ref["gbox"][[0, 2, 3, 4, 5, 6, 7, 8, 9]].any(axis=(1, 2)).all()
    assert _zero_rows(ref).tolist() == [257, 952]       # the 1-atom molecule and the 5-atom molecule's first atom
    sym = _handle(species, offsets, fset, torchani)
    tpos, tboxes, wr, wa = _t(pos), _t(boxes), _t(ref["wr"]), _t(ref["wa"])
    radial, angular, g, gbox = _run(sym, tpos, tboxes, wr, wa)
    what = sym.describe()
    assert what["batch_boxes"] == "1" and what["cells"] == "0" and what["fused_build"] == "0", what
    assert what["generic"] == ("1" if fset == "no_grid" else "0"), what
    assert gbox.shape == (10, 3, 3) and gbox.dtype == torch.float32
    label = f"size_edges {fset} torchani={torchani}"
    _check_aev(label, radial, angular, ref)
    _check_gradients(label, g, gbox, ref, pos, boxes, offsets)
    assert torch.equal(gbox[1], torch.zeros_like(gbox[1])), "the 1-atom molecule has a box gradient"
    again = _run(sym, tpos, tboxes, wr, wa)
    assert all(torch.equal(a, b) for a, b in zip(again, (radial, angular, g, gbox))), "two calls give different bits"
    assert torch.equal(sym.backprop(wr, wa), g), "the position gradient is not the plain backprop()'s"


def test_size_edges_tangent(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_ANI_")
    ref = _reference("size_edges")
    species, pos, boxes, offsets = pb.size_edges()
    v = np.random.default_rng([957, 4]).standard_normal((957, 3)).astype(np.float32)
    want = pb.tangent(species, pos, boxes, offsets, functions("ani2x"), v)
    sym = _handle(species, offsets)
    tpos, tboxes, wr, wa, tv = _t(pos), _t(boxes), _t(ref["wr"]), _t(ref["wa"]), _t(v)
    sym.compute(tpos, tboxes)
    force = sym.backprop(wr, wa).clone()
    first = tuple(t.clone() for t in sym.tangent(tv))
    second = sym.tangent(tv)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    got = tuple(t.cpu().numpy() for t in first)
    er, ea = block_errors(got, want)
    left = float((wr.double() * first[0].double()).sum() + (wa.double() * first[1].double()).sum())
    right = float((force.double() * tv.double()).sum())
    size = float((wr * first[0]).abs().double().sum() + (wa * first[1]).abs().double().sum() + (force * tv).abs().double().sum())
    print(f"\n[ani-pbatch-edges] size_edges tangent: radial {er:.2e} angular {ea:.2e} of the largest entry; <w, Jv> - <J^T w, v> = "
          f"{abs(left - right) / size:.2e} of the terms", end="")
    assert er <= TANGENT_BAR and ea <= TANGENT_BAR, (er, ea)
    assert abs(left - right) <= TANGENT_BAR * size, (left, right, size)
    # molecule by molecule, each against its own largest entry (a small molecule next to a liquid is not hidden by it)
    for m in range(10):
        rows = slice(int(offsets[m]), int(offsets[m + 1]))
        er_m, ea_m = block_errors((got[0][rows], got[1][rows]), (want[0][rows], want[1][rows]))
        print(f"\n[ani-pbatch-edges]   molecule {m} ({rows.stop - rows.start} atoms): radial {er_m:.2e} angular {ea_m:.2e}", end="")
        assert er_m <= TANGENT_BAR and ea_m <= TANGENT_BAR, (m, er_m, ea_m)
    lone = _zero_rows(ref)
    assert not want[0][lone].any() and not want[1][lone].any()
    assert not got[0][lone].any() and not got[1][lone].any(), "the tangent of an atom without a neighbour is not exactly zero"


WORDS = ("forward", "backward", "generic", "uniform", "literal", "dynamic_quads", "fused_build", "cap_angular", "chunk", "scatter", "bwd_mode",
         "radial_bwd", "batch_boxes")


@pytest.mark.parametrize("quads", ["per_atom", "by_species"])
def test_a_molecule_keeps_its_bits_in_any_company(monkeypatch, quads):
    """the 257-, the 300- and the 5-atom molecules each alone in a handle (a batch of one) against the ten-molecule batch: the order of
    every sum of a molecule depends on its atom count alone, so a mistake in the tables or in the stride shows as a difference of bits.

    The batch path keeps that promise; the matrix-core forward of the ANGULAR AEV keeps it only in one of its two dealings of quads.
    by_species (the default of these handles): nnpops_ani_create deals the quads to the species pairs that OCCUR among the handle's
        atoms (fwd_split in ani.hip) and a pair's triples to its K quads in turn, so the grouping of a block's fused sums follows the
        handle's set of species.  Measured on the MI355X: the 5-atom molecule alone (four species, K = 2) differs from its rows in the
        seven-species batch (K = 1) in 7 of its 320 non-zero angular entries by one unit in the last place (6.0e-8 next to 0.62; both
        9.6e-7 from float64); the same five atoms behind the 256-atom molecule give the batch's bits.  Here the angular AEV is compared
        wherever the two handles hold the same set of species (the 257- and the 300-atom molecules); everything else is compared always.
    per_atom ($NNPOPS_ANI_FWD_DYN=1 on both handles): the quads are dealt per atom from the atom's own bucket sizes, a function of
        the molecule alone.  All twelve comparisons, and the batch's AEV against float64 on that forward."""
    clean_env(monkeypatch, "NNPOPS_ANI_")
    if quads == "per_atom":
        monkeypatch.setenv("NNPOPS_ANI_FWD_DYN", "1")
    ref = _reference("size_edges")
    species, pos, boxes, offsets = pb.size_edges()
    sym = _handle(species, offsets)
    batch = _run(sym, _t(pos), _t(boxes), _t(ref["wr"]), _t(ref["wa"]))
    words = {k: sym.describe()[k] for k in WORDS}
    assert words["dynamic_quads"] == ("1" if quads == "per_atom" else "0"), words
    _check_aev(f"size_edges, quads dealt {quads}", batch[0], batch[1], ref)
    differing = []
    for m in (0, 4, 9):
        lo, hi = int(offsets[m]), int(offsets[m + 1])
        assert hi - lo == (257, 300, 5)[(0, 4, 9).index(m)]
        one = _handle(species[lo:hi], [0, hi - lo])
        alone = _run(one, _t(pos[lo:hi]), _t(boxes[m:m + 1]), _t(ref["wr"][lo:hi]), _t(ref["wa"][lo:hi]))
        words_one = {k: one.describe()[k] for k in WORDS}
        same_species = set(species[lo:hi].tolist()) == set(species.tolist())
        print(f"\n[ani-pbatch-edges] molecule {m} ({hi - lo} atoms) alone, quads dealt {quads}, {len(set(species[lo:hi].tolist()))} species: {words_one}", end="")
        assert words_one == words, (words_one, words)          # (both handles run the same kernels: the comparison is one of bits)
        assert alone[3].shape == (1, 3, 3) and float(alone[3].abs().max()) > 0
        for name, a, b in zip(("radial", "angular", "position gradient", "box gradient"), alone, batch[:3] + (batch[3][m:m + 1],)):
            b = b if name == "box gradient" else b[lo:hi]
            n_diff, largest = int((a != b).sum()), float((a - b).abs().max())
            compared = name != "angular" or quads == "per_atom" or same_species
            print(f"\n[ani-pbatch-edges]   {name}: {n_diff} of {a.numel()} entries differ, by up to {largest:.1e}"
                  f"{'' if compared else ' (other species in the handle, other dealing: not compared)'}", end="")
            if compared and not torch.equal(a, b):
                differing.append(f"{name} of molecule {m} ({hi - lo} atoms): {n_diff} entries, up to {largest:.1e}")
    assert not differing, ("a molecule's bits depend on its companions", differing)


# ---------------------------------------------------------------------------------------------- many molecules
def test_many_molecules_against_float64(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_ANI_")
    ref = _reference("many_molecules")
    species, pos, boxes, offsets = pb.many_molecules()
    M = len(boxes)
    assert M == 70 and len(species) == 343
    sym = _handle(species, offsets)
    out = _run(sym, _t(pos), _t(boxes), _t(ref["wr"]), _t(ref["wa"]))
    assert sym.describe()["batch_boxes"] == "1" and out[3].shape == (70, 3, 3)
    _check_aev("many_molecules", out[0], out[1], ref)
    _check_gradients("many_molecules", out[2], out[3], ref, pos, boxes, offsets)
    single = [m for m in range(M) if offsets[m + 1] - offsets[m] == 1]
    assert len(single) == 8 and not out[3][single].any(), "a 1-atom molecule has a box gradient"
    # the same molecules in reversed order behind a second handle: every molecule's bits at its new place
    frames = pb.many_molecule_frames()[::-1]
    species_r, pos_r, boxes_r, offsets_r = pb.assemble(frames)
    rows = np.concatenate([np.arange(offsets[m], offsets[m + 1]) for m in range(M - 1, -1, -1)])
    assert np.array_equal(pos_r, pos[rows]) and np.array_equal(boxes_r, boxes[::-1])
    rev = _handle(species_r, offsets_r)
    out_r = _run(rev, _t(pos_r), _t(boxes_r), _t(ref["wr"][rows]), _t(ref["wa"][rows]))
    trows = torch.tensor(rows, device=DEV)
    for name, a, b in zip(("radial", "angular", "position gradient"), out[:3], out_r[:3]):
        assert torch.equal(a[trows], b), f"{name} of a molecule depends on its place in the batch"
    assert torch.equal(out[3].flip(0), out_r[3]), "the box gradient of a molecule depends on its place in the batch"


def test_repartitioning_a_live_handle(monkeypatch):
    """set_molecules on a handle that has run: 70 molecules, then the same atoms as 35 (neighbours two by two under the box of the
    first: other table lengths, 343 atoms in 17-atom molecules at the most so no record grows), then 70 again -- the bits of the first
    run and of a fresh handle.  (The ten molecules of size_edges() cannot be merged this way: a 64-atom liquid laid over a 300-atom one
    outgrows the 32-slot records, and a handle that has grown its records is no longer comparable by bits with a fresh one.)"""
    clean_env(monkeypatch, "NNPOPS_ANI_")
    ref = _reference("many_molecules")
    species, pos, boxes, offsets = pb.many_molecules()
    boxes2, offsets2 = pb.paired(boxes, offsets)
    tpos, tboxes, tboxes2, wr, wa = _t(pos), _t(boxes), _t(boxes2), _t(ref["wr"]), _t(ref["wa"])
    sym = _handle(species, offsets)
    first = _run(sym, tpos, tboxes, wr, wa)
    before = sym.describe()
    sym.set_molecules(offsets2)
    with pytest.raises(ValueError, match="box"):       # (one box per molecule: the 70 boxes no longer fit)
        sym.compute(tpos, tboxes)
    merged = _run(sym, tpos, tboxes2, wr, wa)
    assert merged[3].shape == (35, 3, 3) and all(bool(torch.isfinite(t).all()) for t in merged)
    assert not torch.equal(merged[0], first[0]), "merging the molecules changed nothing"
    assert {k: sym.describe()[k] for k in ("cap", "cap_angular")} == {k: before[k] for k in ("cap", "cap_angular")}
    sym.set_molecules(offsets)
    back = _run(sym, tpos, tboxes, wr, wa)
    assert sym.describe() == before
    fresh = _run(_handle(species, offsets), tpos, tboxes, wr, wa)
    for name, a, b, c in zip(("radial", "angular", "position gradient", "box gradient"), first, back, fresh):
        assert torch.equal(a, b), f"{name} differs after re-partitioning the handle twice"
        assert torch.equal(a, c), f"{name} of a fresh handle differs"
    _check_gradients("many_molecules, re-partitioned 70 -> 35 -> 70", back[2], back[3], ref, pos, boxes, offsets)


# ---------------------------------------------------------------------------------------------- every backward path on the dense batch
CLASS_LAUNCHES = (("BWD_CLASSES", "1"), ("BWD_CLASS_MIN", "0"), ("BWD_CLASS_ATOMS", "0"))
SWITCHES = ([("default", ()), ("SCATTER=0", (("SCATTER", "0"),)), ("SCATTER=1", (("SCATTER", "1"),))]
            + [(f"BACKWARD={v}", (("BACKWARD", v),)) for v in "01234"]
            + [("RBWD=0", (("RBWD", "0"),)), ("GENERIC=1", (("GENERIC", "1"),)), ("LPT=0", (("LPT", "0"),)),
               ("classes-SCATTER=0", CLASS_LAUNCHES + (("SCATTER", "0"),)), ("classes-SCATTER=1", CLASS_LAUNCHES + (("SCATTER", "1"),))])


def _dense_run(monkeypatch, settings):
    for k, v in settings:
        monkeypatch.setenv("NNPOPS_ANI_" + k, v)
    ref = _reference("dense_pair")
    species, pos, boxes, offsets = pb.dense_pair()
    sym = _handle(species, offsets)
    out = _run(sym, _t(pos), _t(boxes), _t(ref["wr"]), _t(ref["wa"]))
    return out, sym.describe()


@pytest.mark.parametrize("name,settings", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_dense_batch_every_backward_path(monkeypatch, name, settings):
    clean_env(monkeypatch, "NNPOPS_ANI_")
    ref = _reference("dense_pair")
    species, pos, boxes, offsets = pb.dense_pair()
    out, what = _dense_run(monkeypatch, settings)
    label = (f"dense_pair {name}: scatter={what['scatter']} bwd_mode={what['bwd_mode']} radial_bwd={what['radial_bwd']} generic={what['generic']} "
             f"classes={what['classes']} cap_angular={what['cap_angular']}")
    print(f"\n[ani-pbatch-edges] {label}", end="")
    assert what["batch_boxes"] == "1" and what["cells"] == "0" and what["fused_build"] == "0" and what["cap_angular"] == "64", what
    switch = dict(settings)
    if name in ("default", "LPT=0"):                   # more than 200 triples per atom: two waves per atom, leg forces in the receivers' rows
        assert what["scatter"] == "1" and what["bwd_mode"] == "3" and what["radial_bwd"] == "lanes" and what["generic"] == "0", what
    if "SCATTER" in switch:
        assert what["scatter"] == switch["SCATTER"] and what["bwd_mode"] == "3" and what["radial_bwd"] == "lanes", what
    if "BACKWARD" in switch:                           # (a forced kernel parks its leg forces)
        assert what["backward"] == switch["BACKWARD"] and what["bwd_mode"] == switch["BACKWARD"] and what["scatter"] == "0", what
    if "RBWD" in switch:
        assert what["radial_bwd"] == "rows" and what["scatter"] == "0", what
    else:
        assert what["radial_bwd"] == "lanes", what
    if "GENERIC" in switch:
        assert what["generic"] == "1" and what["scatter"] == "0", what
    if "BWD_CLASSES" in switch:                        # (no atom has more than 44 neighbours: the top class is empty, bwd_mode is the next one's)
        assert int(what["classes"]) >= 1, what
    _check_aev(label, out[0], out[1], ref)
    _check_gradients(label, out[2], out[3], ref, pos, boxes, offsets)
    if name == "LPT=0":                                # only another schedule: the bits of the default run
        clean_env(monkeypatch, "NNPOPS_ANI_")
        default, default_what = _dense_run(monkeypatch, ())
        assert {k: default_what[k] for k in WORDS} == {k: what[k] for k in WORDS}, (default_what, what)
        for word, a, b in zip(("radial", "angular", "position gradient", "box gradient"), out, default):
            assert torch.equal(a, b), f"{word} depends on the schedule of the angular kernels"


# ---------------------------------------------------------------------------------------------- records of 128 slots
def test_slots128_batch_against_float64(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_ANI_")
    ref = _reference("slots128")
    species, pos, boxes, offsets = pb.slots128_pair()
    assert offsets.tolist() == [0, 400, 700] and pb.SLOTS128 == system("slots128")[:3]
    sym = _handle(species, offsets, config=pb.SLOTS128)
    tpos, tboxes, wr, wa = _t(pos), _t(boxes), _t(ref["wr"]), _t(ref["wa"])
    out = _run(sym, tpos, tboxes, wr, wa)
    what = sym.describe()
    label = f"slots128 scatter={what['scatter']} bwd_mode={what['bwd_mode']} radial_bwd={what['radial_bwd']} cap_angular={what['cap_angular']}"
    assert what["batch_boxes"] == "1" and what["cells"] == "0" and what["fused_build"] == "0" and what["cap_angular"] == "128", what
    _check_aev(label, out[0], out[1], ref)
    _check_gradients(label, out[2], out[3], ref, pos, boxes, offsets)
    again = _run(sym, tpos, tboxes, wr, wa)
    assert all(torch.equal(a, b) for a, b in zip(again, out)), "two calls give different bits"
