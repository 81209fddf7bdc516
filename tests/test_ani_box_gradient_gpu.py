"""Box-vector gradient (virial) of the ANI symmetry functions: nnpops_ani_backprop_box_strided and the torch surface above it.

The judge is the float64 restatement of tests/ani_float64.py (pinned by tests/test_ani_box_gradient_reference_cpu.py to
oracle.AniOracle64 and to finite differences of it): L = <w_r, radial> + <w_a, angular> with seeded float32 weights, dL/dB with the
minimum-image shifts held fixed, all nine entries.  One float64 evaluation per (system, angle mode), kept for the module.

Bar (the project's force tolerance, FORCE_RTOL of test_ani_dispatch_gpu.py): max |gB - gB_ref| <= 1e-4 max |gB_ref|.
Properties, same bar: the stress is symmetric -- the antisymmetric part of W = sum_i x_i (x) dL/dx_i + B^T dL/dB (rotation
invariance of the AEV) stays below 1e-4 of the largest entry of W; two calls give equal bits; the position gradient is the plain
backprop()'s, bit for bit.  Every evaluation prints its measured figures (pytest -s).
"""
import numpy as np
import pytest
import torch

from ani_float64 import Restatement, system
from box_gradient_judge import clean_env, judge
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu

FORCE_RTOL = 1e-4
DEV = torch.device("cuda:0")

_REFERENCES = {}


def _reference(tag, torchani):
    """float64: dict(g, gbox, wr, wa), once per (system, angle mode)"""
    key = (tag, torchani)
    if key not in _REFERENCES:
        n_species, rcr, rca, species, pos, box = system(tag)
        rf, af = workloads.ani2x_functions()
        base = tag.split("_")[0]                  # (the moved frames take the weights of the frame they come from)
        rng = np.random.default_rng([len(species), int(torchani), sum(map(ord, base))])
        wr = rng.standard_normal((len(species), 7 * 16)).astype(np.float32)
        wa = rng.standard_normal((len(species), 28 * 32)).astype(np.float32)
        out = Restatement(n_species, rcr, rca, species, rf, af, torchani).evaluate(pos, box, wr, wa)
        _REFERENCES[key] = dict(g=out["g"], gbox=out["gbox"], wr=wr, wa=wa)
    return _REFERENCES[key]


def _handle(tag, torchani):
    from nnpops_amd.capi import AniSymmetryFunctions
    n_species, rcr, rca, species, _, _ = system(tag)
    return AniSymmetryFunctions(n_species, rcr, rca, species, *workloads.ani2x_functions(), periodic=True, torchani=torchani)


def _evaluate(sym, tag, ref):
    """compute(), the plain backprop(), two backprop_box() -> (position gradient, cell gradient) as float64 numpy arrays"""
    _, _, _, _, pos, box = system(tag)
    tpos, tbox = torch.tensor(pos, device=DEV), torch.tensor(box, device=DEV)
    t_wr, t_wa = torch.tensor(ref["wr"], device=DEV), torch.tensor(ref["wa"], device=DEV)
    sym.compute(tpos, tbox)
    plain = sym.backprop(t_wr, t_wa).clone()
    g1, b1 = (t.clone() for t in sym.backprop_box(tpos, tbox, t_wr, t_wa))
    g2, b2 = sym.backprop_box(tpos, tbox, t_wr, t_wa)
    torch.cuda.synchronize()
    assert torch.equal(b1, b2), "two calls give different cell gradients"
    assert torch.equal(g1, plain) and torch.equal(g2, plain), "the position gradient is not the plain backprop()'s"
    assert b1.shape == (3, 3) and b1.dtype == torch.float32
    return g1.cpu().numpy().astype(np.float64), b1.cpu().numpy().astype(np.float64)


def _judge(label, tag, ref, g, gbox):
    _, _, _, _, pos, box = system(tag)
    judge("ani-box", label, pos, box, ref, g, gbox, FORCE_RTOL, what="cell gradient")


def _clean_env(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_ANI_")


# ---------------------------------------------------------------------------------------------- the systems
SYSTEMS = [("triclinic200", None), ("liquid600", None), ("dense900", None), ("dense900", "0"), ("liquid2100", None),
           ("liquid600_shifted", None), ("liquid600_wrapped", None)]


@pytest.mark.parametrize("torchani", [True, False], ids=["torchani", "paper"])
@pytest.mark.parametrize("tag,scatter", SYSTEMS, ids=[t + ("" if s is None else "-scatter" + s) for t, s in SYSTEMS])
def test_cell_gradient_against_float64(monkeypatch, tag, scatter, torchani):
    _clean_env(monkeypatch)
    if scatter is not None:
        monkeypatch.setenv("NNPOPS_ANI_SCATTER", scatter)
    ref = _reference(tag, torchani)
    sym = _handle(tag, torchani)
    g, gbox = _evaluate(sym, tag, ref)
    what = sym.describe()
    assert what["cells"] == ("1" if tag == "liquid2100" else "0"), what
    if tag == "dense900":
        assert what["cap_angular"] == "64" and what["bwd_mode"] == "3" and what["scatter"] == ("1" if scatter is None else "0"), what
    else:
        assert what["scatter"] == "0", what
    _judge(f"{tag} torchani={torchani} scatter={what['scatter']} cells={what['cells']} bwd_mode={what['bwd_mode']}", tag, ref, g, gbox)
    if tag == "liquid600_shifted":
        # the same frame somewhere else: no displacement changes, so neither does dL/dB -- up to the rounding of the moved float32
        # positions, which the float64 evaluations of the two frames show as well
        ref0 = _reference("liquid600", torchani)
        g0, gbox0 = _evaluate(_handle("liquid600", torchani), "liquid600", ref0)
        top = float(np.abs(ref0["gbox"]).max())
        moved, moved_ref = float(np.abs(gbox - gbox0).max()), float(np.abs(ref["gbox"] - ref0["gbox"]).max())
        print(f"[ani-box] liquid600 moved by 0.37 L: cell gradient changes by {moved / top:.2e} of max (float64: {moved_ref / top:.2e})")
        assert moved <= FORCE_RTOL * top, (moved, top)


# ---------------------------------------------------------------------------------------------- every backward path on the 600-atom frame
SWITCHES = [("BACKWARD", v) for v in "01234"] + [("RBWD", "0"), ("GENERIC", "1"), ("FUSE", "0"), ("FUSE", "1"), ("FINE_GRID", "0"),
                                                 ("BWD_CLASS_ATOMS", "0")]


@pytest.mark.parametrize("switch,value", SWITCHES, ids=[f"{s}={v}" for s, v in SWITCHES])
def test_cell_gradient_on_every_backward_path(monkeypatch, switch, value):
    _clean_env(monkeypatch)
    monkeypatch.setenv("NNPOPS_ANI_" + switch, value)
    if switch == "BWD_CLASS_ATOMS":
        monkeypatch.setenv("NNPOPS_ANI_BWD_CLASSES", "1")
        monkeypatch.setenv("NNPOPS_ANI_BWD_CLASS_MIN", "0")
    ref = _reference("liquid600", True)
    sym = _handle("liquid600", True)
    g, gbox = _evaluate(sym, "liquid600", ref)
    what = sym.describe()
    if switch == "BACKWARD":
        assert what["backward"] == value and what["bwd_mode"] == value, what
    elif switch == "RBWD":
        assert what["radial_bwd"] == "rows", what
    elif switch == "GENERIC":
        assert what["generic"] == "1", what
    elif switch == "FUSE":
        assert what["fused_build"] == value, what
    if switch != "RBWD":
        assert what["radial_bwd"] == "lanes", what
    _judge(f"liquid600 {switch}={value} bwd_mode={what['bwd_mode']} radial={what['radial_bwd']} fused={what['fused_build']} "
           f"classes={what['classes']}", "liquid600", ref, g, gbox)


@pytest.mark.parametrize("scatter", ["1", "0"])
def test_cell_gradient_behind_class_launches(monkeypatch, scatter):
    """Records of 32 slots are one class, so the 600-atom frame above runs the switch without class launches; the 64-slot dense
    frame is cut into classes (each followed by the clean-up launch), with the leg forces in either layout."""
    _clean_env(monkeypatch)
    for k, v in (("BWD_CLASSES", "1"), ("BWD_CLASS_MIN", "0"), ("BWD_CLASS_ATOMS", "0"), ("SCATTER", scatter)):
        monkeypatch.setenv("NNPOPS_ANI_" + k, v)
    ref = _reference("dense900", True)
    sym = _handle("dense900", True)
    g, gbox = _evaluate(sym, "dense900", ref)
    what = sym.describe()
    assert int(what["classes"]) >= 1 and what["scatter"] == scatter and what["cap_angular"] == "64", what
    _judge(f"dense900 classes={what['classes']} scatter={scatter} bwd_mode={what['bwd_mode']}", "dense900", ref, g, gbox)


def test_cell_gradient_with_the_coarse_cell_grid(monkeypatch):
    """$NNPOPS_ANI_FINE_GRID=0 only matters where the cell grid builds the rows (full-width cells, another row order)."""
    _clean_env(monkeypatch)
    monkeypatch.setenv("NNPOPS_ANI_FINE_GRID", "0")
    ref = _reference("liquid2100", True)
    sym = _handle("liquid2100", True)
    g, gbox = _evaluate(sym, "liquid2100", ref)
    assert sym.describe()["cells"] == "1", sym.describe()
    _judge("liquid2100 FINE_GRID=0", "liquid2100", ref, g, gbox)


def test_refused_without_a_box_or_with_molecules():
    from nnpops_amd.capi import AniSymmetryFunctions, NNPOpsHipError
    pos, species = workloads.conformer(40, seed=3)
    sym = AniSymmetryFunctions(7, 5.1, 3.5, species, *workloads.ani2x_functions(), periodic=False)
    tpos = torch.tensor(pos, device=DEV)
    radial, angular = sym.compute(tpos, None)
    with pytest.raises(NNPOpsHipError, match="periodic"):
        sym.backprop_box(tpos, torch.eye(3, device=DEV) * 50, torch.ones_like(radial), torch.ones_like(angular))
    sym.set_molecules([0, 20, 40])
    sym.compute(tpos, None)
    with pytest.raises(NNPOpsHipError):
        sym.backprop_box(tpos, torch.eye(3, device=DEV) * 50, torch.ones_like(radial), torch.ones_like(angular))


# ---------------------------------------------------------------------------------------------- the torch surface
Z_OF_SPECIES = [1, 6, 7, 8, 16, 9, 17]


def _numbers(species):
    return torch.tensor([[Z_OF_SPECIES[s] for s in species]], device=DEV)


def _aev_module(species):
    from NNPOps.SymmetryFunctions import TorchANISymmetryFunctions
    model = workloads.torchani_like_model(n_models=1, seed=0)
    return TorchANISymmetryFunctions(model.species_converter, model.aev_computer, _numbers(species).cpu()).to(DEV)


@pytest.mark.parametrize("surface", ["aev", "operation", "module"])
def test_torch_cell_gradient_is_the_c_abi_result(monkeypatch, surface):
    """cell.requires_grad_(): cell.grad is the C ABI's result bit for bit, positions.grad the bits of a run without a cell gradient;
    a cell that does not require a gradient still gets None."""
    _clean_env(monkeypatch)
    tag = "liquid600"
    _, _, _, species, pos, box = system(tag)
    ref = _reference(tag, True)
    module = _aev_module(species)
    w = torch.tensor(np.concatenate([ref["wr"], ref["wa"]], axis=1), device=DEV)

    def run(cell_grad):
        tpos = torch.tensor(pos, device=DEV).requires_grad_(True)
        cell = torch.tensor(box, device=DEV).requires_grad_(cell_grad)
        if surface == "aev":
            loss = (torch.ops.NNPOpsANISymmetryFunctions.aev(module.holder, tpos, cell) * w).sum()
        elif surface == "operation":
            radial, angular = torch.ops.NNPOpsANISymmetryFunctions.operation(module.holder, tpos, cell)
            loss = (radial * w[:, :112]).sum() + (angular * w[:, 112:]).sum()
        else:
            sp = torch.tensor(species, device=DEV).unsqueeze(0)
            loss = (module((sp, tpos.unsqueeze(0)), cell, torch.tensor([True, True, True], device=DEV))[1][0] * w).sum()
        loss.backward()
        return tpos.grad, cell.grad

    g_plain, none = run(False)
    assert none is None
    g, gcell = run(True)
    torch.cuda.synchronize()
    assert gcell is not None and gcell.shape == (3, 3)
    assert torch.equal(g, g_plain)
    g_abi, b_abi = _evaluate(_handle(tag, True), tag, ref)
    assert np.array_equal(gcell.cpu().numpy().astype(np.float64), b_abi)
    assert np.array_equal(g.cpu().numpy().astype(np.float64), g_abi)
    _judge(f"torch {surface} liquid600", tag, ref, g_abi, b_abi)


def test_torch_cell_gradient_refuses_second_derivatives(monkeypatch):
    _clean_env(monkeypatch)
    _, _, _, species, pos, box = system("triclinic200")
    module = _aev_module(species)
    tpos = torch.tensor(pos, device=DEV).requires_grad_(True)
    cell = torch.tensor(box, device=DEV).requires_grad_(True)
    for op in ("aev", "operation"):
        out = getattr(torch.ops.NNPOpsANISymmetryFunctions, op)(module.holder, tpos, cell)
        loss = out.sum() if op == "aev" else out[0].sum() + out[1].sum()
        with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
            torch.autograd.grad(loss, [tpos, cell], create_graph=True)


def test_optimized_torchani_cell_gradient_fused_against_composition(monkeypatch):
    """The fused step (one autograd node that keeps dE/dcell next to dE/dpositions) against the four-module composition, whose cell
    gradient comes through the AEV node: a periodic water box of the 2 001-atom benchmark's kind, 300 atoms."""
    _clean_env(monkeypatch)
    from NNPOps import OptimizedTorchANI
    model = workloads.torchani_like_model(n_models=2, seed=2)
    pos, species, box = workloads.water_box(100, seed=1)
    numbers = _numbers(species)
    pbc = torch.tensor([True, True, True], device=DEV)
    grads = {}
    for fused in (True, False):
        opt = OptimizedTorchANI(model, numbers.cpu(), fused_step=fused).to(DEV)
        assert (type(opt).__name__ == "FusedOptimizedTorchANI") == fused
        tpos = torch.tensor(pos, device=DEV).unsqueeze(0).requires_grad_(True)
        cell = torch.tensor(box, device=DEV).requires_grad_(True)
        energy = opt((numbers, tpos), cell, pbc).energies
        (3.0 * energy.sum()).backward()
        assert cell.grad is not None and cell.grad.shape == (3, 3) and bool(torch.isfinite(cell.grad).all())
        grads[fused] = (tpos.grad.clone(), cell.grad.clone())
        if fused:                                  # ... no cell gradient asked: none given; create_graph: refused
            tpos2 = torch.tensor(pos, device=DEV).unsqueeze(0).requires_grad_(True)
            cell2 = torch.tensor(box, device=DEV)
            opt((numbers, tpos2), cell2, pbc).energies.sum().backward()
            assert cell2.grad is None and torch.equal(tpos2.grad * 3.0, tpos.grad)
            cell3 = torch.tensor(box, device=DEV).requires_grad_(True)
            with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
                torch.autograd.grad(opt((numbers, tpos2), cell3, pbc).energies.sum(), [cell3], create_graph=True)
    top = float(grads[False][1].abs().max())
    err = float((grads[True][1] - grads[False][1]).abs().max())
    print(f"\n[ani-box] OptimizedTorchANI 300 atoms: fused vs composition cell gradient {err / top:.2e} of max {top:.3e}")
    assert top > 0 and err <= FORCE_RTOL * top, (err, top)
    ftop = float(grads[False][0].abs().max())
    assert float((grads[True][0] - grads[False][0]).abs().max()) <= FORCE_RTOL * ftop


def test_cell_gradient_replays_in_a_captured_graph(monkeypatch):
    """Forward + backward with a cell gradient captured once and replayed on new positions gives the eager result: the box pass
    allocates nothing (its partial sums belong to the handle)."""
    _clean_env(monkeypatch)
    pos, species, box = workloads.water_box(400, seed=7)               # 1 200 atoms
    module = _aev_module(species)
    sp = torch.tensor(species, device=DEV).unsqueeze(0)
    pbc = torch.tensor([True, True, True])                              # host pbc: .tolist() cannot be captured
    cell = torch.tensor(box, device=DEV).requires_grad_(True)
    static_pos = torch.tensor(pos, device=DEV).unsqueeze(0).requires_grad_(True)
    w = torch.randn((1, len(species), 1008), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))

    def step(p):
        aev = module((sp, p), cell, pbc)[1]
        return torch.autograd.grad((aev * w).sum(), [p, cell])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                              # calibrates neighbour capacities, warms allocators
            step(static_pos)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_pos, g_cell = step(static_pos)
    rng = np.random.default_rng(1)
    for _ in range(2):
        new = (pos + rng.normal(0, 0.05, pos.shape)).astype(np.float32)
        with torch.no_grad():
            static_pos.copy_(torch.tensor(new, device=DEV).unsqueeze(0))
        graph.replay()
        torch.cuda.synchronize()
        e_pos, e_cell = step(static_pos.detach().clone().requires_grad_(True))
        assert torch.equal(g_cell, e_cell) and torch.equal(g_pos, e_pos)
        assert float(e_cell.abs().max()) > 0
