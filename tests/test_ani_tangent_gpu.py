"""The tangent J.v of the ANI symmetry functions (nnpops_ani_tangent_strided) and the recorded backward of the torch ops above it.

C ABI.  The judge is tests/ani_tangent_float64.py's (float64 autograd over the restatement; pinned by
tests/test_ani_tangent_reference_cpu.py).  Bar: 1e-4 of the largest entry of the radial block and of the angular block -- the
project's force tolerance.  Properties: the adjoint identity <w, tangent(v)> = <backprop(w), v> on the device, to 1e-4 of the sum of
the absolute values of the terms; v = 0 and a rigid translation give zeros (the translation exactly in the radial block); a rigid
rotation of a vacuum frame gives zero to rounding -- below the bar times the largest entry of the tangent along a random field of the
same size, which is what the parts that cancel are made of; two calls give equal bits; compute() and backprop() around the call keep
theirs.

Torch surface.  torch.ops.NNPOpsANISymmetryFunctions.aev / operation under create_graph=True keep the bits of the plain backward, and
the parameter gradient of (E - E0)^2 + sum (F - F0)^2 through OptimizedTorchANI(nn_layout='grouped', trainable=True) is held against
float64 -- the restatement's AEV and mlp_weights_float64's networks, differentiated twice by autograd -- at 1e-4 of the largest entry
of each of the eight arrays of each kind.  What is out of scope is refused with a message.  Every case prints its figures (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import ani_members_float64 as AJ
import ani_tangent_float64 as T
import mlp_weights_float64 as W
from ani_float64 import Restatement, weights
from box_gradient_judge import clean_env
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = T.BAR


def _clean_env(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_ANI_")


@functools.lru_cache(maxsize=None)
def _reference(tag, fset="ani2x", torchani=True):
    """-> (restatement, v [N, 3] float32, (radial, angular) float64): once per case"""
    rest = T.restatement(tag, fset, torchani)
    _, _, _, species, pos, box = T.frame(tag)
    v = T.tangent_field(len(species), 5)
    return rest, v, T.judge(rest, pos, box, v)


def _handle(tag, fset="ani2x", torchani=True):
    from nnpops_amd.capi import AniSymmetryFunctions
    n_species, rcr, rca, species, _, box = T.frame(tag)
    return AniSymmetryFunctions(n_species, rcr, rca, species, *T.functions(fset), periodic=box is not None, torchani=torchani)


def _compute(sym, tag):
    _, _, _, _, pos, box = T.frame(tag)
    tpos = torch.tensor(pos, device=DEV)
    tbox = None if box is None else torch.tensor(box, device=DEV)
    return tpos, tbox, sym.compute(tpos, tbox)


def _numpy(pair):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().astype(np.float64) for t in pair)


def _check(label, got, ref):
    er, ea = T.block_errors(got, ref)
    print(f"\n[ani-tangent] {label}: radial {er:.2e} angular {ea:.2e} of the largest entry (bar {BAR:.0e})", end="")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert er <= BAR and ea <= BAR, (label, er, ea)


# ---------------------------------------------------------------------------------------------- the frames
SLOTS = dict(liquid600="32", liquid600_wrapped="32", dense900="64", slots128="128", slots256="256", liquid2100="32")      # record slots the frame is there for


@pytest.mark.parametrize("tag", T.FRAMES)
def test_tangent_against_float64(monkeypatch, tag):
    _clean_env(monkeypatch)
    rest, v, ref = _reference(tag)
    sym = _handle(tag)
    tpos, tbox, (radial, angular) = _compute(sym, tag)
    radial, angular = radial.clone(), angular.clone()
    wr, wa = (torch.tensor(w, device=DEV) for w in weights(ref[0].shape, ref[1].shape, seed=3))
    force = sym.backprop(wr, wa).clone()                # (dense900: this backprop stores its leg forces in the receivers' rows)
    what = sym.describe()
    assert what["cap_angular"] == SLOTS.get(tag, what["cap_angular"]) and what["cells"] == ("1" if tag == "liquid2100" else "0"), what
    if tag == "dense900":
        assert what["scatter"] == "1", what
    tv = torch.tensor(v, device=DEV)
    first = tuple(t.clone() for t in sym.tangent(tv))
    second = sym.tangent(tv)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), "two calls give different bits"
    # the calls around it keep their bits: backprop() on what the tangent left, then a fresh compute()
    assert torch.equal(sym.backprop(wr, wa), force), "backprop() after tangent() changed"
    again = sym.compute(tpos, tbox)
    assert torch.equal(again[0], radial) and torch.equal(again[1], angular), "compute() after tangent() changed"
    got = _numpy(first)
    _check(f"{tag} slots={what['cap_angular']} cells={what['cells']} scatter={what['scatter']}", got, ref)
    # the adjoint identity on the device
    left = float((wr.double() * first[0].double()).sum() + (wa.double() * first[1].double()).sum())
    right = float((force.double() * tv.double()).sum())
    size = float((wr * first[0]).abs().double().sum() + (wa * first[1]).abs().double().sum() + (force * tv).abs().double().sum())
    print(f"; <w, Jv> - <J^T w, v> = {abs(left - right) / size:.2e} of the terms", end="")
    assert abs(left - right) <= BAR * size, (left, right, size)


@pytest.mark.parametrize("tag", ["conformer60", "liquid600"])
def test_paper_angle_convention(monkeypatch, tag):
    _clean_env(monkeypatch)
    rest, v, ref = _reference(tag, "ani2x", False)
    sym = _handle(tag, "ani2x", False)
    _compute(sym, tag)
    _check(f"{tag} paper angles", _numpy(sym.tangent(torch.tensor(v, device=DEV))), ref)


@pytest.mark.parametrize("tag", ["one_atom", "two_atoms", "lone_angular"])
def test_smallest_frames(monkeypatch, tag):
    _clean_env(monkeypatch)
    rest, v, ref = _reference(tag)
    sym = _handle(tag)
    _compute(sym, tag)
    got = _numpy(sym.tangent(torch.tensor(v, device=DEV)))
    _check(tag, got, ref)
    assert not got[1].any(), "no atom of these frames has a triple"
    if tag == "one_atom":
        assert not got[0].any()


@pytest.mark.parametrize("tag", ["conformer60", "liquid600"])
def test_two_eta_two_zeta_padded_shape(monkeypatch, tag):
    """2 x 3 radial factors and 2 x 3 angle factors, each in a padded shape of 8: 36 angular functions, 4 radial ones"""
    _clean_env(monkeypatch)
    rest, v, ref = _reference(tag, "two_eta_two_zeta")
    sym = _handle(tag, "two_eta_two_zeta")
    _compute(sym, tag)
    assert sym.describe()["generic"] == "0"
    _check(f"{tag} two eta x two zeta", _numpy(sym.tangent(torch.tensor(v, device=DEV))), ref)


def test_list_that_does_not_factor(monkeypatch):
    """the generic kernels' lists (C ABI only) get their result: the tangent kernel evaluates every function as given"""
    _clean_env(monkeypatch)
    rest, v, ref = _reference("conformer60", "no_grid")
    sym = _handle("conformer60", "no_grid")
    _compute(sym, "conformer60")
    assert sym.describe()["generic"] == "1"
    _check("conformer60, 31 functions that are no grid", _numpy(sym.tangent(torch.tensor(v, device=DEV))), ref)


def test_batch_of_three_molecules(monkeypatch):
    from nnpops_amd.capi import AniSymmetryFunctions
    _clean_env(monkeypatch)
    species, pos, offsets = T.batch3()
    rf, af = workloads.ani2x_functions()
    v = T.tangent_field(len(species), 6)
    parts = []
    for lo, hi in zip(offsets[:-1], offsets[1:]):          # the judge: every molecule on its own
        parts.append(T.judge(Restatement(7, 5.1, 3.5, species[lo:hi], rf, af), pos[lo:hi], None, v[lo:hi]))
    ref = tuple(np.concatenate([p[k] for p in parts]) for k in range(2))
    sym = AniSymmetryFunctions(7, 5.1, 3.5, species, rf, af)
    sym.set_molecules(offsets)
    sym.compute(torch.tensor(pos, device=DEV))
    _check("three molecules (23, 9, 31 atoms) behind one handle", _numpy(sym.tangent(torch.tensor(v, device=DEV))), ref)


def test_strided_outputs_are_the_dense_bits(monkeypatch):
    _clean_env(monkeypatch)
    tag = "triclinic200"
    _, v, _ = _reference(tag)
    sym = _handle(tag)
    _compute(sym, tag)
    tv = torch.tensor(v, device=DEV)
    dense = tuple(t.clone() for t in sym.tangent(tv))
    wr, wa = sym.radial_width, sym.angular_width
    fused = torch.full((sym.num_atoms, wr + wa + 4), float("nan"), device=DEV)
    sym.tangent(tv, fused[:, :wr], fused[:, wr:wr + wa])
    assert torch.equal(fused[:, :wr], dense[0]) and torch.equal(fused[:, wr:wr + wa], dense[1])
    assert bool(torch.isnan(fused[:, wr + wa:]).all()), "the padding behind the rows was written"


def test_exact_cases(monkeypatch):
    _clean_env(monkeypatch)
    for tag in ("conformer60", "liquid600"):
        _, v, ref = _reference(tag)
        sym = _handle(tag)
        tpos, _, _ = _compute(sym, tag)
        n = sym.num_atoms
        zr, za = sym.tangent(torch.zeros((n, 3), device=DEV))
        assert not bool(zr.any()) and not bool(za.any()), "v = 0"
        shift = torch.tensor([0.3, -1.1, 0.7], device=DEV).repeat(n, 1)
        sr, sa = sym.tangent(shift)
        top_r, top_a = float(np.abs(ref[0]).max()), float(np.abs(ref[1]).max())
        print(f"\n[ani-tangent] {tag} rigid translation: radial {float(sr.abs().max()):.1e}, angular {float(sa.abs().max()) / top_a:.1e} of a random field's", end="")
        assert not bool(sr.any()), "a rigid translation moves no displacement: exactly zero in the radial block"
        assert float(sa.abs().max()) <= 1e-6 * top_a
        if tag == "conformer60":                            # a rigid rotation of a vacuum frame: v = omega x x, scaled to the random field's size
            omega = torch.tensor([0.4, -0.7, 0.5], device=DEV)
            rot = torch.linalg.cross(omega.expand(n, 3), tpos)
            rot = rot * (float(np.abs(v).max()) / float(rot.abs().max()))
            rr, ra = sym.tangent(rot)
            print(f"; rigid rotation: radial {float(rr.abs().max()) / top_r:.1e}, angular {float(ra.abs().max()) / top_a:.1e}", end="")
            assert float(rr.abs().max()) <= BAR * top_r and float(ra.abs().max()) <= BAR * top_a


def test_tangent_needs_a_compute(monkeypatch):
    from nnpops_amd.capi import NNPOpsHipError
    _clean_env(monkeypatch)
    sym = _handle("two_atoms")
    with pytest.raises(NNPOpsHipError, match="must follow compute"):
        sym.tangent(torch.zeros((2, 3), device=DEV))


# ---------------------------------------------------------------------------------------------- the torch surface
def _numbers(species):
    return torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=DEV)


def _module(species, layout="grouped", members=3):
    from NNPOps import OptimizedTorchANI
    numbers = _numbers(species)
    return OptimizedTorchANI(AJ.model_of(members), numbers.cpu(), nn_layout=layout, trainable=True).to(DEV), numbers


@pytest.mark.parametrize("op", ["aev", "operation"])
def test_recorded_backward_keeps_the_bits(monkeypatch, op):
    """create_graph=True with a cotangent that carries a graph: the force is the plain backward's, bit for bit, and it now has a
    graph of its own whose derivative in the cotangent is Holder.tangent"""
    from NNPOps.SymmetryFunctions import TorchANISymmetryFunctions
    _clean_env(monkeypatch)
    species, confs = AJ.molecule(23, 67)
    model = AJ.model_of(3)
    module = TorchANISymmetryFunctions(model.species_converter, model.aev_computer, _numbers(species).cpu()).to(DEV)
    pos = torch.tensor(confs[0], device=DEV).requires_grad_(True)
    gen = torch.Generator().manual_seed(4)
    cot = torch.randn((23, 1008), generator=gen).to(DEV).requires_grad_(True)
    v = torch.randn((23, 3), generator=gen).to(DEV)

    def outputs():
        out = getattr(torch.ops.NNPOpsANISymmetryFunctions, op)(module.holder, pos, None)
        return out if op == "aev" else torch.cat(list(out), dim=1)

    plain, = torch.autograd.grad((outputs() * cot.detach()).sum(), pos)
    assert plain.grad_fn is None
    count = module.holder.build_count()
    recorded, = torch.autograd.grad((outputs() * cot).sum(), pos, create_graph=True)
    assert module.holder.build_count() == count + 1
    assert torch.equal(recorded, plain) and recorded.grad_fn is not None
    tangent, = torch.autograd.grad((recorded * v).sum(), cot)
    assert torch.equal(tangent, module.holder.tangent(v))
    split = module.holder.tangent_split(v)
    assert torch.equal(torch.cat(list(split), dim=1), tangent)
    # without a graph behind the cotangent nothing is recorded, as before
    unrecorded, = torch.autograd.grad((outputs() * cot.detach()).sum(), pos, create_graph=True)
    assert torch.equal(unrecorded, plain) and not unrecorded.requires_grad


def _float64_gradients(nets, species, frames, box, e0, f0, kinds=None):
    """(E - E0)^2 + sum (F - F0)^2 summed over the frames [B][N][3], in float64: the restatement's AEV, the networks of the module as
    mlp_weights_float64 states them, F = -dE/dx by autograd with create_graph.  -> (gradient per kind, E [B], F [B][N][3], leaves)"""
    rf, af = workloads.ani2x_functions()
    rest = Restatement(7, 5.1, 3.5, species, rf, af, True)
    kinds = W.kinds_of_module(nets, torch.float64) if kinds is None else kinds
    leaves = [{name: kd[name].clone().requires_grad_(True) for name in W.ARRAY_OF.values()} for kd in kinds]
    members = leaves[0]["w0"].shape[0]
    box64 = np.asarray(T.VACUUM if box is None else box, dtype=np.float32).astype(np.float64).reshape(3, 3)
    loss, energies, forces = 0, [], []
    for b in range(len(frames)):
        pos64 = np.asarray(frames[b], dtype=np.float32).astype(np.float64)
        pairs, triples = rest.lists(pos64, box64)
        x, B = torch.tensor(pos64, requires_grad=True), torch.tensor(box64)
        radial = torch.zeros(rest.N * rest.S, rest.nR, dtype=torch.float64)
        angular = torch.zeros(rest.N * rest.NB, rest.nA, dtype=torch.float64)
        terms, rows = rest._radial_terms(x, B, pairs)
        radial = radial.index_add(0, rows, terms)
        if len(triples[0]):
            terms, rows = rest._angular_terms(x, B, triples)
            angular = angular.index_add(0, rows, terms)
        aev = torch.cat([radial.reshape(rest.N, -1), angular.reshape(rest.N, -1)], dim=1)
        energy = AJ.self_energy(species)
        for kd, p in zip(kinds, leaves):
            y = aev[kd["atoms"].long()].unsqueeze(0).expand(members, -1, -1)
            for w, bias in (("w0", "b0"), ("w2", "b2"), ("w4", "b4")):
                y = torch.nn.functional.celu(torch.baddbmm(p[bias].unsqueeze(1), y, p[w].transpose(1, 2)), alpha=0.1)
            energy = energy + (torch.einsum("mnh,mh->mn", y, p["w6"]) + p["b6"].unsqueeze(1)).sum() / members
        force = -torch.autograd.grad(energy, x, create_graph=True)[0]
        e0_b = float(energy.detach()) + 0.3 if e0 is None else e0[b]
        f0_b = force.detach() + 0.05 * torch.randn(force.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(70 + b)) \
            if f0 is None else torch.as_tensor(f0[b])
        loss = loss + (energy - e0_b) ** 2 + ((force - f0_b) ** 2).sum()
        energies.append(e0_b)
        forces.append(f0_b.numpy())
    flat = [p[name] for p in leaves for name in W.ARRAY_OF.values()]
    grads = torch.autograd.grad(loss, flat)
    it = iter(grads)
    out = [{g: next(it).numpy() for g in W.ARRAY_OF} for _ in leaves]
    return out, np.array(energies), np.stack(forces), float(loss.detach())


def _device_loss(module, numbers, coords, cell, e0, f0, batch):
    """the same loss through the module: E, F = -dE/dx with create_graph -> (loss, F)"""
    x = coords.clone().requires_grad_(True)
    if batch:
        energies = module.forward_batch((numbers.expand(x.shape[0], -1), x)).energies
    else:
        pbc = None if cell is None else torch.tensor([True, True, True], device=DEV)
        energies = module((numbers, x), cell, pbc).energies
    force = -torch.autograd.grad(energies.sum(), x, create_graph=True)[0]
    assert force.requires_grad, "the force carries no graph: the backward was not recorded"
    loss = ((energies - torch.tensor(e0, device=DEV)) ** 2).sum() + ((force - torch.tensor(f0, device=DEV, dtype=force.dtype)) ** 2).sum()
    return loss, force


FORCE_LOSS = ["molecule23", "batch3", "water100"]


@functools.lru_cache(maxsize=None)
def _force_loss_frame(case):
    if case == "water100":
        pos, species, box = workloads.water_box(100, seed=21)
        return species, pos[None], box
    species, confs = AJ.molecule(23, 67)
    return species, confs[AJ.SLOTS[:1]] if case == "molecule23" else confs[AJ.SLOTS[:3]], None


@pytest.mark.parametrize("case", FORCE_LOSS)
def test_force_loss_parameter_gradients(monkeypatch, case):
    _clean_env(monkeypatch)
    species, frames, box = _force_loss_frame(case)
    module, numbers = _module(species)
    nets = module.neural_networks[0]
    want, e0, f0, loss64 = _float64_gradients(nets, species, frames, box, None, None)
    coords = torch.tensor(frames, device=DEV)
    cell = None if box is None else torch.tensor(box, device=DEV)
    batch = case == "batch3"
    loss, _ = _device_loss(module, numbers, coords, cell, e0, f0 if batch else f0[:1], batch)
    loss.backward(inputs=list(module.neural_networks.parameters()))
    got = W.gradients_of_module(nets)
    err, where = W.worst(got, want)
    print(f"\n[ani-tangent] force loss through OptimizedTorchANI(grouped, trainable) {case}: loss {float(loss.detach()):.6e} (float64 {loss64:.6e}), "
          f"parameter gradients {err:.2e} of the largest entry at {where} (bar {BAR:.0e})", end="")
    assert err <= BAR, (err, where)
    # the same gradient by torch.autograd.grad, and the force term is in it: the energy term alone gives another one
    loss2, _ = _device_loss(module, numbers, coords, cell, e0, f0 if batch else f0[:1], batch)
    params = list(module.neural_networks.parameters())
    again = torch.autograd.grad(loss2, params, allow_unused=True)
    for p, g in zip(params, again):
        assert torch.equal(p.grad, g if g is not None else torch.zeros_like(p))


def test_a_loss_of_forces_alone_trains(monkeypatch):
    """what used to raise 'does not require grad'"""
    _clean_env(monkeypatch)
    species, frames, _ = _force_loss_frame("molecule23")
    module, numbers = _module(species)
    x = torch.tensor(frames, device=DEV).requires_grad_(True)
    force = -torch.autograd.grad(module((numbers, x)).energies.sum(), x, create_graph=True)[0]
    (force ** 2).sum().backward(inputs=list(module.neural_networks.parameters()))
    assert float(module.neural_networks[0].layer0_weights.grad.abs().max()) > 0


def test_three_sgd_steps_follow_the_float64_trajectory(monkeypatch):
    """12 atoms, 3 members, the force loss, lr = 1e-3.  Bound per array, as for the energy-only trajectory of test_mlp_weights_gpu.py:
    every step's gradient is within BAR of its largest entry gmax; the trajectories then differ by at most lr BAR gmax per step, and
    a gradient taken at parameters that far apart moves by a relative 1e-4 of that again -- doubled to have room for it:
    3 lr 2 BAR gmax, plus the float32 rounding of the parameters themselves, 3 steps of 2^-24 |p|."""
    _clean_env(monkeypatch)
    species, confs = AJ.molecule(12, 67)
    frames = confs[AJ.SLOTS[:1]]
    module, numbers = _module(species)
    nets = module.neural_networks[0]
    coords = torch.tensor(frames, device=DEV)
    lr = 1e-3
    kinds = W.kinds_of_module(nets, torch.float64)
    start = [{a: kd[a].clone() for a in W.ARRAY_OF.values()} for kd in kinds]
    _, e0, f0, _ = _float64_gradients(nets, species, frames, None, None, None, kinds)
    gmax = [{a: 0.0 for a in W.ARRAY_OF.values()} for _ in kinds]
    opt = torch.optim.SGD(module.neural_networks.parameters(), lr=lr)
    for step in range(3):
        want, _, _, _ = _float64_gradients(nets, species, frames, None, e0, f0, kinds)
        for k, kd in enumerate(kinds):
            for g, a in W.ARRAY_OF.items():
                gmax[k][a] = max(gmax[k][a], float(np.abs(want[k][g]).max()))
                kd[a] = kd[a] - lr * torch.as_tensor(want[k][g])
        opt.zero_grad()
        loss, _ = _device_loss(module, numbers, coords, None, e0, f0, False)
        loss.backward(inputs=list(module.neural_networks.parameters()))
        opt.step()
    now = W.kinds_of_module(nets, torch.float64)
    worst = 0.0
    for k, kd in enumerate(kinds):
        for a in W.ARRAY_OF.values():
            bound = 3 * lr * 2 * BAR * gmax[k][a] + 3 * 2.0 ** -24 * float(kd[a].abs().max())
            diff = float((now[k][a] - kd[a]).abs().max())
            worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else np.inf))
            assert diff <= bound, (k, a, diff, bound)
            assert gmax[k][a] == 0 or float((kd[a] - start[k][a]).abs().max()) > 0
    print(f"\n[ani-tangent] three SGD steps on the force loss: largest deviation {worst:.2f} of its bound", end="")


def test_refusals(monkeypatch):
    _clean_env(monkeypatch)
    species, frames, _ = _force_loss_frame("molecule23")
    module, numbers = _module(species)
    params = list(module.neural_networks.parameters())
    coords = torch.tensor(frames, device=DEV)

    def force_of(x):
        return -torch.autograd.grad(module((numbers, x)).energies.sum(), x, create_graph=True)[0]

    # loss.backward() without inputs= also differentiates in the positions: second derivatives of the AEV
    x = coords.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="second derivatives with respect to the positions are not implemented.*inputs=parameters"):
        (force_of(x) ** 2).sum().backward()
    x = coords.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="second derivatives with respect to the positions are not implemented"):
        torch.autograd.grad((force_of(x) ** 2).sum(), x)
    # a third derivative
    x = coords.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="third derivatives are not implemented"):
        torch.autograd.grad((force_of(x) ** 2).sum(), params, create_graph=True)
    # a forward on the same holder between the forward and the double backward
    x = coords.clone().requires_grad_(True)
    loss = (force_of(x) ** 2).sum()
    module((numbers, coords))
    with pytest.raises(RuntimeError, match="another forward pass"):
        loss.backward(inputs=params)
    # ... and between the forward and the recorded backward itself
    x = coords.clone().requires_grad_(True)
    energy = module((numbers, x)).energies.sum()
    module((numbers, coords))
    with pytest.raises(RuntimeError, match="another forward pass"):
        torch.autograd.grad(energy, x, create_graph=True)


def test_cell_gradient_with_create_graph_is_still_refused(monkeypatch):
    _clean_env(monkeypatch)
    pos, species, box = workloads.water_box(100, seed=21)
    module, numbers = _module(species)
    x = torch.tensor(pos[None], device=DEV).requires_grad_(True)
    cell = torch.tensor(box, device=DEV).requires_grad_(True)
    energy = module((numbers, x), cell, torch.tensor([True, True, True], device=DEV)).energies.sum()
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(energy, [x, cell], create_graph=True)


def test_fused_layout_still_trains_on_energies_only(monkeypatch):
    _clean_env(monkeypatch)
    species, frames, _ = _force_loss_frame("molecule23")
    module, numbers = _module(species, layout="fused")
    assert type(module).__name__ == "TrainableOptimizedTorchANI"
    x = torch.tensor(frames, device=DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(module((numbers, x)).energies.sum(), x, create_graph=True)
