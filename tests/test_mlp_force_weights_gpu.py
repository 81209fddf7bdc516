"""Weight gradients of the fused atomic networks under a force loss (csrc/mlp_weight_grad_tangent.h) on the GPU against
tests/mlp_force_weights_float64.py's float64 judge: through the C ABI (capi.FusedMLP.weight_grad_tangent) on every case of the judge's
table, and through the torch surface (torch.ops.NNPOpsBatchedNN.FusedMLPMembersForceTrainable / FusedMLPMeanForceTrainable behind
OptimizedTorchANI(..., force_trainable=True)).

The bar is G_BAR = 1e-4 of the largest entry of each of the eight arrays of each kind, and of the largest E'.  Every case of the table
also asserts: a second call gives the same bits, and `energies`, input_grad() and weight_grad() are the same bits before and after the
call.  Torch surface: the bits of trainable=True without create_graph, the bits of the plain backward under it, the parameter
gradients of (E - E0)^2 + sum (F - F0)^2 against float64 and against the grouped module, the force of the QBC factor, three SGD steps,
the launch counter, the plane-rebuild counter and every refusal by its message.  `pytest -s` prints a line per case.
"""
import functools

import numpy as np
import pytest
import torch

import ani_members_float64 as AJ
import mlp_force_weights_float64 as T
import mlp_weights_float64 as W
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _mlp(fr, kinds=None):
    from nnpops_amd.capi import FusedMLP
    c = fr.case
    kinds_dev = [{k: v.to(DEV) for k, v in kd.items()} for kd in (kinds or fr.kinds)]
    return FusedMLP(kinds_dev, c.x_width if c.live is not None else c.F, alpha=0.1, live_groups=c.live, act_scale_log2=c.k)


def _tables(fr):
    w = None if fr.weights is None else torch.tensor(fr.weights, device=DEV)
    offsets = None if fr.offsets is None else torch.tensor(fr.offsets, dtype=torch.int32, device=DEV)
    return w, offsets


def _same_bits(a, b):
    return all(torch.equal(ka[name], kb[name]) for ka, kb in zip(a, b) for name in T.NAMES)


@pytest.mark.parametrize("name", list(T.CASES))
def test_weight_grad_tangent_against_the_judge(name):
    fr = T.frame(name)
    mlp = _mlp(fr)
    x, t = fr.x.to(DEV).contiguous(), fr.t.to(DEV).contiguous()
    w, offsets = _tables(fr)
    energies = mlp.forward(x, with_gradient=True).clone()
    dx = mlp.input_grad(x, member_weights=w, molecule_offsets=offsets).clone()
    first_order = mlp.weight_grad(member_weights=w, molecule_offsets=offsets)
    got, edot = mlp.weight_grad_tangent(t, member_weights=w, molecule_offsets=offsets, tangent_energies=True)
    assert torch.equal(mlp.energies, energies)
    assert torch.equal(mlp.input_grad(x, member_weights=w, molecule_offsets=offsets), dx)
    assert _same_bits(mlp.weight_grad(member_weights=w, molecule_offsets=offsets), first_order)
    again, edot_again = mlp.weight_grad_tangent(t, member_weights=w, molecule_offsets=offsets, tangent_energies=True)
    assert _same_bits(again, got) and torch.equal(edot, edot_again)
    assert _same_bits(mlp.weight_grad_tangent(t, member_weights=w, molecule_offsets=offsets), got)      # (with or without E')
    torch.cuda.synchronize()
    for kd, judged in zip(got, fr.judged):
        for g, a in T.ARRAY_OF.items():
            assert kd[g].shape == judged[a].shape and kd[g].dtype == torch.float32
    err, where = T.worst(got, fr.want)
    err_e = T.worst_edot(edot, fr.edot)
    print(f"\n[mlp-force-weights] {name}: {err:.2e} of the largest entry at {where}, E' {err_e:.2e}", end="")
    assert err <= T.G_BAR, (err, where)
    assert err_e <= T.G_BAR, err_e
    assert all(not kd["db6"].any() for kd in got)     # E' does not depend on b6: exactly zero
    if name == "zero-member":                         # the member nobody weighs is skipped: exact zeros, next to a member that is not
        for g in T.NAMES[:-1]:
            assert not got[0][g][1].any() and got[0][g][0].any()
    if name == "two-kinds":                           # a kind without atoms: exact zeros
        for k, count in enumerate(fr.case.counts):
            assert all(bool(got[k][g].any()) == (count > 0) for g in T.NAMES[:-1])


def test_a_zero_tangent_gives_zeros():
    fr = T.frame("default")
    mlp = _mlp(fr)
    x = fr.x.to(DEV).contiguous()
    mlp.forward(x, with_gradient=True)
    got, edot = mlp.weight_grad_tangent(torch.zeros_like(x), tangent_energies=True)
    torch.cuda.synchronize()
    assert all(not kd[g].any() for kd in got for g in T.NAMES) and not edot.any()


def test_a_zero_weight_member_gives_zeros_whatever_its_planes_hold():
    fr = T.frame("zero-member")
    kinds = [dict(kd) for kd in fr.kinds]
    for name in ("w0", "b0", "w2", "b2", "w4", "b4", "w6", "b6"):
        poisoned = kinds[0][name].clone()
        poisoned[1] = float("nan")
        kinds[0][name] = poisoned
    mlp = _mlp(fr, kinds=kinds)
    x, t = fr.x.to(DEV).contiguous(), fr.t.to(DEV).contiguous()
    w, offsets = _tables(fr)
    mlp.forward(x, with_gradient=True)
    got = mlp.weight_grad_tangent(t, member_weights=w, molecule_offsets=offsets)
    torch.cuda.synchronize()
    for g in T.NAMES:
        assert not got[0][g][1].any() and bool(torch.isfinite(got[0][g]).all())
    want = [{g: fr.want[0][g][[0, 2]] for g in T.NAMES}]
    err, where = T.worst([{g: got[0][g][[0, 2]] for g in T.NAMES}], want)
    assert err <= T.G_BAR, (err, where)


def test_a_frame_without_atoms_gives_zeros():
    fr = T.frame("two-kinds")
    empty = [dict(kd, atoms=kd["atoms"][:0]) for kd in fr.kinds]
    mlp = _mlp(fr, kinds=empty)
    x, t = fr.x.to(DEV).contiguous(), fr.t.to(DEV).contiguous()
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    energies = torch.full((4, fr.case.M), -7.25, device=DEV)
    mlp.frame.rows, mlp.frame.energies = rows.data_ptr(), energies.data_ptr()      # (the C ABI asks for pointers, not for atoms)
    mlp.forward(x, with_gradient=True)
    for w in (None, torch.ones((1, fr.case.M), device=DEV)):
        got = mlp.weight_grad_tangent(t, member_weights=w)
        torch.cuda.synchronize()
        assert len(got) == 2 and all(not kd[g].any() for kd in got for g in T.NAMES)
    assert bool((energies == -7.25).all())


def test_bad_descriptors_are_refused():
    import ctypes as C
    from nnpops_amd import capi
    fr = T.frame("default")
    mlp = _mlp(fr)
    x, t = fr.x.to(DEV).contiguous(), fr.t.to(DEV).contiguous()
    mlp.forward(x, with_gradient=True)
    with pytest.raises(ValueError):
        mlp.weight_grad_tangent(t[:, :8].contiguous())
    out = capi._MlpWeightGradTangentOut()
    ws = torch.empty((64,), dtype=torch.float32, device=DEV)
    out.t, out.ldt, out.workspace, out.workspace_bytes = t.data_ptr(), t.shape[1], ws.data_ptr(), 256      # a workspace that is too small
    assert capi.lib().nnpops_mlp_weight_grad_tangent(None, C.byref(mlp.frame), C.byref(out)) == capi.lib().nnpops_mlp_weight_grad_tangent(
        None, None, C.byref(out)) != 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the torch surface
def _numbers(species):
    return torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=DEV)


def _module(species, flag="force_trainable", layout="fused", members=3):
    from NNPOps import OptimizedTorchANI
    numbers = _numbers(species)
    return OptimizedTorchANI(AJ.model_of(members), numbers.cpu(), nn_layout=layout, **{flag: True}).to(DEV), numbers


def _parameters(module):
    return list(module.neural_networks.parameters())


def _calls():
    return list(torch.ops.NNPOpsBatchedNN.WeightGradientCalls())


@functools.lru_cache(maxsize=None)
def _frames(case):
    if case == "water100":
        pos, species, box = workloads.water_box(100, seed=21)
        return species, pos[None], box
    species, confs = AJ.molecule(12 if case == "molecule12" else 23, 67)
    return species, confs[AJ.SLOTS[:3]] if case == "batch3" else confs[AJ.SLOTS[:1]], None


def _energies(module, numbers, x, cell, batch):
    if batch:
        return module.forward_batch((numbers.expand(x.shape[0], -1), x)).energies
    pbc = None if cell is None else torch.tensor([True, True, True], device=DEV)
    return module((numbers, x), cell, pbc).energies


def _device_loss(module, numbers, coords, cell, e0, f0, batch):
    """(E - E0)^2 + sum (F - F0)^2 through the module: F = -dE/dx with create_graph -> (loss, F)"""
    x = coords.clone().requires_grad_(True)
    energies = _energies(module, numbers, x, cell, batch)
    force = -torch.autograd.grad(energies.sum(), x, create_graph=True)[0]
    assert force.requires_grad, "the force carries no graph: the backward was not recorded"
    loss = ((energies - torch.tensor(e0, device=DEV)) ** 2).sum() + ((force - torch.tensor(f0, device=DEV, dtype=force.dtype)) ** 2).sum()
    return loss, force


def test_without_create_graph_everything_is_the_trainable_modules_bits():
    species, frames, _ = _frames("molecule23")
    out = []
    for flag in ("force_trainable", "trainable"):
        module, numbers = _module(species, flag)
        assert type(module).__name__ == ("ForceTrainableOptimizedTorchANI" if flag == "force_trainable" else "TrainableOptimizedTorchANI")
        x = torch.tensor(frames, device=DEV).requires_grad_(True)
        e = module((numbers, x)).energies
        e.sum().backward()
        m = module.members_energies((numbers, x)).energies
        w = torch.tensor([0.7, -0.2, 0.4], device=DEV, dtype=m.dtype)
        (m[:, 0] * w).sum().backward()
        xb = torch.tensor(_frames("batch3")[1], device=DEV).requires_grad_(True)
        eb = module.forward_batch((numbers.expand(3, -1), xb)).energies
        (eb * torch.tensor([1.0, -0.5, 2.0], device=DEV, dtype=eb.dtype)).sum().backward()
        out.append([e.detach(), m.detach(), eb.detach(), x.grad, xb.grad] + [p.grad for p in _parameters(module)])
    assert all(torch.equal(a, b) for a, b in zip(*out)) and all(float(a.abs().max()) > 0 for a in out[0])


def test_under_create_graph_the_force_is_the_plain_backwards_bits_and_no_weight_gradient_is_launched():
    species, frames, _ = _frames("molecule23")
    module, numbers = _module(species)
    x = torch.tensor(frames, device=DEV).requires_grad_(True)
    plain, = torch.autograd.grad(module((numbers, x)).energies.sum(), x)
    before = _calls()
    recorded, = torch.autograd.grad(module((numbers, x)).energies.sum(), x, create_graph=True)
    assert _calls() == before, "a force evaluation pays for no weight gradient"
    assert torch.equal(recorded, plain) and recorded.grad_fn is not None and plain.grad_fn is None
    (recorded ** 2).sum().backward(inputs=_parameters(module))
    assert _calls() == [before[0], before[1] + 1], "ONE call of the tangent weight gradient, no first-order one"
    def weighted():
        members = module.members_energies((numbers, x)).energies
        return (members[:, 0] * torch.tensor([0.7, -0.2, 0.4], device=DEV, dtype=members.dtype)).sum()

    plain, = torch.autograd.grad(weighted(), x)
    recorded, = torch.autograd.grad(weighted(), x, create_graph=True)
    assert torch.equal(recorded, plain) and recorded.grad_fn is not None


@functools.lru_cache(maxsize=None)
def _float64_of(case):
    species, frames, box = _frames(case)
    module, numbers = _module(species)
    want, e0, f0, loss64 = T.force_loss_float64(W.kinds_of_module(module.neural_networks[0], torch.float64), species, frames, box)
    return module, numbers, want, e0, f0, loss64


@pytest.mark.parametrize("case", ["molecule23", "batch3", "water100"])
def test_force_loss_parameter_gradients(case):
    species, frames, box = _frames(case)
    module, numbers, want, e0, f0, loss64 = _float64_of(case)
    nets = module.neural_networks[0]
    coords = torch.tensor(frames, device=DEV)
    cell = None if box is None else torch.tensor(box, device=DEV)
    batch = case == "batch3"
    module.zero_grad()
    loss, _ = _device_loss(module, numbers, coords, cell, e0, f0, batch)
    loss.backward(inputs=_parameters(module))
    got = W.gradients_of_module(nets)
    err, where = W.worst(got, want)
    # the grouped module, plain torch and twice differentiable, on the same parameters
    grouped, _ = _module(species, "trainable", "grouped")
    grouped.load_state_dict(module.state_dict())
    loss_g, _ = _device_loss(grouped, numbers, coords, cell, e0, f0, batch)
    loss_g.backward(inputs=_parameters(grouped))
    theirs = [{g: a.double().numpy() for g, a in kd.items()} for kd in W.gradients_of_module(grouped.neural_networks[0])]
    scale = [{g: float(np.abs(w[g]).max()) for g in W.NAMES} for w in want]
    err_g = max((float(np.abs(kd[g].double().numpy() - th[g]).max()) / sc[g] if sc[g] > 0 else 0.0)
                for kd, th, sc in zip(got, theirs, scale) for g in W.NAMES)
    print(f"\n[mlp-force-weights] force loss through OptimizedTorchANI(force_trainable) {case}: loss {float(loss.detach()):.6e} (float64 {loss64:.6e}), "
          f"parameter gradients {err:.2e} of the largest entry at {where}, {err_g:.2e} from the grouped module's", end="")
    assert err <= T.G_BAR, (err, where)
    assert err_g <= T.G_BAR, err_g
    # the same gradient by torch.autograd.grad
    loss2, _ = _device_loss(module, numbers, coords, cell, e0, f0, batch)
    params = _parameters(module)
    for p, g in zip(params, torch.autograd.grad(loss2, params, allow_unused=True)):
        assert torch.equal(p.grad, g if g is not None else torch.zeros_like(p))


def test_a_loss_of_forces_alone_trains():
    species, frames, _ = _frames("molecule23")
    module, numbers = _module(species)
    x = torch.tensor(frames, device=DEV).requires_grad_(True)
    force = -torch.autograd.grad(module((numbers, x)).energies.sum(), x, create_graph=True)[0]
    (force ** 2).sum().backward(inputs=_parameters(module))
    assert all(float(p.grad.abs().max()) > 0 for p in _parameters(module)[:7])
    assert not module.neural_networks[0].layer6_biases.grad.any()      # a force does not depend on the last bias


def test_the_force_of_the_qbc_factor_reaches_the_parameters():
    """the upstream weights of the member energies depend on the parameters: the recorded node's gradient in its upstream tensor"""
    species, frames, _ = _frames("molecule23")
    module, numbers = _module(species)
    nets = module.neural_networks[0]
    want, _, f0, _ = T.force_loss_float64(W.kinds_of_module(nets, torch.float64), species, frames, None, what="qbcs")
    x = torch.tensor(frames, device=DEV).requires_grad_(True)
    qbcs = module.energies_qbcs((numbers, x))[2]
    force = -torch.autograd.grad(qbcs.sum(), x, create_graph=True)[0]
    module.zero_grad()
    ((force - torch.tensor(f0, device=DEV, dtype=force.dtype)) ** 2).sum().backward(inputs=_parameters(module))
    err, where = W.worst(W.gradients_of_module(nets), want)
    print(f"\n[mlp-force-weights] force of the QBC factor: parameter gradients {err:.2e} of the largest entry at {where}", end="")
    assert err <= T.G_BAR, (err, where)


def test_three_sgd_steps_follow_the_float64_trajectory():
    """12 atoms, 3 members, the force loss, lr = 1e-3.  Bound per array, as in test_ani_tangent_gpu.py: every step's gradient is within
    G_BAR of its largest entry gmax; the trajectories then differ by at most lr G_BAR gmax per step, and a gradient taken at parameters
    that far apart moves by a relative 1e-4 of that again -- doubled to have room for it: 3 lr 2 G_BAR gmax, plus the float32 rounding
    of the parameters themselves, 3 steps of 2^-24 |p|."""
    species, frames, _ = _frames("molecule12")
    module, numbers = _module(species)
    nets = module.neural_networks[0]
    coords = torch.tensor(frames, device=DEV)
    lr = 1e-3
    kinds = W.kinds_of_module(nets, torch.float64)
    start = [{a: kd[a].clone() for a in W.ARRAY_OF.values()} for kd in kinds]
    _, e0, f0, _ = T.force_loss_float64(kinds, species, frames, None)
    gmax = [{a: 0.0 for a in W.ARRAY_OF.values()} for _ in kinds]
    opt = torch.optim.SGD(module.neural_networks.parameters(), lr=lr)
    module((numbers, coords))                              # (the planes of the parameters where they now lie)
    rebuilds = nets.plane_rebuilds
    for step in range(3):
        want, _, _, _ = T.force_loss_float64(kinds, species, frames, None, e0, f0)
        for k, kd in enumerate(kinds):
            for g, a in W.ARRAY_OF.items():
                gmax[k][a] = max(gmax[k][a], float(np.abs(want[k][g]).max()))
                kd[a] = kd[a] - lr * torch.as_tensor(want[k][g])
        opt.zero_grad()
        loss, _ = _device_loss(module, numbers, coords, None, e0, f0, False)
        loss.backward(inputs=_parameters(module))
        opt.step()
    now = W.kinds_of_module(nets, torch.float64)
    worst = 0.0
    for k, kd in enumerate(kinds):
        for a in W.ARRAY_OF.values():
            bound = 3 * lr * 2 * T.G_BAR * gmax[k][a] + 3 * 2.0 ** -24 * float(kd[a].abs().max())
            diff = float((now[k][a] - kd[a]).abs().max())
            worst = max(worst, diff / bound if bound > 0 else (0.0 if diff == 0 else np.inf))
            assert diff <= bound, (k, a, diff, bound)
            assert gmax[k][a] == 0 or float((kd[a] - start[k][a]).abs().max()) > 0
    print(f"\n[mlp-force-weights] three SGD steps on the force loss: largest deviation {worst:.2f} of its bound", end="")
    # the planes follow the parameters: one rebuild per optimizer step, none while they stand (the third step's is still due)
    assert nets.plane_rebuilds == rebuilds + 2
    _device_loss(module, numbers, coords, None, e0, f0, False)
    _device_loss(module, numbers, coords, None, e0, f0, False)
    assert nets.plane_rebuilds == rebuilds + 3


def test_refusals():
    species, frames, _ = _frames("molecule23")
    module, numbers = _module(species)
    params = _parameters(module)
    coords = torch.tensor(frames, device=DEV)

    def force_of(x):
        return -torch.autograd.grad(module((numbers, x)).energies.sum(), x, create_graph=True)[0]

    # loss.backward() without inputs= also differentiates in the positions
    x = coords.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="second derivatives with respect to the (positions|AEV) are not implemented.*inputs=parameters"):
        (force_of(x) ** 2).sum().backward()
    # the networks' Hessian in the AEV alone: the AEV as the leaf
    nets = module.neural_networks[0]
    aev = torch.ops.NNPOpsANISymmetryFunctions.aev(module.aev_computer.holder, coords[0], None).detach().requires_grad_(True)
    g, = torch.autograd.grad(nets.fused_mean(aev).sum(), aev, create_graph=True)
    with pytest.raises(RuntimeError, match="second derivatives with respect to the AEV are not implemented.*inputs=parameters"):
        (g ** 2).sum().backward()
    # a cotangent on a first-order weight gradient
    energy = nets.fused_mean(aev).sum()
    first = torch.autograd.grad(energy, params, create_graph=True, allow_unused=True)[0]
    with pytest.raises(RuntimeError, match="second derivatives with respect to the parameters are not implemented"):
        (first ** 2).sum().backward(inputs=params)
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


def test_cell_gradient_with_create_graph_is_refused():
    species, frames, box = _frames("water100")
    module, numbers = _module(species)
    x = torch.tensor(frames, device=DEV).requires_grad_(True)
    cell = torch.tensor(box, device=DEV).requires_grad_(True)
    energy = module((numbers, x), cell, torch.tensor([True, True, True], device=DEV)).energies.sum()
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(energy, [x, cell], create_graph=True)
