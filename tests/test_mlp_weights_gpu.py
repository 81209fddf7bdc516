"""Weight gradients of the fused atomic networks (csrc/mlp_weight_grad.h) on the GPU against tests/mlp_weights_float64.py's float64
judge: through the C ABI (capi.FusedMLP.weight_grad) on every case of the judge's table, and through the torch surface
(torch.ops.NNPOpsBatchedNN.FusedMLPMembersTrainable behind TorchANIBatchedNN / OptimizedTorchANI with trainable=True).

The bar is G_BAR = 1e-4 of the largest entry of each of the eight arrays of each kind.  Every case of the table also asserts: a
second call gives the same bits, and `energies` and input_grad() are the same bits before and after weight_grad().  `pytest -s`
prints a line per case.
"""
import functools

import numpy as np
import pytest
import torch

import ani_members_float64 as AJ
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
    return all(torch.equal(ka[name], kb[name]) for ka, kb in zip(a, b) for name in W.NAMES)


@pytest.mark.parametrize("name", list(W.CASES))
def test_weight_grad_against_the_judge(name):
    fr = W.frame(name)
    mlp = _mlp(fr)
    x = fr.x.to(DEV).contiguous()
    w, offsets = _tables(fr)
    energies = mlp.forward(x, with_gradient=True).clone()
    dx = mlp.input_grad(x, member_weights=w, molecule_offsets=offsets).clone()
    got = mlp.weight_grad(member_weights=w, molecule_offsets=offsets)
    assert torch.equal(mlp.energies, energies)
    assert torch.equal(mlp.input_grad(x, member_weights=w, molecule_offsets=offsets), dx)
    assert _same_bits(mlp.weight_grad(member_weights=w, molecule_offsets=offsets), got)
    torch.cuda.synchronize()
    for kd, judged in zip(got, fr.judged):
        for g, a in W.ARRAY_OF.items():
            assert kd[g].shape == judged[a].shape and kd[g].dtype == torch.float32
    err, where = W.worst(got, fr.want)
    print(f"\n[mlp-weights] {name}: {err:.2e} of the largest entry at {where}", end="")
    assert err <= W.G_BAR, (err, where)
    if name == "zero-member":                       # the member nobody weighs is skipped: exact zeros, next to a member that is not
        for g in W.NAMES:
            assert not got[0][g][1].any() and got[0][g][0].any()
    if name == "eight-kinds":                       # kinds without atoms: exact zeros
        for k, count in enumerate(fr.case.counts):
            assert all(bool(got[k][g].any()) == (count > 0) for g in W.NAMES)


def test_a_frame_without_atoms_gives_zeros():
    fr = W.frame("eight-kinds")
    empty = [dict(kd, atoms=kd["atoms"][:0]) for kd in fr.kinds[:3]]
    mlp = _mlp(fr, kinds=empty)
    x = fr.x.to(DEV)
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    energies = torch.full((4, fr.case.M), -7.25, device=DEV)
    mlp.frame.rows, mlp.frame.energies = rows.data_ptr(), energies.data_ptr()      # (the C ABI asks for pointers, not for atoms)
    mlp.forward(x, with_gradient=True)
    for w in (None, torch.ones((1, fr.case.M), device=DEV)):
        got = mlp.weight_grad(member_weights=w)
        torch.cuda.synchronize()
        assert len(got) == 3 and all(not kd[g].any() for kd in got for g in W.NAMES)
    assert bool((energies == -7.25).all())


# ---------------------------------------------------------------------------------------------- the torch surface
def _numbers(species):
    return torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=DEV)


@functools.lru_cache(maxsize=None)
def build(trainable, n_atoms=23, members=3):
    from NNPOps import OptimizedTorchANI
    species, _ = AJ.molecule(n_atoms, 67)
    numbers = _numbers(species)
    module = OptimizedTorchANI(AJ.model_of(members), numbers.cpu(), trainable=trainable).to(DEV)
    assert type(module).__name__ == ("TrainableOptimizedTorchANI" if trainable else "FusedOptimizedTorchANI")
    return module, numbers


def _coords(n_atoms, picks):
    return torch.tensor(AJ.molecule(n_atoms, 67)[1][picks], device=DEV)


def _judge_of_model(module, numbers, coords, weights):
    """the judge's gradient for sum_m weights[m] E_m of ONE frame: over the float32 AEV the module's own AEV kernels give"""
    with torch.no_grad():
        aev = module.aev_computer((module.species_converter((numbers, coords)).species, coords))[1][0].cpu()
    want, _ = W.autograd(W.kinds_of_module(module.neural_networks[0]), aev, np.asarray(weights, dtype=np.float64))
    return want, aev


@pytest.mark.parametrize("what", ["forward", "members", "qbcs"])
def test_parameter_gradients_of_the_model(what):
    module, numbers = build(True)
    nets = module.neural_networks[0]
    coords = _coords(23, AJ.SLOTS[:1])
    module.zero_grad()
    M = nets.num_models
    if what == "forward":
        module((numbers, coords)).energies.sum().backward()
        weights = np.full(M, 1.0 / M)
    elif what == "members":
        weights = AJ.random_weights(1, M, seed=5)[0].astype(np.float64)
        E = module.members_energies((numbers, coords)).energies
        (E[:, 0] * torch.tensor(weights, device=DEV)).sum().backward()
    else:
        E = module.members_energies((numbers, coords)).energies.detach().requires_grad_(True)      # d qbcs / d E_m, from the energies themselves
        module._qbcs(numbers, E, True)[2].sum().backward()
        weights = E.grad[:, 0].cpu().numpy()
        module.energies_qbcs((numbers, coords))[2].sum().backward()
    want, aev = _judge_of_model(module, numbers, coords, weights)
    got = W.gradients_of_module(nets)
    err, where = W.worst(got, want)
    print(f"\n[mlp-weights] OptimizedTorchANI(trainable=True) {what}: {err:.2e} of the largest entry at {where}", end="")
    assert err <= W.G_BAR, (err, where)
    # columns of the AEV this molecule's species cannot fill, and everything outside a species' own widths: exact zeros
    dead = torch.nonzero(aev.abs().amax(0) == 0)[:, 0]
    assert nets.x_blocks.numel() > 0 and dead.numel() >= 1008 - 16 * nets.x_blocks.numel()
    assert not nets.layer0_weights.grad[:, :, :, dead.to(DEV)].any()
    for k in range(len(nets.group_sizes)):
        h1, h2, h3 = nets.widths[3 * k:3 * k + 3]
        assert not nets.layer0_weights.grad[k][:, h1:].any() and not nets.layer2_weights.grad[k][:, h2:].any()
        assert not nets.layer2_weights.grad[k][:, :, h1:].any() and not nets.layer6_weights.grad[k][:, :, h3:].any()


@pytest.mark.parametrize("batch", [1, 3])
def test_member_energies_and_coordinate_gradients_are_the_default_modules_bits(batch):
    trainable, numbers = build(True)
    default, _ = build(False)
    coords = _coords(23, AJ.SLOTS[:batch])
    w = torch.tensor(AJ.random_weights(batch, 3, seed=batch), device=DEV)
    out = []
    for module in (trainable, default):
        p = coords.clone().requires_grad_(True)
        if batch == 1:
            E = module.members_energies((numbers, p)).energies
        else:
            E = module.members_energies_batch((numbers.expand(batch, -1), p)).energies
        (E.t() * w).sum().backward()
        out.append((E.detach(), p.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("batch", [1, 3])
def test_energy_and_coordinate_gradient_are_the_default_modules_bits(batch):
    """forward / forward_batch: two autograd nodes against the default module's one, the same launches on the same numbers"""
    trainable, numbers = build(True)
    default, _ = build(False)
    coords = _coords(23, AJ.SLOTS[:batch])
    sp = numbers if batch == 1 else numbers.expand(batch, -1)
    out = []
    for module in (trainable, default):
        p = coords.clone().requires_grad_(True)
        e = (module((sp, p)) if batch == 1 else module.forward_batch((sp, p))).energies
        e.sum().backward()
        out.append((e.detach(), p.grad))
    assert out[0][0].shape == (batch,) and out[0][0].dtype == torch.float64 and float(out[0][1].abs().max()) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_the_networks_alone_are_the_default_modules_bits():
    """TorchANIBatchedNN(..., trainable=True) on an AEV of its own (no OptimizedTorchANI around it): energy and AEV gradient of forward
    and members_energies against the default module"""
    from NNPOps.BatchedNN import TorchANIBatchedNN
    species, _ = AJ.molecule(23, 67)
    model = AJ.model_of(3)
    numbers = _numbers(species)
    sp = torch.tensor(species[None].astype(np.int64), device=DEV)
    aev = (torch.rand((1, 23, 1008), generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV)
    out = []
    for flag in (True, False):
        nets = TorchANIBatchedNN(model.species_converter, model.neural_networks, numbers.cpu(), trainable=flag).to(DEV)
        x = aev.clone().requires_grad_(True)
        e = nets((sp, x)).energies
        (ge,) = torch.autograd.grad(e.sum(), x)
        m = nets.members_energies((sp, x)).energies
        (gm,) = torch.autograd.grad((m[:, 0] * torch.tensor([0.7, -0.2, 0.4], device=DEV)).sum(), x)
        out.append((e.detach(), ge, m.detach(), gm))
    assert all(torch.equal(a, b) for a, b in zip(*out)) and float(out[0][1].abs().max()) > 0


def test_three_sgd_steps_follow_the_float64_restatement():
    """12 atoms, 3 members, L = sum_m w_m E_m, lr = 1e-2, the AEV held fixed.  Bound per array: every step's gradient is within G_BAR of
    its largest entry gmax (the bar of this file); the two trajectories then differ by at most lr G_BAR gmax per step, and a
    gradient taken at parameters that far apart moves by a relative 1e-4 of that again -- doubled to have room for it: 3 lr 2 G_BAR
    gmax, plus the float32 rounding of the parameters themselves, 3 steps of 2^-24 |p|."""
    from NNPOps import OptimizedTorchANI
    species, confs = AJ.molecule(12, 67)
    numbers = _numbers(species)
    module = OptimizedTorchANI(AJ.model_of(3), numbers.cpu(), trainable=True).to(DEV)
    nets = module.neural_networks[0]
    coords = torch.tensor(confs[AJ.SLOTS[:1]], device=DEV)
    weights = np.array([0.7, -0.2, 0.4])
    lr = 1e-2
    opt = torch.optim.SGD(module.neural_networks.parameters(), lr=lr)
    with torch.no_grad():
        aev = module.aev_computer((module.species_converter((numbers, coords)).species, coords))[1][0].cpu()
    kinds = [{k: (v.double() if k != "atoms" else v) for k, v in kd.items()} for kd in W.kinds_of_module(nets)]
    start, first = W.kinds_of_module(nets), None
    for _ in range(3):
        opt.zero_grad()
        (module.members_energies((numbers, coords)).energies[:, 0] * torch.tensor(weights, device=DEV)).sum().backward()
        opt.step()
        grads, _ = W.autograd(kinds, aev, weights)
        first = first or grads
        for kd, g in zip(kinds, grads):
            for name, array in W.ARRAY_OF.items():
                kd[array] = kd[array] - lr * torch.as_tensor(g[name])
    after = W.kinds_of_module(nets)
    for k, (kd, ref) in enumerate(zip(after, kinds)):
        for name, array in W.ARRAY_OF.items():
            gmax = float(np.abs(first[k][name]).max())
            bound = 3 * lr * 2 * W.G_BAR * gmax + 3 * 2.0 ** -24 * float(ref[array].abs().max())
            err = float((kd[array].double() - ref[array]).abs().max())
            assert gmax > 0 and err <= bound, (k, name, err, bound)
            assert float((kd[array] - start[k][array]).abs().max()) > 0          # (and the parameters did move)


def test_planes_are_rebuilt_once_per_step_and_after_load_state_dict():
    from NNPOps import OptimizedTorchANI
    species, confs = AJ.molecule(12, 67)
    numbers = _numbers(species)
    module = OptimizedTorchANI(AJ.model_of(3), numbers.cpu(), trainable=True).to(DEV)
    nets = module.neural_networks[0]
    coords = torch.tensor(confs[AJ.SLOTS[:1]], device=DEV)
    opt = torch.optim.SGD(module.neural_networks.parameters(), lr=1e-3)
    module((numbers, coords))
    built = nets.plane_rebuilds
    for step in range(3):
        opt.zero_grad()
        module((numbers, coords)).energies.sum().backward()
        module.members_energies((numbers, coords))
        assert nets.plane_rebuilds == built + step                             # while the parameters stand, nothing is rebuilt
        opt.step()
        module((numbers, coords))
        assert nets.plane_rebuilds == built + step + 1                         # one rebuild per optimizer step
    state = {k: v.clone() for k, v in module.state_dict().items()}
    module.load_state_dict(state)
    assert nets.plane_rebuilds == built + 4
    e = module((numbers, coords)).energies
    module.energy_and_forces((numbers, coords))
    assert nets.plane_rebuilds == built + 4
    # the step outside autograd uses the current weights: its energy is the default arithmetic's on the trained parameters
    default = OptimizedTorchANI(AJ.model_of(3), numbers.cpu()).to(DEV)
    default.load_state_dict(state)
    assert torch.equal(module.energy_and_forces((numbers, coords))[0], default.energy_and_forces((numbers, coords))[0])
    assert float((e.detach() - default((numbers, coords)).energies.detach()).abs().max()) <= 1e-5


def test_second_derivatives_are_refused():
    module, numbers = build(True)
    coords = _coords(23, AJ.SLOTS[:1]).requires_grad_(True)
    E = module.members_energies((numbers, coords)).energies
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(E.sum(), [module.neural_networks[0].layer0_weights, coords], create_graph=True)
