"""Per-member energies of an ANI ensemble without a GPU: the float64 judge of tests/ani_members_float64.py is pinned -- its mean to
the formula of the mean's judge, its sigma-gradient to central differences of its own sigma --, the plain-torch path of
TorchANIBatchedNN.members_energies is checked against the networks one by one, and the library and the binding have the new entries.
"""
import ctypes

import numpy as np
import pytest
import torch

import ani_members_float64 as J
from nnpops_amd import workloads
from oracle import AniOracle, AniOracle64


def test_judge_mean_is_the_mean_judge_formula():
    """the formula of judge() in test_ani_batch_energy_gpu.py: the sum over members and species of the networks' outputs, divided by
    the number of members, plus the self energy; its gradient through one oracle.backward of the mean's AEV gradient"""
    species, confs = J.molecule(23, 67)
    model = J.model_of(3)
    E, G = J.judge(23, 67, "HCNO", 3, tuple(J.SLOTS[:2]))
    oracle = AniOracle(7, 5.1, 3.5, species, *workloads.ani2x_functions(), periodic=False)
    nets = [{sym: net.double() for sym, net in member.items()} for member in model.neural_networks]
    try:
        for b, slot in enumerate(J.SLOTS[:2]):
            r_ref, a_ref = oracle.forward(confs[slot])
            aev = torch.tensor(np.concatenate([r_ref, a_ref], axis=1), dtype=torch.float64, requires_grad=True)
            total = 0
            for member in nets:
                for s in sorted(set(species.tolist())):
                    total = total + member[J.SYMS[s]](aev[torch.tensor(np.nonzero(species == s)[0])]).sum()
            e = total / len(nets)
            e.backward()
            g = aev.grad.float().numpy()
            grad = oracle.backward(np.ascontiguousarray(g[:, :112]), np.ascontiguousarray(g[:, 112:]))
            assert abs(E[b].mean() - float(e.detach())) <= 1e-12 * max(1.0, abs(float(e.detach())))
            # (float32 AEV gradients through a float32 backward on both sides: the mean of three roundings against one rounding of the mean)
            assert np.abs(G[b].mean(axis=0) - grad).max() <= 1e-5 * np.abs(grad).max()
    finally:
        for member in model.neural_networks:
            member.float()
    assert E.shape == (2, 3) and G.shape == (2, 3, 23, 3)
    assert E.min() > -1.5 and E.max() < 4.5 and 1.5 < J.sigma(E).min() and J.sigma(E).max() < 1.9      # (the figures of the inputs' survey)


@pytest.mark.parametrize("unbiased", [True, False])
def test_judge_sigma_gradient_against_central_differences(unbiased):
    """float64 throughout (AniOracle64), step 1e-4 A.  The oracle takes float32 positions, so the step actually taken is the
    difference of the two rounded positions.  Bound: truncation h^2 f''' / 6 with h = 1e-4 and third derivatives of sigma of the order
    of 1e2 of its first (Gaussians of width ~0.25 A: (1 / 0.25)^2 = 16 per derivative) is 1e-6 relative, rounding 1e-16 sigma / h =
    1e-12; asserted at 1e-5 of the largest entry."""
    species, confs = J.molecule(23, 67)
    model = J.model_of(3)
    pos = confs[J.SLOTS[0]]
    E, G = J.judge_frames(species, [pos], model, oracle_cls=AniOracle64)
    analytic = J.combine(J.sigma_weights(E[0], unbiased), G[0])
    frames, steps = [], []
    for a in range(23):
        for c in range(3):
            plus, minus = pos.copy(), pos.copy()
            plus[a, c] = np.float32(pos[a, c] + 1e-4)
            minus[a, c] = np.float32(pos[a, c] - 1e-4)
            frames += [plus, minus]
            steps.append(float(plus[a, c]) - float(minus[a, c]))
    Es, _ = J.judge_frames(species, frames, model, oracle_cls=AniOracle64, gradients=False)
    s = J.sigma(Es, unbiased)
    numeric = ((s[0::2] - s[1::2]) / np.array(steps)).reshape(23, 3)
    err = np.abs(numeric - analytic).max() / np.abs(analytic).max()
    print(f"\n[ani-members] sigma-gradient (unbiased={unbiased}) against central differences: {err:.2e} of the largest entry")
    assert err <= 1e-5
    # the float32-oracle judge the GPU tests use agrees with the float64 one far inside their bars
    E32, G32 = J.judge(23, 67, "HCNO", 3, tuple(J.SLOTS[:2]))
    assert np.abs(E32[0] - E[0]).max() <= 1e-5 and np.abs(G32[0] - G[0]).max() <= 1e-5 * np.abs(G[0]).max()


@pytest.mark.parametrize("layout", ["grouped", "reference"])
def test_plain_members_energies_on_cpu(layout):
    from NNPOps.BatchedNN import TorchANIBatchedNN
    species, _ = J.molecule(23, 67)
    model = J.model_of(3)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]])
    nets = TorchANIBatchedNN(model.species_converter, model.neural_networks, numbers, layout=layout)
    aev = torch.rand((1, 23, 1008), generator=torch.Generator().manual_seed(3)) * 0.5
    aev.requires_grad_(True)
    sp = torch.tensor(species[None].astype(np.int64))
    out = nets.members_energies((sp, aev))
    assert out.energies.shape == (3, 1) and out.energies.dtype == torch.float32 and torch.equal(out.species, sp)
    nets64 = [{sym: net.double() for sym, net in member.items()} for member in model.neural_networks]
    try:
        want = J.member_energies(nets64, species, aev[0].detach().double()).detach()
    finally:
        for member in model.neural_networks:
            member.float()
    assert float((out.energies[:, 0].detach().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    mean = nets((sp, aev)).energies
    assert float((out.energies.mean(0) - mean).detach().abs().max()) <= 1e-5 * float(mean.detach().abs().max())
    # plain torch: twice differentiable
    w = torch.tensor([[0.7], [-0.2], [0.4]])
    (first,) = torch.autograd.grad((out.energies * w).sum(), aev, create_graph=True)
    assert first.requires_grad and first.shape == aev.shape
    (second,) = torch.autograd.grad(first.square().sum(), aev)
    assert bool(torch.isfinite(second).all()) and float(second.abs().max()) > 0
    # several molecules at once keep TorchANI's shape [models, molecules]
    two = nets.members_energies((sp.expand(2, -1), torch.cat([aev, 0.5 * aev]).detach())).energies
    assert two.shape == (3, 2) and torch.allclose(two[:, 0], out.energies[:, 0].detach(), rtol=1e-5, atol=1e-6)


def test_library_and_binding_have_the_new_entries():
    from nnpops_amd import build, capi, torch_binding
    handle = ctypes.CDLL(build.build())
    for name in ("nnpops_mlp_member_sums", "nnpops_mlp_member_sums_shifted"):
        assert hasattr(handle, name) and name in capi.SIGNATURES
    fields = [f[0] for f in capi._MlpFrame._fields_]
    assert fields[-2:] == ["member_weights", "member_weights_ld"]            # appended: every earlier field keeps its place
    torch_binding.load()
    assert hasattr(torch.ops.NNPOpsBatchedNN, "FusedMLPMembers")
    schema = str(torch.ops.NNPOpsBatchedNN.FusedMLPMembers.default._schema)
    for word in ("x_blocks", "dead_blocks", "act_scale_log2=4", "offsets", "places", "shift"):
        assert word in schema, schema
