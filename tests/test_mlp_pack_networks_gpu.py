"""The whole-ensemble pack of the fused networks on the device (csrc/mlp_pack_networks.h behind torch.ops.NNPOpsBatchedNN.PackNetworks
and _TrainableFusedNN._refresh_planes) against the library's host route, ``_FusedSpeciesNN._refresh_planes``: planes as int16, floats
as int32, bit for bit; the decisions taken from the status block against the host's; determinism, aliasing, the refusals, and three
optimizer steps of a model.

The thresholds of the activation scale lie a factor 2 apart (62 500 * 2^k, k = 4 .. 12), so a bound BETWEEN two of them is at most a
factor sqrt(2) from the nearer one: the cases for k = 8 and k = 12 sit in the geometric middle of their windows (1.41 from both ends;
asserted at 1.4 on the CPU with the host formula), the others at least 1.5 from their only neighbour.  The device forms its sums in
float64, the host in float32: they differ by parts in 1e6.
"""

import numpy as np
import pytest
import torch

import ani_members_float64 as AJ
import mlp_pack_cases as P
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _parameters(nets):
    from NNPOps.BatchedNN import PARAMETER_NAMES
    return [getattr(nets, name).detach() for name in PARAMETER_NAMES]


def _pack(nets):
    return torch.ops.NNPOpsBatchedNN.PackNetworks(_parameters(nets), nets.widths, nets.x_blocks if nets.live_blocks else None)


def _same(got, judge):
    return (torch.equal(P.bits(got[0]), P.bits(judge.mlp_planes)) and torch.equal(P.bits(got[1]), P.bits(judge.mlp_floats))
            and torch.equal(P.bits(got[2]), P.bits(judge.live_planes)))


# ---------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("name", list(P.CASES))
def test_planes_and_floats_are_the_host_routes_bits(name):
    judge = P.module(name, False, seed=3)
    with torch.no_grad():                                      # one value above fp16's range (hi = inf, lo = -inf on both routes)
        judge.layer2_weights[0, 0, 1, 2] = 1.0e5
        judge.layer0_weights[-1, -1, 3, 5] = -7.0e4
    judge._refresh_planes()                                    # the host route, on the CPU
    lo = judge.mlp_planes.view(-1, 2, 512)[:, 1]
    assert bool((lo != 0).any()) and bool(torch.isinf(judge.mlp_planes).any())           # both planes carry bits
    judge = judge.to(DEV)
    got = _pack(judge)
    assert got[0].dtype == torch.float16 and got[1].dtype == torch.float32 and got[3].dtype == torch.int32 and got[3].numel() == 44
    assert got[0].numel() == judge.mlp_planes.numel() and got[2].numel() == judge.live_planes.numel()
    assert _same(got, judge)
    # the ctypes entry writes the same, and a second call of either the same again
    from nnpops_amd import capi
    again = capi.FusedMLP.pack_networks(_parameters(judge), judge.widths, judge.x_blocks if judge.live_blocks else None)
    assert _same(again, judge) and torch.equal(got[3], again[3]) and torch.equal(P.bits(again[2]), P.bits(got[2]))
    once_more = _pack(judge)
    assert all(torch.equal(P.bits(a), P.bits(b)) for a, b in zip(got, once_more))


def test_the_host_route_on_the_device_writes_the_same_bits():
    """the judge of the other tests packs on the CPU; the same route over device tensors (what a rebuild was before) agrees with it"""
    judge = P.module("two-kinds", False, seed=3)
    planes, floats = judge.mlp_planes.clone(), judge.mlp_floats.clone()
    judge = judge.to(DEV)
    judge._refresh_planes()
    assert judge.mlp_planes.is_cuda and torch.equal(P.bits(judge.mlp_planes), P.bits(planes)) and torch.equal(P.bits(judge.mlp_floats), P.bits(floats))


# ---------------------------------------------------------------------------------------------- the status block
def test_status_block_against_float64():
    """last used rows exact; the maxima of single values exact; the abs-sums against numpy's float64 sums: up to 1024 terms in another
    order, 1024 * 2^-53 = 1.1e-13 of the sum, asserted at 1e-12"""
    nets = P.module("two-kinds", False, seed=5, wide=False).to(DEV)
    words = _pack(nets)[3].cpu()
    F, kinds, members, _ = P.CASES["two-kinds"]
    assert words[:24].tolist() == [h for kind in kinds for h in kind] + [0] * 18 and int(words[24]) == 0
    got = words[26:44].view(torch.float64).numpy()
    w = [getattr(nets, f"layer{l}_weights").double().cpu().numpy() for l in (0, 2, 4, 6)]
    b = [getattr(nets, f"layer{l}_biases").double().cpu().numpy() for l in (0, 2, 4)]
    want = [np.abs(w[0]).sum(-1).max(), np.abs(w[1]).sum(-1).max(), np.abs(w[2]).sum(-1).max(), np.abs(w[2]).sum(-2).max(), np.abs(w[1]).sum(-2).max(),
            np.abs(b[0]).max(), np.abs(b[1]).max(), np.abs(b[2]).max(), np.abs(w[3]).max()]
    assert np.all(got[5:] == want[5:]) and np.all(np.abs(got[:5] - want[:5]) <= 1e-12 * np.abs(want[:5])) and np.all(got > 0)


def _trained_pair(seed=5):
    """a trainable module on the device (its rebuilds pack there) and a default module that follows it through state dicts (host route)"""
    nets = P.module("two-kinds", True, seed=seed, wide=False).to(DEV)
    judge = P.module("two-kinds", False, seed=seed, wide=False).to(DEV)
    return nets, judge


STATUS_CASES = {                 # name -> (array, index, the bound it is to produce, expected act_scale_log2, expected fused_ok)
    "ordinary": (None, None, None, 4, True),
    "k8": ("layer4_biases", (1, 2, 5, 0), P.THRESHOLD * 2.0 ** 7.5, 8, True),               # through the forward bound
    "k12": ("layer6_weights", (0, 1, 0, 3), P.THRESHOLD * 2.0 ** 11.5, 12, True),           # through the backward bound
    "beyond": ("layer4_biases", (0, 0, 1, 0), P.THRESHOLD * 2.0 ** 14, 12, False),
}


@pytest.mark.parametrize("name", list(STATUS_CASES))
def test_decisions_are_the_host_routes(name):
    array, index, target, k, ok = STATUS_CASES[name]
    nets, judge = _trained_pair()
    with torch.no_grad():
        if array == "layer4_biases":
            getattr(nets, array)[index] = target
        elif array == "layer6_weights":                         # back = |w6| ||W4||_1 ||W2||_1: one entry carries the target
            _, back = P.host_bounds(nets)
            getattr(nets, array)[index] = target / (back / float(nets.layer6_weights.abs().max()))
    bound, back = P.host_bounds(nets)
    worst = max(bound, back)
    want_k, want_ok, margin = P.scale_of(worst)
    print(f"\n[mlp-pack] {name}: bound {bound:.4g}, back {back:.4g}, {margin:.3f} from the nearest threshold")
    assert (want_k, want_ok) == (k, ok) and margin >= (1.4 if name in ("k8", "k12") else 1.5)
    if target is not None:
        assert 0.99 <= worst / target <= 1.01                   # (the entry that was set carries the bound)
    packs = nets.device_packs
    nets._current_planes()
    judge.load_state_dict(nets.state_dict())
    assert nets.device_packs == packs + 1
    assert (nets.act_scale_log2, nets.fused_ok, nets.widths) == (judge.act_scale_log2, judge.fused_ok, judge.widths) == (k, ok, nets._fixed_widths)
    assert _same((nets.mlp_planes, nets.mlp_floats, nets.live_planes), judge)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("array", ["layer2_weights", "layer0_biases", "layer6_weights"])
def test_a_value_that_is_not_finite_turns_the_fused_kernels_off(array, value):
    nets, judge = _trained_pair()
    with torch.no_grad():
        getattr(nets, array)[1, 2, 0, 0] = value                # (row 0: a NaN hides its row from the width on both routes; the last row stands)
    nets._current_planes()
    judge.load_state_dict(nets.state_dict())
    assert not judge.fused_ok and judge.act_scale_log2 == 12
    assert (nets.act_scale_log2, nets.fused_ok, nets.widths) == (judge.act_scale_log2, judge.fused_ok, judge.widths)
    assert _same((nets.mlp_planes, nets.mlp_floats, nets.live_planes), judge)          # (int16 views: the NaNs compare)


# ---------------------------------------------------------------------------------------------- aliasing
def test_a_rebuild_leaves_the_previous_planes_alone():
    nets = P.module("ani2x-live3", True, seed=7, wide=False).to(DEV)
    nets._current_planes()                                      # (the move to the device: one rebuild, there)
    assert nets.device_packs == 1
    before = (nets.mlp_planes, nets.mlp_floats, nets.live_planes)
    kept = [t.clone() for t in before]
    with torch.no_grad():
        nets.layer0_weights.mul_(1.5)
        nets.layer4_biases.mul_(0.5)
    nets._current_planes()
    after = (nets.mlp_planes, nets.mlp_floats, nets.live_planes)
    assert nets.device_packs == 2
    for old, copy, new in zip(before, kept, after):
        assert new is not old and new.data_ptr() != old.data_ptr() and torch.equal(P.bits(old), P.bits(copy)) and not torch.equal(P.bits(new), P.bits(old))


# ---------------------------------------------------------------------------------------------- refusals
def _networks_of_a_molecule():
    from NNPOps.BatchedNN import TorchANIBatchedNN
    species, _ = AJ.molecule(23, 67)
    model = AJ.model_of(3)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]])
    nets = TorchANIBatchedNN(model.species_converter, model.neural_networks, numbers, trainable=True).to(DEV)
    aev = (torch.rand((1, 23, 1008), generator=torch.Generator().manual_seed(4)) * 0.5).to(DEV)
    return nets, (torch.tensor(species[None].astype(np.int64), device=DEV), aev)


def test_a_refused_structure_leaves_the_module_as_it_was_on_the_device():
    """tests/test_mlp_weights_reference_cpu.py::test_a_refused_structure_leaves_the_module_as_it_was with the module on the GPU"""
    nets, frame = _networks_of_a_molecule()
    nets(frame)
    planes, widths, built, packs = nets[0].mlp_planes, list(nets[0].widths), nets[0].plane_rebuilds, nets[0].device_packs
    kept = planes.clone()
    assert packs >= 1
    with torch.no_grad():
        nets[0].layer0_biases.add_(0.01)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="fixed at construction"):
            nets(frame)
    assert nets[0].mlp_planes is planes and torch.equal(P.bits(planes), P.bits(kept))
    assert nets[0].widths == widths and nets[0].plane_rebuilds == built and nets[0].device_packs == packs
    with torch.no_grad():
        nets[0].layer0_biases.sub_(0.01)
        nets[0].layer0_biases[nets[0].layer0_weights.abs().amax(3, keepdim=True) == 0] = 0.0
    nets(frame)
    assert nets[0].plane_rebuilds == built + 1 and nets[0].device_packs == packs + 1


def test_a_narrowed_structure_is_refused_on_the_device():
    nets, frame = _networks_of_a_molecule()
    nets(frame)
    planes, built, packs = nets[0].mlp_planes, nets[0].plane_rebuilds, nets[0].device_packs
    h2 = nets[0].widths[3 * 1 + 1]                              # the second layer of the second kind: its last 32 used rows go
    with torch.no_grad():
        saved = (nets[0].layer2_weights[1, :, h2 - 32:h2].clone(), nets[0].layer2_biases[1, :, h2 - 32:h2].clone())
        assert bool(saved[0].any())
        nets[0].layer2_weights[1, :, h2 - 32:h2] = 0.0
        nets[0].layer2_biases[1, :, h2 - 32:h2] = 0.0
    for _ in range(2):
        with pytest.raises(RuntimeError, match="fixed at construction"):
            nets(frame)
    assert nets[0].mlp_planes is planes and nets[0].plane_rebuilds == built and nets[0].device_packs == packs
    with torch.no_grad():
        nets[0].layer2_weights[1, :, h2 - 32:h2] = saved[0]
        nets[0].layer2_biases[1, :, h2 - 32:h2] = saved[1]
    nets(frame)
    assert nets[0].plane_rebuilds == built + 1 and nets[0].device_packs == packs + 1


# ---------------------------------------------------------------------------------------------- the model
def test_three_sgd_steps_of_a_model_rebuild_on_the_device():
    from NNPOps import OptimizedTorchANI
    from NNPOps.BatchedNN import _FusedSpeciesNN
    species, confs = AJ.molecule(12, 67)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=DEV)
    module = OptimizedTorchANI(AJ.model_of(3), numbers.cpu(), trainable=True)
    nets = module.neural_networks[0]
    assert nets.device_packs == 0 and nets.plane_rebuilds >= 1            # the constructor packs on the host
    built = nets.plane_rebuilds
    module = module.to(DEV)
    coords = torch.tensor(confs[AJ.SLOTS[:1]], device=DEV)
    module((numbers, coords))
    assert (nets.plane_rebuilds, nets.device_packs) == (built + 1, 1)     # .to(device): one rebuild, on the device
    judge = OptimizedTorchANI(AJ.model_of(3), numbers.cpu()).to(DEV).neural_networks[0]
    assert judge.live_blocks == nets.live_blocks and len(nets.live_blocks) > 0
    weights = torch.tensor([0.7, -0.2, 0.4], device=DEV)
    opt = torch.optim.SGD(module.neural_networks.parameters(), lr=1e-3)

    def outputs(model):
        p = coords.clone().requires_grad_(True)
        e = model((numbers, p)).energies
        m = model.members_energies((numbers, p)).energies
        grads = torch.autograd.grad(e.sum() + (m[:, 0] * weights).sum(), [p, *model.neural_networks.parameters()])
        return [e.detach(), m.detach(), *grads]

    for step in range(3):
        opt.zero_grad()
        module((numbers, coords)).energies.sum().backward()
        opt.step()
        got = outputs(module)
        assert (nets.plane_rebuilds, nets.device_packs) == (built + 2 + step, 2 + step)
        state = {k: v.clone() for k, v in module.state_dict().items()}
        judge.load_state_dict({k[len("neural_networks.0."):]: v for k, v in state.items() if k.startswith("neural_networks.0.")}, strict=False)
        assert _same((nets.mlp_planes, nets.mlp_floats, nets.live_planes), judge) and nets.live_planes.numel() > 0
        assert (nets.act_scale_log2, nets.fused_ok, nets.widths) == (judge.act_scale_log2, judge.fused_ok, judge.widths)
        fresh = OptimizedTorchANI(AJ.model_of(3), numbers.cpu(), trainable=True)
        fresh.load_state_dict({k: v.cpu() for k, v in state.items()})
        fresh = fresh.to(DEV)
        other = fresh.neural_networks[0]
        with torch.no_grad():
            _FusedSpeciesNN._refresh_planes(other)             # (on the device too it is to run on planes of the host route)
        other._plane_versions = other._versions()
        want = outputs(fresh)
        assert other.device_packs == 0
        assert len(got) == len(want) == 11 and all(torch.equal(a, b) for a, b in zip(got, want))
        assert all(float(g.abs().max()) > 0 for g in got[2:])
    module.load_state_dict(state)
    assert (nets.plane_rebuilds, nets.device_packs) == (built + 5, 5)      # load_state_dict: one rebuild, on the device
    module((numbers, coords))
    assert (nets.plane_rebuilds, nets.device_packs) == (built + 5, 5)
