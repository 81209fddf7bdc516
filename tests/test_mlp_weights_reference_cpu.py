"""Weight gradients of the fused atomic networks without a GPU: the float64 judge of tests/mlp_weights_float64.py is pinned -- to the
closed form of the backward pass and to central differences of its own loss --, its float32 witness stays a tenth inside the bar on
every case the GPU file runs, the library and the binding have the new entries, and the trainable modules are checked where they are
plain torch: names, shapes, state dicts, gradients against the judge, and the refusals.
"""
import ctypes

import numpy as np
import pytest
import torch

import ani_members_float64 as AJ
import mlp_weights_float64 as W
from nnpops_amd import workloads


@pytest.mark.parametrize("name", ["default", "molecules", "eight-kinds", "saturated"])
def test_judge_is_the_closed_form(name):
    """float64 on both sides, but torch's float64 CELU' is not exp(z / alpha) to the last bit: at single points it is off by up to
    5e-9 relative (its backward forms the slope with a reciprocal of alpha that has float32's digits).  Three slopes multiply along
    the chain and the errors of a sum's terms do not cancel: a few 1e-8 at most.  Asserted at 1e-7 of each array's largest entry,
    three orders inside the bar the judge is used at."""
    f = W.frame(name)
    closed = W.closed_form(f.judged, f.x[:, f.columns].contiguous(), f.weights, f.offsets)
    err, where = W.worst(closed, f.want)
    print(f"\n[mlp-weights] {name}: closed form against autograd {err:.2e} at {where}")
    assert err <= 1e-7


def test_judge_against_central_differences():
    """float64, step h = 1e-5 on entries of the order of 0.1 .. 1: truncation h^2 L''' / 6 ~ 1e-10 of the gradient, rounding
    1e-16 |L| / h ~ 1e-9 with |L| ~ 1e2; asserted at 1e-6 of the array's largest entry, on four entries of every array"""
    f = W.frame("molecules")
    x = f.x[:, f.columns].contiguous()
    rng = np.random.default_rng(11)
    h = 1e-5
    for name in W.NAMES:
        array = W.ARRAY_OF[name]
        want = f.want[0][name]
        for _ in range(4):
            idx = tuple(int(rng.integers(0, s)) for s in want.shape)
            values = []
            for sign in (1.0, -1.0):
                kd = dict(f.judged[0])
                moved = kd[array].double().clone()
                moved[idx] += sign * h
                kd[array] = moved
                values.append(W.autograd([kd], x, f.weights, f.offsets)[1])
            numeric = (values[0] - values[1]) / (2 * h)
            assert abs(numeric - want[idx]) <= 1e-6 * np.abs(want).max(), (name, idx, numeric, want[idx])


@pytest.mark.parametrize("name", list(W.CASES))
def test_witness_is_a_tenth_inside_the_bar(name):
    err, where = W.worst(W.witness(name), W.frame(name).want)
    print(f"\n[mlp-weights] {name}: float32 witness {err:.2e} of the largest entry at {where}")
    assert err <= 0.1 * W.G_BAR


def test_zero_member_and_empty_kinds_are_zeros_in_the_judge():
    f = W.frame("zero-member")
    for name in W.NAMES:
        assert not f.want[0][name][1].any() and f.want[0][name][0].any()
    f = W.frame("eight-kinds")
    for k, count in enumerate(f.case.counts):
        assert all((not f.want[k][name].any()) == (count == 0) for name in W.NAMES)


def test_library_and_binding_have_the_new_entries():
    from nnpops_amd import build, capi, torch_binding
    handle = ctypes.CDLL(build.build())
    for name in ("nnpops_mlp_weight_grad", "nnpops_mlp_weight_grad_workspace_bytes"):
        assert hasattr(handle, name) and name in capi.SIGNATURES
    assert [f[0] for f in capi._MlpWeightGradKind._fields_] == list(W.NAMES)
    torch_binding.load()
    assert hasattr(torch.ops.NNPOpsBatchedNN, "FusedMLPMembersTrainable")
    schema = str(torch.ops.NNPOpsBatchedNN.FusedMLPMembersTrainable.default._schema)
    members = str(torch.ops.NNPOpsBatchedNN.FusedMLPMembers.default._schema)
    assert "Tensor[] parameters" in schema
    mean = str(torch.ops.NNPOpsBatchedNN.FusedMLPMeanTrainable.default._schema)           # the same node with the ensemble mean as its output
    assert "Tensor[] parameters" in mean and "bool total=False" in mean
    for word in ("x_blocks", "dead_blocks", "act_scale_log2", "offsets", "places", "shift"):
        assert word in schema and word in members
    # the workspace query without a device: per-atom data only, nothing for a frame without atoms but the members' flags
    frame = capi._MlpFrame()
    frame.num_kinds, frame.num_members = 1, 3
    frame.kinds[0].h1, frame.kinds[0].h2, frame.kinds[0].h3 = 96, 64, 32
    handle.nnpops_mlp_weight_grad_workspace_bytes.restype = ctypes.c_int64
    query = lambda n: (setattr(frame.kinds[0], "num_atoms", n), handle.nnpops_mlp_weight_grad_workspace_bytes(ctypes.byref(frame)))[1]
    per_tile = 4 * 3 * (2 * (96 + 64 + 32) + 1) * 64
    assert query(0) == 4 * 64 and query(1) == query(64) == 4 * 64 + per_tile and query(65) == 4 * 64 + 2 * per_tile


def _module(layout, trainable, members=3):
    from NNPOps.BatchedNN import TorchANIBatchedNN
    species, _ = AJ.molecule(23, 67)
    model = AJ.model_of(members)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]])
    return TorchANIBatchedNN(model.species_converter, model.neural_networks, numbers, layout=layout, trainable=trainable), species


def test_trainable_grouped_module_on_the_cpu():
    from NNPOps.BatchedNN import PARAMETER_NAMES
    nets, species = _module("grouped", True)
    default, _ = _module("grouped", False)
    assert [n for n, _ in nets.named_parameters()] == ["0." + n for n in PARAMETER_NAMES]
    assert list(default.parameters()) == []                                     # the default module keeps its buffers
    for name in PARAMETER_NAMES:
        assert getattr(nets[0], name).shape == getattr(default[0], name).shape and torch.equal(getattr(nets[0], name), getattr(default[0], name))
    assert sorted(nets.state_dict()) == sorted(default.state_dict())
    # state dicts interchange in both directions, and the reference's per-atom state dict still loads
    with torch.no_grad():
        nets[0].layer2_weights.mul_(1.5)
    default.load_state_dict(nets.state_dict())
    assert torch.equal(default[0].layer2_weights, nets[0].layer2_weights)
    fresh, _ = _module("grouped", True)
    fresh.load_state_dict(default.state_dict())
    assert torch.equal(fresh[0].layer2_weights, nets[0].layer2_weights) and isinstance(fresh[0].layer2_weights, torch.nn.Parameter)
    reference, _ = _module("reference", False)
    fresh.load_state_dict(reference.state_dict())
    restored, _ = _module("grouped", False)
    assert torch.equal(fresh[0].layer2_weights, restored[0].layer2_weights)
    # gradients of a weighted sum of the member energies against the judge (float32 plain torch: the witness's bar)
    nets, species = _module("grouped", True)
    aev = torch.rand((1, 23, 1008), generator=torch.Generator().manual_seed(3)) * 0.5
    sp = torch.tensor(species[None].astype(np.int64))
    w = torch.tensor([[0.7], [-0.2], [0.4]])
    (nets.members_energies((sp, aev)).energies * w).sum().backward()
    want, _ = W.autograd(W.kinds_of_module(nets[0]), aev[0], w[:, 0].numpy())
    err, where = W.worst(W.gradients_of_module(nets[0]), want)
    print(f"\n[mlp-weights] trainable grouped module on the CPU: {err:.2e} at {where}")
    assert err <= 0.1 * W.G_BAR
    # the structural padding has an exactly zero gradient: a species whose third layer is narrower than the widest one's
    widths = list(workloads.ANI2X_WIDTHS.values())
    padded = [(k, widths[s][2]) for k, s in enumerate(sorted(set(species.tolist()))) if widths[s][2] < nets[0].layer4_weights.shape[2]]
    assert padded
    for k, h3 in padded:
        assert not nets[0].layer4_weights.grad[k][:, h3:].any() and not nets[0].layer4_biases.grad[k][:, h3:].any()
        assert not nets[0].layer6_weights.grad[k][:, :, h3:].any() and nets[0].layer4_weights.grad[k][:, :h3].any()
    # and the mean's gradient is the members' with weights 1 / M
    nets.zero_grad()
    nets((sp, aev)).energies.sum().backward()
    want, _ = W.autograd(W.kinds_of_module(nets[0]), aev[0], np.full(3, 1.0 / 3.0))
    assert W.worst(W.gradients_of_module(nets[0]), want)[0] <= 0.1 * W.G_BAR


def test_trainable_fused_module_on_the_cpu_takes_plain_torch():
    """CPU tensors take the grouped path of the fused trainable module: parameters, their gradients, and the rebuild counter"""
    nets, species = _module("fused", True)
    default, _ = _module("fused", False)
    assert len(list(nets.parameters())) == 8 and list(default.parameters()) == []
    assert sorted(nets.state_dict()) == sorted(default.state_dict())
    built = nets[0].plane_rebuilds
    aev = torch.rand((1, 23, 1008), generator=torch.Generator().manual_seed(4)) * 0.5
    sp = torch.tensor(species[None].astype(np.int64))
    nets((sp, aev)).energies.sum().backward()
    assert nets[0].plane_rebuilds == built                                      # while the parameters stand, nothing is rebuilt
    want, _ = W.autograd(W.kinds_of_module(nets[0]), aev[0], np.full(3, 1.0 / 3.0))
    assert W.worst(W.gradients_of_module(nets[0]), want)[0] <= 0.1 * W.G_BAR
    with torch.no_grad():
        nets[0].layer0_biases.mul_(1.01)                                  # (a product: the zero padding stays zero)
    nets((sp, aev))
    nets((sp, aev))
    assert nets[0].plane_rebuilds == built + 1                                  # one rebuild after the edit, none after that
    nets.load_state_dict(default.state_dict())
    assert nets[0].plane_rebuilds == built + 2
    nets((sp, aev))
    assert nets[0].plane_rebuilds == built + 2


def test_a_refused_structure_leaves_the_module_as_it_was():
    """a value in the zero padding changes a species' packed width: the rebuild is refused before anything is replaced"""
    nets, species = _module("fused", True)
    aev = torch.rand((1, 23, 1008), generator=torch.Generator().manual_seed(4)) * 0.5
    sp = torch.tensor(species[None].astype(np.int64))
    planes, widths, built = nets[0].mlp_planes, list(nets[0].widths), nets[0].plane_rebuilds
    with torch.no_grad():
        nets[0].layer0_biases.add_(0.01)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="fixed at construction"):
            nets((sp, aev))
    assert nets[0].mlp_planes is planes and nets[0].widths == widths and nets[0].plane_rebuilds == built
    with torch.no_grad():
        nets[0].layer0_biases.sub_(0.01)
        nets[0].layer0_biases[nets[0].layer0_weights.abs().amax(3, keepdim=True) == 0] = 0.0      # (0.01 - 0.01 on a zero is a zero; to be sure)
    nets((sp, aev))
    assert nets[0].plane_rebuilds == built + 1


@pytest.mark.parametrize("layout", ["gemm", "reference"])
def test_layouts_without_a_weight_gradient_refuse(layout):
    with pytest.raises(ValueError, match="trainable"):
        _module(layout, True)
