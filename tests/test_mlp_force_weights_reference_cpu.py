"""Weight gradients of the fused atomic networks under a force loss, without a GPU: the float64 judge of
tests/mlp_force_weights_float64.py is pinned -- to the closed form of the reverse pass over the joint (z, z') graph, to central
differences of M in every array and of E along t --, its float32 witness stays inside half the bar on every case the GPU file runs,
no case of the table has a unit on the kink of CELU'', the library and the binding have the new entries, and the force_trainable
modules are checked where they are plain Python: the flags' errors, names, state dicts.
"""
import ctypes

import numpy as np
import pytest
import torch

import ani_members_float64 as AJ
import mlp_force_weights_float64 as T
from nnpops_amd import workloads


@pytest.mark.parametrize("name", ["default", "molecules", "two-kinds", "saturated", "live", "t-large"])
def test_judge_is_the_closed_form(name):
    """float64 on both sides; torch's float64 CELU' and CELU'' are not exp(z / alpha) to the last bit (mlp_weights_float64's note: up to
    5e-9 relative at single points), and here four such factors multiply along the chain: asserted at 1e-7 of each array's largest
    entry, three orders inside the bar the judge is used at."""
    f = T.frame(name)
    closed = T.closed_form(f.judged, f.x[:, f.columns].contiguous(), T.tangent_of(f), f.weights, f.offsets)
    err, where = T.worst(closed, f.want)
    print(f"\n[mlp-force-weights] {name}: closed form against autograd {err:.2e} at {where}")
    assert err <= 1e-7
    assert T.worst_edot(T.tangent_energy(f.judged, f.x[:, f.columns].contiguous(), T.tangent_of(f)), f.edot) <= 1e-7


def test_judge_against_central_differences():
    """float64, step h = 1e-6 on entries of the order of 0.1 .. 1, M computed by the forward tangent alone (no autograd): the step moves a
    pre-activation by at most h (|x|_1 or |y|_1) ~ 1e-4 only for the first layer's biggest rows -- so the entries are taken from a case
    whose smallest |z| is known, and a step that crosses the kink would show as an error of the order of the gradient itself.  Truncation
    h^2 M''' / 6 ~ 1e-12, rounding 1e-16 |M| / h ~ 1e-9; asserted at 1e-6 of the array's largest entry, on four entries of every array."""
    f = T.frame("molecules")
    x, t = f.x[:, f.columns].contiguous(), T.tangent_of(f)
    c = T.W.atom_weights(f.judged, f.weights, f.offsets)[0]                     # [M][n]
    rng = np.random.default_rng(12)
    h = 1e-6
    assert T.kink_margin("molecules")[0] > 10 * h * float(x.abs().max())        # (a weight moves z by h |x_j| <= h max |x|: far from the kink)
    for name in T.NAMES:
        array = T.ARRAY_OF[name]
        want = f.want[0][name]
        for _ in range(4):
            idx = tuple(int(rng.integers(0, s)) for s in want.shape)
            values = []
            for sign in (1.0, -1.0):
                kd = dict(f.judged[0])
                moved = kd[array].double().clone()
                moved[idx] += sign * h
                kd[array] = moved
                values.append(float((T.tangent_energy([kd], x, t).T * c).sum()))
            numeric = (values[0] - values[1]) / (2 * h)
            assert abs(numeric - want[idx]) <= 1e-6 * max(np.abs(want).max(), 1e-30), (name, idx, numeric, want[idx])


def test_tangent_energies_against_central_differences_of_the_energy():
    """E' = dE(x + s t)/ds at s = 0: central differences with s = 1e-6 (|t| ~ 1: x moves by 1e-6, z by ~1e-6 |w|_1 -- inside the margin
    of the table), asserted at 1e-6 of the largest E'"""
    for name in ("default", "two-kinds", "saturated"):
        f = T.frame(name)
        x, t = f.x[:, f.columns].contiguous().double(), T.tangent_of(f).double()
        s = 1e-6
        numeric = (T.energy(f.judged, x + s * t) - T.energy(f.judged, x - s * t)) / (2 * s)
        assert np.abs(numeric - f.edot).max() <= 1e-6 * np.abs(f.edot).max(), name


@pytest.mark.parametrize("name", list(T.CASES))
def test_witness_is_inside_half_the_bar(name):
    f = T.frame(name)
    got, edot = T.witness(name)
    err, where = T.worst(got, f.want)
    err_e = T.worst_edot(edot, f.edot)
    print(f"\n[mlp-force-weights] {name}: float32 witness {err:.2e} of the largest entry at {where}, E' {err_e:.2e}")
    assert err <= 0.5 * T.G_BAR and err_e <= 0.5 * T.G_BAR


def test_no_unit_of_the_table_sits_on_the_kink():
    """tau = 16 x the largest |z_witness - z_float64| over the table; every case's smallest |z| is above it"""
    margins = {name: T.kink_margin(name) for name in T.CASES}
    tau = T.KINK_FACTOR * max(d for _, d in margins.values())
    closest = min(margins, key=lambda name: margins[name][0])
    print(f"\n[mlp-force-weights] tau = {tau:.2e}; the smallest |z| of the table is {margins[closest][0]:.2e} ({closest})")
    for name, (zmin, _) in margins.items():
        assert zmin >= tau, (name, zmin, tau)


def test_zero_member_and_the_empty_kind_are_zeros_in_the_judge():
    f = T.frame("zero-member")
    for name in T.NAMES:
        assert not f.want[0][name][1].any()
    f = T.frame("two-kinds")
    assert all(not f.want[0][name].any() for name in T.NAMES) and f.want[1]["dw0"].any()
    assert all(not kd["db6"].any() for name in T.CASES for kd in T.frame(name).want)


def test_library_and_binding_have_the_new_entries():
    from nnpops_amd import build, capi, torch_binding
    handle = ctypes.CDLL(build.build())
    for name in ("nnpops_mlp_weight_grad_tangent", "nnpops_mlp_weight_grad_tangent_workspace_bytes"):
        assert hasattr(handle, name) and name in capi.SIGNATURES
    assert hasattr(capi.FusedMLP, "weight_grad_tangent")
    assert [f[0] for f in capi._MlpWeightGradTangentOut._fields_] == ["t", "ldt", "workspace", "workspace_bytes", "tangent_energies", "kinds"]
    torch_binding.load()
    for op, like in (("FusedMLPMembersForceTrainable", "FusedMLPMembersTrainable"), ("FusedMLPMeanForceTrainable", "FusedMLPMeanTrainable")):
        assert hasattr(torch.ops.NNPOpsBatchedNN, op)
        schema = str(getattr(torch.ops.NNPOpsBatchedNN, op).default._schema)
        assert schema.replace(op, like) == str(getattr(torch.ops.NNPOpsBatchedNN, like).default._schema)
    # the workspace query without a device: per-atom data only, atoms rounded up to the tile pass's 32
    frame = capi._MlpFrame()
    frame.num_kinds, frame.num_members = 1, 3
    frame.kinds[0].h1, frame.kinds[0].h2, frame.kinds[0].h3 = 96, 64, 32
    handle.nnpops_mlp_weight_grad_tangent_workspace_bytes.restype = ctypes.c_int64
    query = lambda n: (setattr(frame.kinds[0], "num_atoms", n), handle.nnpops_mlp_weight_grad_tangent_workspace_bytes(ctypes.byref(frame)))[1]
    per_tile = 4 * 3 * (4 * 96 + 4 * 64 + 3 * 32) * 32
    assert query(0) == 4 * 64 and query(1) == query(32) == 4 * 64 + per_tile and query(33) == 4 * 64 + 2 * per_tile


def _module(layout, **flags):
    from NNPOps.BatchedNN import TorchANIBatchedNN
    species, _ = AJ.molecule(23, 67)
    model = AJ.model_of(3)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]])
    return TorchANIBatchedNN(model.species_converter, model.neural_networks, numbers, layout=layout, **flags), species


def test_the_flag_stands_alone_and_needs_a_layout_with_a_weight_gradient():
    from NNPOps import OptimizedTorchANI
    with pytest.raises(ValueError, match="force_trainable=True stands alone"):
        _module("fused", trainable=True, force_trainable=True)
    for layout in ("gemm", "reference"):
        with pytest.raises(ValueError, match="force_trainable=True needs layout"):
            _module(layout, force_trainable=True)
    species, _ = AJ.molecule(23, 67)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]])
    with pytest.raises(ValueError, match="force_trainable=True stands alone"):
        OptimizedTorchANI(AJ.model_of(3), numbers, trainable=True, force_trainable=True)
    grouped, _ = _module("grouped", force_trainable=True)                       # already twice differentiable: a synonym of trainable=True
    assert type(grouped[0]).__name__ == "_TrainableGroupedNN"
    assert type(OptimizedTorchANI(AJ.model_of(3), numbers, force_trainable=True)).__name__ == "ForceTrainableOptimizedTorchANI"


def test_state_dicts_interchange_with_the_trainable_and_the_default_module():
    from NNPOps.BatchedNN import PARAMETER_NAMES
    force, _ = _module("fused", force_trainable=True)
    trainable, _ = _module("fused", trainable=True)
    default, _ = _module("fused")
    assert type(force[0]).__name__ == "_ForceTrainableFusedNN"
    assert [n for n, _ in force.named_parameters()] == ["0." + n for n in PARAMETER_NAMES] == [n for n, _ in trainable.named_parameters()]
    assert sorted(force.state_dict()) == sorted(trainable.state_dict()) == sorted(default.state_dict())
    built = force[0].plane_rebuilds
    with torch.no_grad():
        force[0].layer2_weights.mul_(1.5)
    for other in (trainable, default):
        other.load_state_dict(force.state_dict())
        assert torch.equal(other[0].layer2_weights, force[0].layer2_weights)
    for other in (_module("fused", trainable=True)[0], _module("fused")[0]):
        force.load_state_dict(other.state_dict())
        assert torch.equal(force[0].layer2_weights, other[0].layer2_weights) and isinstance(force[0].layer2_weights, torch.nn.Parameter)
    assert force[0].plane_rebuilds == built + 2                                 # load_state_dict rebuilds the planes, as for trainable=True
