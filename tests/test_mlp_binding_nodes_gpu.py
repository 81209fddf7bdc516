"""The autograd nodes of the fused atomic networks (torch_binding.cpp: FusedMLP, FusedMLPMembers, FusedMLPMembersTrainable,
FusedMLPMeanTrainable) called as ops: what a node keeps is its own, the surfaces agree where the design says so, every forward
argument has its gradient slot, and the upstream gradient may be float64 or hold zeros.  The weight gradients' values are judged in
test_mlp_weights_gpu.py; the surfaces through the modules in its `..._are_the_default_modules_bits` tests.

73 atoms, a kind of 70 (a full tile of 64 and a ragged one) and a kind of 3, three members, ordinary weights; F = 40 over all columns
(the dE/dy1 workspace), F = 1008 over 3 live blocks (dx_partial: the gradient formed in the forward launch) and over 17 (272 columns:
a narrow first layer, dE/dy1 again); one molecule and three conformers with offsets and places; with and without a float64 shift.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mlp_float64 as MJ
import mlp_pack_cases as P
import mlp_weights_float64 as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ATOMS, M, SMALL = 73, 3, (5, 30, 72)                     # the atoms of the second kind: the module's atom order is a real permutation
WIDTHS = [(96, 64, 32), (40, 32, 17)]
COLUMNS = {"F40": (40, None), "live3": (1008, P.CASES["ani2x-live3"][3]), "live17": (1008, P.CASES["ani2x-live17"][3])}
FRAMES = [pytest.param(c, B, s, id=f"{c}-B{B}{'-shift' if s else ''}") for c, B, s in itertools.product(COLUMNS, (1, 3), (False, True))]
SHIFT = -7.25
HOLDER = SimpleNamespace(reset_gradient_cache=lambda: None)          # (what _batch_plan keeps next to its tables)


@functools.lru_cache(maxsize=None)
def nets_of(columns):
    from NNPOps.BatchedNN import PARAMETER_NAMES, TorchANIBatchedNN
    F, live = COLUMNS[columns]
    numbers = torch.tensor([[1 if a in SMALL else 0 for a in range(ATOMS)]])
    nets = TorchANIBatchedNN(P._Converter(), P.ensemble(F, WIDTHS, M, 7, wide=False), numbers, trainable=True)[0].to(DEV)
    if live is not None:
        nets.set_live_blocks(live)
    assert nets.fused_ok and nets.group_sizes == [70, 3] and (nets.x_blocks.numel() == 0) == (live is None)
    return nets, [getattr(nets, name).detach() for name in PARAMETER_NAMES]


def frame(columns, B, seed=0):
    """x [B * 73, F] in [0, 0.5) as an AEV is, and the tables of the op call (the module's own for one molecule, _batch_plan's for B)"""
    nets, _ = nets_of(columns)
    x = (torch.rand((B * ATOMS, COLUMNS[columns][0]), generator=torch.Generator().manual_seed(100 * B + seed)) * 0.5).to(DEV)
    if B == 1:
        return x, (nets.atom_order32, nets.group_sizes, None, None)
    _, rows, sizes, places, offsets = nets._batch_plan(HOLDER, B, DEV)
    return x, (rows, sizes, offsets, places)


def run(op, columns, x, tables, shift=False, parameters=None):
    nets, own = nets_of(columns)
    rows, sizes, offsets, places = tables
    ops = torch.ops.NNPOpsBatchedNN
    if op == "FusedMLP":
        return ops.FusedMLP(x, rows, sizes, nets.widths, M, nets.mlp_planes, nets.mlp_floats, nets.act_scale_log2)
    live = nets.x_blocks.numel() > 0
    common = (x, rows, sizes, nets.widths, M, nets.live_planes if live else nets.mlp_planes, nets.mlp_floats, nets.x_blocks if live else None,
              nets.dead_blocks if live else None, nets.act_scale_log2, offsets, places,
              torch.tensor([SHIFT], dtype=torch.float64, device=DEV) if shift else None)
    parameters = own if parameters is None else parameters
    if op == "members":
        return ops.FusedMLPMembers(*common)
    if op == "members_trainable":
        return ops.FusedMLPMembersTrainable(*common, parameters)
    return ops.FusedMLPMeanTrainable(*common, parameters, op == "total")


def upstream(out, seed=1):
    """a fixed upstream gradient in the shape and type of `out`: both signs, and an exact zero in every row of [B, M]"""
    B = out.shape[0]
    w = MJ.random_weights(B, M, seed) if out.dim() == 2 else np.linspace(-0.75, 1.25, B).astype(np.float32)
    return torch.tensor(w, device=DEV).to(out.dtype)


def leaves(columns, x, with_parameters):
    own = [p.clone().requires_grad_(True) for p in nets_of(columns)[1]] if with_parameters else None
    return x.clone().requires_grad_(True), own


def same_bits(a, b):
    as_bytes = lambda t: t.detach().contiguous().view(torch.uint8)
    return len(a) == len(b) and all(s.dtype == t.dtype and s.shape == t.shape and torch.equal(as_bytes(s), as_bytes(t)) for s, t in zip(a, b))


@pytest.mark.parametrize("op", ["members", "members_trainable", "mean", "total"])
@pytest.mark.parametrize("columns, B, shift", FRAMES)
def test_a_node_owns_what_it_keeps(op, columns, B, shift):
    """two calls with different x, then the FIRST output's backward: the gradients of a run in which only the first call was made"""
    x, tables = frame(columns, B)
    other, _ = frame(columns, B, seed=1)
    got = []
    for second in (True, False):
        p, own = leaves(columns, x, op != "members")
        out = run(op, columns, p, tables, shift, own)
        if second:
            q, others = leaves(columns, other, op != "members")
            later = run(op, columns, q, tables, shift, others)             # (alive, with what IT keeps, while the first goes back)
        got.append(torch.autograd.grad((out * upstream(out)).sum(), [p] + (own or [])))
    assert float(got[0][0].abs().max()) > 0 and same_bits(*got)


def test_the_two_launch_node_owns_what_it_keeps():
    x, tables = frame("F40", 1)
    other, _ = frame("F40", 1, seed=1)
    got = []
    for second in (True, False):
        p = x.clone().requires_grad_(True)
        out = run("FusedMLP", "F40", p, tables)
        if second:
            later = run("FusedMLP", "F40", other.clone().requires_grad_(True), tables)
        got.append(torch.autograd.grad(out.sum() * 0.75, [p]))
    assert float(got[0][0].abs().max()) > 0 and same_bits(*got)


def judged_kinds(columns, tables):
    """the module's networks as the float64 judges take them: over the columns the call reads, the atoms the rows of the call's kinds"""
    nets, _ = nets_of(columns)
    live = COLUMNS[columns][1]
    cols = torch.arange(COLUMNS[columns][0]) if live is None else torch.tensor([16 * g + i for g in live for i in range(16)])
    kinds, first = W.kinds_of_module(nets), 0
    for kd, n in zip(kinds, tables[1]):
        kd["w0"], kd["atoms"] = kd["w0"][:, :, cols].contiguous(), tables[0][first:first + n].cpu()
        first += n
    return kinds, cols


@pytest.mark.parametrize("columns, B, shift", FRAMES)
def test_the_surfaces_agree(columns, B, shift):
    """FusedMLPMembersTrainable is FusedMLPMembers in value and d/dx, bit for bit; the mean node is another kernel sequence than
    members.mean(1): both are judged in float64.  Bar: a per-atom energy is within E_BAR of the largest |e| (mlp_float64.py), a
    molecule adds 73 of them, the mean over the members does not add to it: 73 E_BAR max |e| for either."""
    x, tables = frame(columns, B)
    got = {}
    for op in ("members", "members_trainable", "mean"):
        p, own = leaves(columns, x, op != "members")
        out = run(op, columns, p, tables, shift, own)
        got[op] = (out.detach(), torch.autograd.grad((out * upstream(out)).sum(), p)[0])
    assert same_bits(got["members"], got["members_trainable"]) and got["members"][0].shape == (B, M)
    assert got["mean"][0].shape == (B,) and got["mean"][0].dtype == (torch.float64 if shift else torch.float32)
    kinds, cols = judged_kinds(columns, tables)
    J = MJ.judge(kinds, x.cpu()[:, cols].contiguous())
    e = np.zeros((B * ATOMS, M))
    e[np.concatenate([kd["atoms"].numpy() for kd in kinds])] = J.e                 # (J.e: kind after kind)
    want = e.reshape(B, ATOMS, M).sum(1).mean(1) + (SHIFT if shift else 0.0)
    bar = ATOMS * MJ.E_BAR * float(np.abs(J.e).max())
    for name, mean in (("mean", got["mean"][0]), ("members.mean(1)", got["members"][0].mean(1))):
        err = float(np.abs(mean.double().cpu().numpy() - want).max())
        print(f"\n[mlp-nodes] {columns} B={B} shift={shift} {name}: {err:.2e} (bar {bar:.2e})", end="")
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("op", ["members_trainable", "mean"])
@pytest.mark.parametrize("columns, B, shift", FRAMES)
def test_every_argument_has_its_slot(op, columns, B, shift):
    x, tables = frame(columns, B)
    p, own = leaves(columns, x, True)
    out = run(op, columns, p, tables, shift, own)
    w = upstream(out)
    nine = torch.autograd.grad((out * w).sum(), [p] + own)
    assert len(nine) == 9 and all(g is not None and g.shape == t.shape and g.dtype == t.dtype for g, t in zip(nine, [p] + own))
    _, own = leaves(columns, x, True)
    eight = torch.autograd.grad((run(op, columns, x, tables, shift, own) * w).sum(), own)
    assert same_bits(eight, nine[1:])
    # the last bias alone: the judge's closed form is the sum of the upstream weights over the atoms of the kind
    last = [t.clone() for t in nets_of(columns)[1]]
    last[7].requires_grad_(True)
    db6, = torch.autograd.grad((run(op, columns, x, tables, shift, last) * w).sum(), last[7])
    kinds, _ = judged_kinds(columns, tables)
    per_member = w.double().cpu().numpy() if op == "members_trainable" else np.repeat(w.double().cpu().numpy()[:, None] / M, M, 1)
    c = W.atom_weights(kinds, per_member, None if B == 1 else ATOMS * np.arange(B + 1))
    want = np.stack([ck.sum(1) for ck in c])
    assert db6.shape == (2, M, 1, 1) and (np.abs(db6[:, :, 0, 0].cpu().numpy() - want).max(1) <= W.G_BAR * np.abs(want).max(1)).all()


@pytest.mark.parametrize("op", ["members", "members_trainable"])
@pytest.mark.parametrize("columns, B", [(c, B) for c in COLUMNS for B in (1, 3)])
def test_upstream_in_float64_and_a_member_at_zero(op, columns, B):
    """the float64 upstream gradient of the shifted energies gives the d/dx of its float32 cast on the float32 energies; a member whose
    upstream gradient is zero in every molecule has parameter gradients of exactly zero"""
    x, tables = frame(columns, B)
    w = upstream(torch.empty((B, M), device=DEV), seed=2).abs() + 0.125
    w[:, 1] = 0.0
    got = []
    for shift in (True, False):
        p, own = leaves(columns, x, op != "members")
        out = run(op, columns, p, tables, shift, own)
        assert out.dtype == (torch.float64 if shift else torch.float32)
        got.append(torch.autograd.grad((out * w.to(out.dtype)).sum(), [p] + (own or [])))
    assert float(got[0][0].abs().max()) > 0 and same_bits(*got)
    for g in got[0][1:]:
        assert not g[:, 1].any() and g[:, 0].any() and g[:, 2].any()
