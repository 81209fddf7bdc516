"""Per-member energies of an ANI ensemble and their QBC factor on the GPU: OptimizedTorchANI.members_energies(_batch) /
energies_qbcs(_batch), torch.ops.NNPOpsBatchedNN.FusedMLPMembers and the C entries behind them (nnpops_mlp_member_sums, the
member_weights of nnpops_mlp_input_grad).

Inputs and judge: tests/ani_members_float64.py.  The three paths of the networks' input gradient: "live" -- the 23-atom molecule as
HCNO, 384 live columns, the weighted mlp_input_grad over x_groups with 8, 7 and 6 K steps per member (H, C, N / O); "all-columns" --
live_columns=False, 1 008 columns, the same kernel; "partial" -- the molecule as HCO, 240 columns, every member's share formed by the
forward launch and added up with weights by mlp_sum_members.

Bars: a member energy 5e-6 |E| + 1e-4 (the project's energy bar, applied to the UNSHIFTED member energy); a gradient of
sum_m w_m E_m 1e-4 of the largest entry of sum_m |w_m| |dE_m/dx| per conformer (the sum of magnitudes: cancellation between members
cannot turn rounding of the parts into a failure); sigma 2e-4 absolute (sigma is 1-Lipschitz in the max-norm of the member energies up
to sqrt(M / (M - 1))).  A member whose upstream weight is zero is SKIPPED by the weighted kernels: test_one_hot_weights_skip_the_others.
"""
import functools

import numpy as np
import pytest
import torch

import ani_members_float64 as J
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLOTS = J.SLOTS
ENERGY_RTOL, ENERGY_ATOL, GRAD_RTOL, SIGMA_ATOL = 5e-6, 1e-4, 1e-4, 2e-4
PATHS = [("HCNO", True), ("HCNO", False), ("HCO", True)]
PATH_IDS = ["live", "all-columns", "partial"]


def _numbers(species):
    return torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=DEV)


@functools.lru_cache(maxsize=None)
def build(kinds="HCNO", live_columns=True, members=3, n_atoms=23, count=67):
    from NNPOps import OptimizedTorchANI
    species, _ = J.molecule(n_atoms, count, kinds)
    numbers = _numbers(species)
    module = OptimizedTorchANI(J.model_of(members), numbers.cpu(), live_columns=live_columns).to(DEV)
    assert type(module).__name__ == "FusedOptimizedTorchANI"
    if n_atoms == 23:
        assert 16 * module.neural_networks[0].x_blocks.numel() == ({"HCNO": 384, "HCO": 240}[kinds] if live_columns else 0)
    return module, numbers


def picks_of(batch):
    return list(range(67)) if batch == 67 else SLOTS[:batch]


def coords_of(n_atoms, count, picks):
    return torch.tensor(J.molecule(n_atoms, count)[1][picks], device=DEV)


def members_and_gradient(module, numbers, coords, w):
    """-> E [B][M] float64 (shifted) and the gradient [B, N, 3] of sum_b sum_m w[b][m] E[b][m]"""
    p = coords.clone().requires_grad_(True)
    E = module.members_energies_batch((numbers.expand(p.shape[0], -1), p)).energies
    assert E.dtype == torch.float64 and E.shape == (w.shape[1], p.shape[0])
    (E.t() * torch.tensor(w, device=DEV)).sum().backward()
    return E.detach().t().contiguous(), p.grad.detach()


def unshifted_members(module, coords):
    """the op without a shift: [B][M] float32"""
    nets = module.neural_networks[0]
    B, N = int(coords.shape[0]), int(coords.shape[1])
    _, rows, sizes, places, offsets = nets._batch_plan(module.aev_computer.batch_holder(B), B, DEV)
    aev = torch.ops.NNPOpsANISymmetryFunctions.aev(module.aev_computer.batch_holder(B), coords.reshape(B * N, 3), None)
    out = nets.fused_members(aev, None, (rows, sizes, places, offsets))
    assert out.dtype == torch.float32 and out.shape == (B, nets.num_models)
    return out


def check_energies(tag, E, E_ref):
    E = E.double().cpu().numpy()
    assert E.shape == E_ref.shape
    err = np.abs(E - E_ref)
    print(f"\n[ani-members] {tag}: member energy error up to {err.max():.2e} ({(err / np.abs(E_ref)).max():.2e} of the member energy)")
    assert (err <= ENERGY_RTOL * np.abs(E_ref) + ENERGY_ATOL).all(), (tag, err.max())


def check_gradient(tag, grad, w, G_ref):
    grad = grad.double().cpu().numpy()
    worst, worst_own = 0.0, 0.0
    for b in range(len(w)):
        want = J.combine(w[b], G_ref[b])
        err = np.abs(grad[b] - want).max()
        worst, worst_own = max(worst, err / J.magnitude(w[b], G_ref[b])), max(worst_own, err / np.abs(want).max())
        assert err <= GRAD_RTOL * J.magnitude(w[b], G_ref[b]), (tag, b, err, J.magnitude(w[b], G_ref[b]))
    print(f"\n[ani-members] {tag}: gradient error up to {worst:.2e} of sum |w||g|, {worst_own:.2e} of the result's own largest entry")


# ---------------------------------------------------------------------------------------------- 1. against float64
def against_float64(batch, kinds, live_columns, members):
    module, numbers = build(kinds, live_columns, members)
    picks = picks_of(batch)
    coords = coords_of(23, 67, picks)
    E_ref, G_ref = J.judge(23, 67, kinds, members, None if members == 3 else tuple(picks))
    if members == 3:
        E_ref, G_ref = E_ref[picks], G_ref[picks]
    tag = f"B={batch} {kinds} live_columns={live_columns} M={members}"
    plain = unshifted_members(module, coords)
    check_energies(tag, plain, E_ref)
    w = J.random_weights(batch, members, seed=batch + members)
    E, grad = members_and_gradient(module, numbers, coords, w)
    species = J.molecule(23, 67, kinds)[0]
    assert float((E - J.self_energy(species) - plain.double()).abs().max()) <= 1e-9          # shifted = (double)(float)sum + shift
    check_gradient(tag, grad, w, G_ref)
    return module


@pytest.mark.parametrize("kinds,live_columns", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("batch", [1, 2, 5, 67])
def test_members_against_float64(batch, kinds, live_columns):
    """At B = 67 the species' runs (737, 469, 67, 268 atoms; 804, 469, 268 for HCO) end inside 64-atom tiles and conformers share
    tiles: a tile's columns take the weights of several conformers."""
    module = against_float64(batch, kinds, live_columns, 3)
    if batch == 67:
        assert [n * 67 for n in module.neural_networks[0].group_sizes] == ([737, 469, 67, 268] if kinds == "HCNO" else [804, 469, 268])


@pytest.mark.parametrize("kinds,live_columns", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("members", [8, 2])
def test_eight_and_two_members_against_float64(members, kinds, live_columns):
    """8 members: 64, 56 and 48 K steps, the member boundaries at every phase of the loop's unroll of four; 2 members: the shortest"""
    against_float64(5, kinds, live_columns, members)


# ---------------------------------------------------------------------------------------------- 2. QBC
@pytest.mark.parametrize("unbiased", [True, False])
@pytest.mark.parametrize("kinds", ["HCNO", "HCO"])
def test_energies_qbcs_against_float64(kinds, unbiased):
    module, numbers = build(kinds)
    species = J.molecule(23, 67, kinds)[0]
    E_ref, G_ref = J.judge(23, 67, kinds, 3)
    root_n = np.sqrt(23.0)
    for batch in (1, 5):
        coords = coords_of(23, 67, SLOTS[:batch])
        p = coords.clone().requires_grad_(True)
        if batch == 1:
            sp, e, q = module.energies_qbcs((numbers, p), unbiased=unbiased)
            mean = module((numbers, coords)).energies
        else:
            sp, e, q = module.energies_qbcs_batch((numbers.expand(batch, -1), p), unbiased=unbiased)
            mean = module.forward_batch((numbers.expand(batch, -1), coords)).energies
        assert e.shape == (batch,) and q.shape == (batch,) and e.dtype == torch.float64 and q.dtype == torch.float64 and sp.shape == (batch, 23)
        q.sum().backward()
        for b, slot in enumerate(SLOTS[:batch]):
            s_ref = J.sigma(E_ref[slot], unbiased)
            assert abs(float(q[b].detach()) * root_n - s_ref) <= SIGMA_ATOL, (b, float(q[b].detach()) * root_n, s_ref)
            e_want = E_ref[slot].mean() + J.self_energy(species)
            assert abs(float(e[b].detach()) - e_want) <= ENERGY_RTOL * abs(e_want) + ENERGY_ATOL
            assert abs(float(e[b].detach()) - float(mean[b])) <= ENERGY_RTOL * abs(float(mean[b])) + ENERGY_ATOL      # (another order of summation: not bit-equal)
        w = np.stack([J.sigma_weights(E_ref[slot], unbiased) / root_n for slot in SLOTS[:batch]])
        check_gradient(f"d qbcs / dx B={batch} {kinds} unbiased={unbiased}", p.grad, w, G_ref[SLOTS[:batch]])


# ---------------------------------------------------------------------------------------------- 3. exact cases
def test_exact_member_energies_from_last_layer_biases():
    """layer 6 weights zero, its bias 2^-(k + 1 + m) for species k and member m, self energies zero: member m's energy is
    sum_k count_k 2^-(k + 1 + m) exactly (all terms and partial sums are float32 numbers) and every gradient is exactly zero"""
    from NNPOps import OptimizedTorchANI
    model = workloads.torchani_like_model(n_models=3, seed=8)
    for m, member in enumerate(model.neural_networks):
        for k, sym in enumerate(("H", "C", "N", "O")):
            member[sym][6].weight.data.zero_()
            member[sym][6].bias.data.fill_(2.0 ** -(k + 1 + m))
    for kinds, live_columns in PATHS:
        species = J.molecule(23, 67, kinds)[0]
        numbers = _numbers(species)
        want = torch.tensor([sum(int((species == k).sum()) * 2.0 ** -(k + 1 + m) for k in range(4)) for m in range(3)], dtype=torch.float64, device=DEV)
        module = OptimizedTorchANI(model, numbers.cpu(), live_columns=live_columns).to(DEV)
        for batch in (5, 67):
            coords = coords_of(23, 67, picks_of(batch))
            E, grad = members_and_gradient(module, numbers, coords, J.random_weights(batch, 3, seed=batch))
            assert torch.equal(E, want.expand(batch, 3)), E
            assert torch.equal(unshifted_members(module, coords).double(), want.expand(batch, 3))
            assert torch.equal(grad, torch.zeros_like(grad))


def _poison_first_layers(nets, keep):
    """NaN into the transposed first-layer planes of every member but `keep`, in place -- the K steps of the member in w0t (the
    operand of mlp_input_grad) and its w0tm (the operand of the forward launch's share): those members' shares of dE/dAEV are NaN
    from then on, their energies are untouched.  (the layout of the packed planes: torch_binding.cpp, mlp_prepare)"""
    live = nets.x_blocks.numel() > 0
    planes = nets.live_planes if live else nets.mlp_planes
    F = 16 * int(nets.x_blocks.numel()) if live else 1008
    M = nets.num_models
    halves = lambda rows, cols: ((rows + 15) // 16) * ((cols + 31) // 32) * 1024
    at = 0
    for k in range(len(nets.group_sizes)):
        h1, h2, h3 = nets.widths[3 * k:3 * k + 3]
        at += M * (halves(h1, F) + halves(h2, h1) + halves(h3, h2) + halves(h2, h3) + halves(h1, h2))
        w0t = planes[at:at + halves(F, M * h1)].view((F + 15) // 16, M * (h1 // 32), 1024)       # [row block][K step][2 planes x 512]
        for m in range(M):
            if m != keep:
                w0t[:, m * (h1 // 32):(m + 1) * (h1 // 32)] = float("nan")
        at += halves(F, M * h1)
        if live and F <= 256:
            for m in range(M):
                if m != keep:
                    planes[at + m * halves(F, h1):at + (m + 1) * halves(F, h1)] = float("nan")
            at += M * halves(F, h1)
    assert at == planes.numel()


@pytest.mark.parametrize("kinds,live_columns", PATHS, ids=PATH_IDS)
def test_one_hot_weights_skip_the_others(kinds, live_columns):
    """A zero upstream weight skips its member (nnpops_hip.h: member_weights): with every other member's transposed first layer NaN
    the gradient of all members together is NaN, the gradient of member m alone is finite -- and the very bits the intact module
    gives, since member m's arithmetic is untouched."""
    from NNPOps import OptimizedTorchANI
    module, numbers = build(kinds, live_columns)
    coords = coords_of(23, 67, SLOTS)
    sp = numbers.expand(5, -1)
    for keep in (0, 2):
        broken = OptimizedTorchANI(J.model_of(3), numbers.cpu(), live_columns=live_columns).to(DEV)
        _poison_first_layers(broken.neural_networks[0], keep)
        results = []
        for mod in (module, broken):
            p = coords.clone().requires_grad_(True)
            (together,) = torch.autograd.grad(mod.members_energies_batch((sp, p)).energies.sum(), p)
            E = mod.members_energies_batch((sp, p)).energies
            E[keep].sum().backward()
            results.append((E.detach(), p.grad, together))
        (E0, g0, t0), (E1, g1, t1) = results
        assert torch.equal(E0, E1)
        assert bool(torch.isfinite(t0).all()) and bool(torch.isnan(t1).any())                  # (the poison bites)
        assert bool(torch.isfinite(g1).all()) and torch.equal(g0, g1) and float(g0.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- 4. bitwise properties
@pytest.mark.parametrize("kinds,live_columns", PATHS, ids=PATH_IDS)
def test_repeats_and_batch_placement_are_bitwise(kinds, live_columns):
    module, numbers = build(kinds, live_columns)
    w67 = J.random_weights(67, 3, seed=9)
    five, all67 = coords_of(23, 67, SLOTS), coords_of(23, 67, list(range(67)))
    E5, g5 = members_and_gradient(module, numbers, five, w67[SLOTS])             # (its weights stay with the conformer)
    E5b, g5b = members_and_gradient(module, numbers, five, w67[SLOTS])
    assert torch.equal(E5, E5b) and torch.equal(g5, g5b)
    E67, g67 = members_and_gradient(module, numbers, all67, w67)
    assert torch.equal(E67[SLOTS], E5) and torch.equal(g67[SLOTS], g5)
    assert not torch.equal(E67[:5], E5)


def test_existing_methods_keep_their_bits():
    module, numbers = build()
    coords = coords_of(23, 67, SLOTS)
    sp5 = numbers.expand(5, -1)

    def existing():
        p = coords[:1].clone().requires_grad_(True)
        e = module((numbers, p)).energies
        e.backward()
        pb = coords.clone().requires_grad_(True)
        eb = module.forward_batch((sp5, pb)).energies
        eb.sum().backward()
        ef = module.energy_and_forces((numbers, coords[:1]))
        aev = module.aev_computer((module.species_converter((numbers, coords[:1])).species, coords[:1]))[1].detach().requires_grad_(True)
        net = module.neural_networks((numbers, aev)).energies                   # FusedMLP
        net.backward()
        return [e.detach(), p.grad, eb.detach(), pb.grad, ef[0], ef[1], net.detach(), aev.grad]

    before = existing()
    for _ in range(2):
        members_and_gradient(module, numbers, coords, J.random_weights(5, 3, seed=1))
        p = coords[:1].clone().requires_grad_(True)
        module.energies_qbcs((numbers, p))[2].sum().backward()
    after = existing()
    for a, b in zip(before, after):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 5. larger than a tile and a wave
def test_molecule_larger_than_a_tile():
    module, numbers = build("HCNO", True, 3, 70, 3)
    coords = coords_of(70, 3, [0, 1, 2])
    E_ref, G_ref = J.judge(70, 3, "HCNO", 3)
    check_energies("N=70 B=3", unshifted_members(module, coords), E_ref)
    w = J.random_weights(3, 3, seed=70)
    _, grad = members_and_gradient(module, numbers, coords, w)
    check_gradient("N=70 B=3", grad, w, G_ref)


# ---------------------------------------------------------------------------------------------- 6. surface
def test_periodic_single_molecule():
    from NNPOps import OptimizedTorchANI
    species, pos, box = J.periodic_frame()
    numbers = _numbers(species)
    model = J.model_of(3)
    module = OptimizedTorchANI(model, numbers.cpu()).to(DEV)
    assert type(module).__name__ == "FusedOptimizedTorchANI"
    E_ref, G_ref = J.judge_frames(species, [pos], model, box=box)
    p = torch.tensor(pos[None], device=DEV, requires_grad=True)
    cell, pbc = torch.tensor(box, device=DEV), torch.tensor([True, True, True], device=DEV)
    out = module.members_energies((numbers, p), cell, pbc)
    assert out.energies.shape == (3, 1) and out.energies.dtype == torch.float64
    check_energies("periodic N=100", out.energies.detach().t() - J.self_energy(species), E_ref)
    w = J.random_weights(1, 3, seed=100)
    (out.energies.t() * torch.tensor(w, device=DEV)).sum().backward()
    check_gradient("periodic N=100", p.grad, w, G_ref)
    mean = module((numbers, p.detach()), cell, pbc).energies
    _, e, q = module.energies_qbcs((numbers, p.detach()), cell, pbc)
    assert abs(float(e) - float(mean)) <= ENERGY_RTOL * abs(float(mean)) + ENERGY_ATOL
    assert abs(float(q) * 10.0 - J.sigma(E_ref[0])) <= SIGMA_ATOL
    with pytest.raises(ValueError, match='"pbc" has to be defined'):
        module.members_energies((numbers, p), cell)


def test_plain_path_agrees_with_the_fused_one():
    from NNPOps import OptimizedTorchANI
    module, numbers = build()
    plain = OptimizedTorchANI(J.model_of(3), numbers.cpu(), nn_layout="grouped", fused_step=False).to(DEV)
    assert type(plain).__name__ == "OptimizedTorchANI"
    coords = coords_of(23, 67, SLOTS)
    w = J.random_weights(5, 3, seed=4)
    E, grad = members_and_gradient(module, numbers, coords, w)
    E2, grad2 = members_and_gradient(plain, numbers, coords, w)
    species = J.molecule(23, 67)[0]
    unshifted = (E2 - J.self_energy(species)).abs()
    assert bool(((E - E2).abs() <= ENERGY_RTOL * unshifted + ENERGY_ATOL).all())
    _, G_ref = J.judge(23, 67, "HCNO", 3)
    for b, slot in enumerate(SLOTS):
        assert float((grad[b] - grad2[b]).abs().max()) <= GRAD_RTOL * J.magnitude(w[b], G_ref[slot])
    # one molecule through the module's own members_energies / energies_qbcs
    p = coords[:1].clone().requires_grad_(True)
    one = plain.members_energies((numbers, p)).energies
    assert one.shape == (3, 1) and one.dtype == torch.float64
    assert bool(((one[:, 0] - E[0]).abs() <= ENERGY_RTOL * unshifted[0] + ENERGY_ATOL).all())
    q = plain.energies_qbcs((numbers, p))[2]
    (dq,) = torch.autograd.grad(q.sum(), p)
    want = J.combine(J.sigma_weights(J.judge(23, 67, "HCNO", 3)[0][SLOTS[0]]) / np.sqrt(23.0), G_ref[SLOTS[0]])
    assert np.abs(dq[0].double().cpu().numpy() - want).max() <= 1e-3 * np.abs(want).max()      # (a loose look: the bars are test 2's)


def test_forward_only_op_is_capturable():
    module, _ = build()
    nets = module.neural_networks[0]
    coords = coords_of(23, 67, SLOTS)
    _, rows, sizes, places, offsets = nets._batch_plan(module.aev_computer.batch_holder(5), 5, DEV)
    static = torch.ops.NNPOpsANISymmetryFunctions.aev(module.aev_computer.batch_holder(5), coords.reshape(115, 3), None).detach().clone()
    shift = module.energy_shifter.self_energies
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            nets.fused_members(static, shift, (rows, sizes, places, offsets))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = nets.fused_members(static, shift, (rows, sizes, places, offsets))
    for k in range(2):
        with torch.no_grad():
            static.mul_(0.75 + 0.5 * k)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, nets.fused_members(static, shift, (rows, sizes, places, offsets)))


def test_refusals():
    module, numbers = build()
    nets = module.neural_networks[0]
    sp = numbers.expand(5, -1)
    coords = coords_of(23, 67, SLOTS)
    p = coords.clone().requires_grad_(True)
    E = module.members_energies_batch((sp, p)).energies
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(E.sum(), p, create_graph=True)
    for method in (module.members_energies_batch, module.energies_qbcs_batch):
        with pytest.raises(ValueError, match="non-periodic"):
            method((sp, coords), torch.eye(3, device=DEV), torch.tensor([True, True, True]))
        with pytest.raises(ValueError, match="non-periodic"):
            method((sp, coords), None, torch.tensor([True, True, True]))
        for bad in (coords[:, :22], coords[0], coords[:0]):                      # (the last one: an empty batch)
            with pytest.raises(ValueError, match="positions"):
                method((sp, bad))
    _, rows, sizes, places, offsets = nets._batch_plan(module.aev_computer.batch_holder(5), 5, DEV)
    aev = torch.ops.NNPOpsANISymmetryFunctions.aev(module.aev_computer.batch_holder(5), coords.reshape(115, 3), None).requires_grad_(True)
    out = nets.fused_members(aev, None, (rows, sizes, places, offsets))
    with pytest.raises(RuntimeError, match="shape"):
        out.backward(torch.ones(3, 5, device=DEV))                                # a gradient of the wrong shape
    op = torch.ops.NNPOpsBatchedNN.FusedMLPMembers
    args = (rows, sizes, nets.widths, nets.num_models, nets.live_planes, nets.mlp_floats, nets.x_blocks, nets.dead_blocks, nets.act_scale_log2)
    with pytest.raises(RuntimeError, match="empty batch"):
        op(aev[:0], *args, offsets, places, None)
    with pytest.raises(RuntimeError, match="empty batch"):
        op(aev, *args, offsets[:1].contiguous(), places, None)
    with pytest.raises(RuntimeError, match="come together"):
        op(aev, *args, offsets, None, None)
    with pytest.raises(RuntimeError, match="row places"):                         # tables of another batch
        op(aev, *args, offsets, places[:92].contiguous(), None)
    with pytest.raises(RuntimeError, match="int32"):
        op(aev, *args, offsets.long(), places, None)
    with pytest.raises(RuntimeError, match="self-energy shift"):
        op(aev, *args, offsets, places, torch.zeros(1, device=DEV))


def test_autograd_graph_has_two_custom_nodes():
    module, numbers = build()
    coords = coords_of(23, 67, SLOTS)
    for batch in (1, 5):
        p = coords[:batch].clone().requires_grad_(True)
        E = (module.members_energies((numbers, p)) if batch == 1 else module.members_energies_batch((numbers.expand(5, -1), p))).energies
        names, todo, seen = [], [E.grad_fn], set()
        while todo:
            fn = todo.pop()
            if fn is None or fn in seen:
                continue
            seen.add(fn)
            names.append(fn.name())
            todo += [nxt for nxt, _ in fn.next_functions]
        custom = [n for n in names if "Function" in n]
        assert len(custom) == 2 and any("FusedMLPMembersFunction" in n for n in custom) and any("FusedAutogradFunction" in n for n in custom), names
        assert len(names) <= 8, names                                             # (not the ~45 nodes of the composition)
