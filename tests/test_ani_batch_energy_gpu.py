"""Energies and forces of a conformer batch in one step: OptimizedTorchANI.forward_batch / energy_and_forces_batch, the ops
torch.ops.NNPOpsANISymmetryFunctions.energy_batch / energy_forces_batch and the C entries behind them.

The molecule is workloads.conformer(23) with its species overwritten to 11 H, 7 C, 1 N and 4 O (one species with a single atom per
molecule), the conformers are its positions jittered by up to 0.1 A.  ONE set of 67 conformers serves every test: the batch of five is
its slots 60, 3, 17, 41, 66 (so the batch-invariance test has its placements for free) and the batches of one and two the first of
those.  The judge of energies and forces is the plain per-species evaluation of the networks in float64 on the oracle's AEV, as in
test_torch_surface_gpu.py::test_batched_nn_and_optimized_torchani, at that test's bars: energy 5e-6 |e| + 1e-4, forces 1e-4 of the
conformer's largest force.  It is computed once per molecule and conformer set and not changed.

Which launch takes the mean: H, C, N and O fill 4 * 16 + 10 * 32 = 384 AEV columns, more than the 256 up to which the forward launch
forms the input gradient itself (dx_partial) -- so with that molecule the mean is a launch of its own whether live_columns is set or
not.  The same 23 positions with 12 H, 7 C and 4 O ("HCO": 3 * 16 + 6 * 32 = 240 columns) take the other path, where the means ride in
the launch that adds the members up; every check that depends on the path runs on both molecules.
"""
import functools
import io

import numpy as np
import pytest
import torch

from ani_float64 import random_grouping, segment_means
from nnpops_amd import workloads
from oracle import AniOracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SAE = [-0.5, -38.0, -54.7, -75.2, -398.1, -99.8, -460.1]
SLOTS = [60, 3, 17, 41, 66]
ENERGY_RTOL, ENERGY_ATOL, FORCE_RTOL = 5e-6, 1e-4, 1e-4


def _numbers(species):
    return torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=DEV)


@functools.lru_cache(maxsize=None)
def molecule(n_atoms, count, kinds="HCNO"):
    """-> (species [n], conformers [count][n][3] float32); the conformers do not depend on `kinds`"""
    base, species = workloads.conformer(n_atoms, seed=40 + n_atoms)
    if n_atoms == 23:
        species = np.array({"HCNO": [0] * 11 + [1] * 7 + [2] + [3] * 4, "HCO": [0] * 12 + [1] * 7 + [3] * 4}[kinds], dtype=np.int32)
        species = species[np.random.default_rng(5).permutation(23)]
    rng = np.random.default_rng(100 + n_atoms)
    confs = np.stack([base + rng.uniform(-0.1, 0.1, base.shape).astype(np.float32) for _ in range(count)]).astype(np.float32)
    return species, confs


@functools.lru_cache(maxsize=None)
def model_of(seed=12):
    return workloads.torchani_like_model(n_models=3, seed=seed, self_energies=SAE)


@functools.lru_cache(maxsize=None)
def judge(n_atoms, count, kinds="HCNO", seed=12):
    """float64 energies [count] and dE/dpositions [count][n][3] of every conformer: the networks of model_of(seed) per species on the
    oracle's AEV, the AEV backward by the oracle"""
    species, confs = molecule(n_atoms, count, kinds)
    model = model_of(seed)
    syms = list(workloads.ANI2X_WIDTHS)
    oracle = AniOracle(7, 5.1, 3.5, species, *workloads.ani2x_functions(), periodic=False)
    sae = float(sum(SAE[s] for s in species))
    nets = [{sym: net.double() for sym, net in member.items()} for member in model.neural_networks]
    energies, grads = np.empty(count), np.empty((count, n_atoms, 3))
    try:
        for b in range(count):
            r_ref, a_ref = oracle.forward(confs[b])
            aev = torch.tensor(np.concatenate([r_ref, a_ref], axis=1), dtype=torch.float64, requires_grad=True)
            total = 0
            for member in nets:
                for s in sorted(set(species.tolist())):
                    idx = torch.tensor(np.nonzero(species == s)[0])
                    total = total + member[syms[s]](aev[idx]).sum()
            e = total / len(nets)
            e.backward()
            energies[b] = float(e.detach()) + sae
            g = aev.grad.float().numpy()
            grads[b] = oracle.backward(np.ascontiguousarray(g[:, :112]), np.ascontiguousarray(g[:, 112:]))
    finally:
        for member in model.neural_networks:
            member.float()
    return energies, grads


def build(n_atoms=23, count=67, kinds="HCNO", **kwargs):
    from NNPOps import OptimizedTorchANI
    species, _ = molecule(n_atoms, count, kinds)
    numbers = _numbers(species)
    module = OptimizedTorchANI(model_of(), numbers.cpu(), **kwargs).to(DEV)
    if n_atoms == 23 and kwargs.get("live_columns", True):        # (the path the mean takes: see the head of this file)
        assert 16 * module.neural_networks[0].x_blocks.numel() == {"HCNO": 384, "HCO": 240}[kinds]
    return module, numbers


def batch_of(n_atoms, count, picks):
    _, confs = molecule(n_atoms, count)
    return torch.tensor(confs[picks], device=DEV)


def run_weighted(module, numbers, coords, seed=0):
    """energies and the gradient of sum(w_b e_b) with a different random weight per conformer -> (e [B], grad [B, N, 3], w [B])"""
    p = coords.clone().requires_grad_(True)
    e = module.forward_batch((numbers.expand(p.shape[0], -1), p)).energies
    w = torch.rand(p.shape[0], dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) + 0.5
    (e * w).sum().backward()
    return e.detach(), p.grad.detach(), w


def check_against_judge(tag, e, grad, w, e_ref, g_ref):
    e, grad, w = e.cpu().numpy(), grad.cpu().numpy().astype(np.float64), w.cpu().numpy()
    assert e.dtype == np.float64 and e.shape == e_ref.shape and grad.shape == g_ref.shape
    worst_e, worst_f = 0.0, 0.0
    for b in range(len(e)):
        err_e = abs(e[b] - e_ref[b])
        err_f = np.abs(grad[b] - w[b] * g_ref[b]).max() / np.abs(w[b] * g_ref[b]).max()
        worst_e, worst_f = max(worst_e, err_e), max(worst_f, err_f)
        assert err_e <= ENERGY_RTOL * abs(e_ref[b]) + ENERGY_ATOL, (tag, b, e[b], e_ref[b])
        assert err_f <= FORCE_RTOL, (tag, b, err_f)
    print(f"\n[ani-batch-energy] {tag}: energy error up to {worst_e:.2e}, force error up to {worst_f:.2e} of the conformer's largest")


def picks_of(batch):
    return list(range(67)) if batch == 67 else SLOTS[:batch]


# ---------------------------------------------------------------------------------------------- 1. against float64
PATHS = [("HCNO", True), ("HCNO", False), ("HCO", True)]
PATH_IDS = ["live", "all-columns", "mean-rides"]


@pytest.mark.parametrize("kinds,live_columns", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("batch", [1, 2, 5, 67])
def test_batch_against_float64(batch, kinds, live_columns):
    """737, 469, 67 and 268 atoms per species at B = 67: every species' run ends inside a 64-atom tile and molecules share tiles
    (804, 469 and 268 for the three species of "HCO").  live: 384 of the 1 008 columns, a separate gradient launch and a mean launch
    of its own; all-columns: 1 008 columns, the same launches; mean-rides: 240 columns, the gradient is formed in the forward launch
    and the means ride with the sum over the members."""
    module, numbers = build(kinds=kinds, live_columns=live_columns)
    assert type(module).__name__ == "FusedOptimizedTorchANI"
    assert (module.neural_networks[0].x_blocks.numel() > 0) == live_columns
    picks = picks_of(batch)
    e, grad, w = run_weighted(module, numbers, batch_of(23, 67, picks), seed=batch)
    e_ref, g_ref = judge(23, 67, kinds)
    check_against_judge(f"B={batch} {kinds} live_columns={live_columns}", e, grad, w, e_ref[picks], g_ref[picks])
    if batch == 67:
        assert [n * 67 for n in module.neural_networks[0].group_sizes] == ([737, 469, 67, 268] if kinds == "HCNO" else [804, 469, 268])


# ---------------------------------------------------------------------------------------------- 2. larger than a tile and a wave
def test_molecule_larger_than_a_tile():
    module, numbers = build(70, 3)
    e, grad, w = run_weighted(module, numbers, batch_of(70, 3, [0, 1, 2]))
    check_against_judge("N=70 B=3", e, grad, w, *judge(70, 3))


# ---------------------------------------------------------------------------------------------- 3. exact case
def test_exact_energies_from_last_layer_biases():
    """layer6 weights zero, layer6 biases 2^-1 .. 2^-4 per species, self energies zero: every energy is sum of count_s * bias_s -- exactly,
    all terms and partial sums are float32 numbers -- and every force is exactly zero."""
    from NNPOps import OptimizedTorchANI
    model = workloads.torchani_like_model(n_models=3, seed=8)
    for member in model.neural_networks:
        for k, sym in enumerate(("H", "C", "N", "O")):
            member[sym][6].weight.data.zero_()
            member[sym][6].bias.data.fill_(2.0 ** -(k + 1))
    for kinds, live_columns in PATHS:
        species, _ = molecule(23, 67, kinds)
        numbers = _numbers(species)
        want = sum(int((species == k).sum()) * 2.0 ** -(k + 1) for k in range(4))
        assert want == {"HCNO": 11 * 2.0 ** -1 + 7 * 2.0 ** -2 + 1 * 2.0 ** -3 + 4 * 2.0 ** -4, "HCO": 12 * 2.0 ** -1 + 7 * 2.0 ** -2 + 4 * 2.0 ** -4}[kinds]
        module = OptimizedTorchANI(model, numbers.cpu(), live_columns=live_columns).to(DEV)
        for batch in (5, 67):
            e, grad, _ = run_weighted(module, numbers, batch_of(23, 67, picks_of(batch)))
            assert torch.equal(e, torch.full((batch,), want, dtype=torch.float64, device=DEV)), e
            assert torch.equal(grad, torch.zeros_like(grad))


# ---------------------------------------------------------------------------------------------- 4. batch invariance, bitwise
@pytest.mark.parametrize("kinds,live_columns", PATHS, ids=PATH_IDS)
def test_batch_invariance_is_bitwise(kinds, live_columns):
    module, numbers = build(kinds=kinds, live_columns=live_columns)
    five, all67 = batch_of(23, 67, SLOTS), batch_of(23, 67, list(range(67)))
    e5, f5 = module.energy_and_forces_batch((numbers.expand(5, -1), five))
    e5b, f5b = module.energy_and_forces_batch((numbers.expand(5, -1), five))
    assert torch.equal(e5, e5b) and torch.equal(f5, f5b)                        # two calls on the same input
    e67, f67 = module.energy_and_forces_batch((numbers.expand(67, -1), all67))
    assert torch.equal(e67[SLOTS], e5) and torch.equal(f67[SLOTS], f5)          # the same conformers at slots 60, 3, 17, 41, 66 of 67
    assert not torch.equal(e67[:5], e5)


# ---------------------------------------------------------------------------------------------- 5. agreement with what exists
@pytest.mark.parametrize("kinds", ["HCNO", "HCO"])
def test_agrees_with_single_forward_and_with_the_composition(kinds):
    from NNPOps import OptimizedTorchANI
    module, numbers = build(kinds=kinds)
    coords = batch_of(23, 67, SLOTS)
    e, grad, w = run_weighted(module, numbers, coords, seed=3)
    # B separate forward calls of the same module
    for b in range(5):
        p = coords[b:b + 1].clone().requires_grad_(True)
        one = module((numbers, p)).energies
        (one * w[b]).sum().backward()
        assert abs(float(one) - float(e[b])) <= ENERGY_RTOL * abs(float(one)) + ENERGY_ATOL
        assert float((p.grad[0] - grad[b]).abs().max()) <= FORCE_RTOL * float(p.grad.abs().max())
    # the plain composition on the library GEMMs
    plain = OptimizedTorchANI(model_of(), numbers.cpu(), nn_layout="grouped", fused_step=False).to(DEV)
    assert type(plain).__name__ == "OptimizedTorchANI"
    e2, grad2, _ = run_weighted(plain, numbers, coords, seed=3)
    assert e2.dtype == torch.float64 and e2.shape == (5,)
    for b in range(5):
        assert abs(float(e2[b]) - float(e[b])) <= ENERGY_RTOL * abs(float(e2[b])) + ENERGY_ATOL
        assert float((grad2[b] - grad[b]).abs().max()) <= FORCE_RTOL * float(grad2[b].abs().max())
    # energy_and_forces_batch: the same bits, outside autograd
    p = coords.clone().requires_grad_(True)
    ea = module.forward_batch((numbers.expand(5, -1), p)).energies
    ea.sum().backward()
    eb, fb = module.energy_and_forces_batch((numbers.expand(5, -1), coords))
    assert eb.grad_fn is None and fb.grad_fn is None and fb.shape == (5, 23, 3) and eb.dtype == torch.float64
    assert torch.equal(eb, ea.detach()) and torch.equal(fb, -p.grad)


# ---------------------------------------------------------------------------------------------- 6. op level
def test_energy_batch_op_without_shift_is_float32_and_one_node():
    module, numbers = build()
    nets = module.neural_networks[0]
    coords = batch_of(23, 67, SLOTS).requires_grad_(True)
    holder = module.aev_computer.batch_holder(5)
    e = nets.fused_energy_batch(holder, coords)
    assert e.dtype == torch.float32 and e.shape == (5,)
    names, fn = [], e.grad_fn
    while fn is not None:
        names.append(fn.name())
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert len(names) == 2 and "EnergyBatchFunction" in names[0] and "AccumulateGrad" in names[1], names
    shifted = module.forward_batch((numbers.expand(5, -1), coords)).energies
    assert torch.equal(shifted.detach(), e.detach().double() + module.energy_shifter.self_energies)
    (e.float() * torch.arange(1, 6, device=DEV)).sum().backward()               # a float32 upstream gradient takes the same node
    assert coords.grad.shape == (5, 23, 3)


def test_segment_mean_entry_against_the_float64_judge():
    """Bound: the kernel adds in double and rounds once to float32 (half an ulp, 2^-24 relative); a float32 summation of n terms is
    allowed n 2^-24 of the sum of the absolute values, which is what is asserted."""
    from nnpops_amd import capi
    sizes = [23, 1, 70, 0, 64, 65, 7, 200]
    members = 3
    energies, rows, places, offsets, _ = random_grouping(sizes, 4, members, 21)
    want = segment_means(energies, places, offsets, 1.0 / members)
    t_e, t_p, t_o = (torch.tensor(a, device=DEV) for a in (energies, places, offsets))
    got = capi.mlp_energy_mean_segments(t_e, t_o, t_p, 1.0 / members)
    assert got.dtype == torch.float32 and got.shape == (len(sizes),)
    shift = torch.tensor([-1234.5678], dtype=torch.float64, device=DEV)
    got_shifted = capi.mlp_energy_mean_segments(t_e, t_o, t_p, 1.0 / members, shift)
    assert torch.equal(got_shifted, got.double() + shift)
    by_row = np.abs(energies.astype(np.float64))[places]
    for b, size in enumerate(sizes):
        mass = by_row[offsets[b]:offsets[b + 1]].sum() / members
        assert abs(float(got[b]) - want[b]) <= size * members * 2.0 ** -24 * mass, (b, float(got[b]), want[b])
    assert float(got[3]) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scale_by_segment_is_exact(dtype):
    from nnpops_amd import capi
    sizes = [23, 1, 70, 0, 64, 65, 7]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rng = np.random.default_rng(4)
    values = rng.standard_normal((int(offsets[-1]), 3)).astype(np.float32)
    factors = rng.standard_normal(len(sizes))
    t_f = torch.tensor(factors, dtype=dtype, device=DEV)
    got = capi.scale_by_segment(torch.tensor(values, device=DEV), torch.tensor(offsets, device=DEV), t_f).cpu().numpy()
    per_row = np.repeat(t_f.cpu().numpy().astype(np.float32), sizes)
    assert np.array_equal(got, values * per_row[:, None])


# ---------------------------------------------------------------------------------------------- 7. regrowth
@pytest.mark.parametrize("kinds", ["HCNO", "HCO"])
def test_first_batched_call_regrows_tiny_neighbour_buffers(kinds, monkeypatch):
    """(the re-issued step takes the means again, whichever launch they are in)"""
    monkeypatch.setenv("NNPOPS_ANI_CAP", "4")
    module, numbers = build(kinds=kinds)
    e, grad, w = run_weighted(module, numbers, batch_of(23, 67, SLOTS), seed=7)
    e_ref, g_ref = judge(23, 67, kinds)
    check_against_judge(f"regrown B=5 {kinds}", e, grad, w, e_ref[SLOTS], g_ref[SLOTS])


# ---------------------------------------------------------------------------------------------- 8. surface
@pytest.mark.parametrize("kinds", ["HCNO", "HCO"])
def test_graph_capture_and_replays(kinds):
    module, numbers = build(kinds=kinds)
    _, confs = molecule(23, 67)
    sp = numbers.expand(5, -1)
    static = batch_of(23, 67, SLOTS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            module.energy_and_forces_batch((sp, static))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_e, g_f = module.energy_and_forces_batch((sp, static))
    for k in range(3):
        with torch.no_grad():
            static.copy_(torch.tensor(confs[5 * k + 20:5 * k + 25], device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        e_ref, f_ref = module.energy_and_forces_batch((sp, static))
        assert torch.equal(g_e, e_ref) and torch.equal(g_f, f_ref)


def test_refusals():
    module, numbers = build()
    nets = module.neural_networks[0]
    sp = numbers.expand(5, -1)
    coords = batch_of(23, 67, SLOTS)
    p = coords.clone().requires_grad_(True)
    e = module.forward_batch((sp, p)).energies
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(e.sum(), p, create_graph=True)
    with pytest.raises(ValueError, match="non-periodic"):
        module.forward_batch((sp, coords), torch.eye(3, device=DEV), torch.tensor([True, True, True]))
    with pytest.raises(ValueError, match="non-periodic"):
        module.energy_and_forces_batch((sp, coords), torch.eye(3, device=DEV))
    for bad in (coords[:, :22], coords[0], coords[:0]):
        with pytest.raises(ValueError, match="positions"):
            module.forward_batch((sp, bad))
    holder, rows, sizes, places, offsets = nets._batch_plan(module.aev_computer.batch_holder(5), 5, DEV)
    op = torch.ops.NNPOpsANISymmetryFunctions.energy_batch
    args = (rows, sizes, nets.widths, nets.num_models, nets.live_planes, nets.mlp_floats)
    tail = (None, nets.x_blocks, nets.dead_blocks, nets.act_scale_log2)
    with pytest.raises(RuntimeError, match="cell is not supported"):
        op(holder, coords, torch.eye(3, device=DEV), *args, offsets, places, *tail)
    with pytest.raises(RuntimeError, match="no molecule offsets"):
        op(module.aev_computer.holder, coords, None, *args, offsets, places, *tail)
    with pytest.raises(RuntimeError, match="molecule offsets"):
        op(holder, coords, None, *args, offsets[:-1].contiguous(), places, *tail)
    with pytest.raises(RuntimeError, match="not the ones of the holder"):
        op(holder, coords, None, *args, (offsets + (offsets == 23).int()).contiguous(), places, *tail)
    with pytest.raises(RuntimeError, match="the holder"):
        op(holder, batch_of(23, 67, SLOTS[:4]), None, *args, offsets[:-1].contiguous(), places, *tail)


def test_scripting_and_the_single_molecule_path_are_untouched():
    module, numbers = build()
    coords = batch_of(23, 67, SLOTS)

    def single(m):
        p = coords[:1].clone().requires_grad_(True)
        e = m((numbers, p)).energies
        e.backward()
        return e.detach().clone(), p.grad.clone()

    e0, f0 = single(module)
    module.forward_batch((numbers.expand(5, -1), coords)).energies.sum()
    module.energy_and_forces_batch((numbers.expand(5, -1), coords))
    e1, f1 = single(module)
    assert torch.equal(e0, e1) and torch.equal(f0, f1)
    scripted = torch.jit.script(module)
    e2, f2 = single(scripted)
    assert torch.equal(e0, e2) and torch.equal(f0, f2)
    buffer = io.BytesIO()
    torch.jit.save(scripted, buffer)
    buffer.seek(0)
    e3, f3 = single(torch.jit.load(buffer, map_location=DEV))
    assert torch.equal(e0, e3) and torch.equal(f0, f3)
    # a state dict loaded into the module resets the gradient caches of its batch plans too: same numbers afterwards
    eb, fb = module.energy_and_forces_batch((numbers.expand(5, -1), coords))
    module.load_state_dict(module.state_dict())
    eb2, fb2 = module.energy_and_forces_batch((numbers.expand(5, -1), coords))
    assert torch.equal(eb, eb2) and torch.equal(fb, fb2)
