"""Box-vector gradients of PME on the MI355X: pme::pme_direct_box and the box gradient of pme::pme_reciprocal against autograd of the
float64 pure-torch restatement of tests/pme_float64.py and of its independent Ewald sum, the CPU key, virial symmetry (up to config 5's 100 000 atoms), the
indexed direct path, bitwise repeatability and unchanged outputs, graph capture on a box written in place, and create_graph."""
import numpy as np
import pytest
import torch
from torch.profiler import ProfilerActivity, profile

import NNPOps  # noqa: F401  (loads the torch ops)
import pme_float64 as f64
from NNPOps.neighbors import getNeighborPairs
from NNPOps.pme import PME
from nnpops_amd import workloads
from nnpops_amd.pme.pme import bspline_moduli

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA, COULOMB, CUTOFF = 3.0, 138.935, 1.0


def direct_step(pos, q, box, ex, device=DEV, max_num_pairs=-1, cutoff=CUTOFF, alpha=ALPHA):
    """compute_direct with everything requiring grad -> (energy, dE/dx, dE/dq, dE/dB)"""
    pme = PME(16, 16, 16, 5, alpha, COULOMB, ex)
    tp = torch.tensor(pos, device=device, requires_grad=True)
    tq = torch.tensor(q, device=device, requires_grad=True)
    tb = torch.tensor(box, device=device, requires_grad=True)
    e = pme.compute_direct(tp, tq, cutoff, tb, max_num_pairs)
    return (e.detach(),) + torch.autograd.grad(e, (tp, tq, tb))


def recip_step(pos, q, box, grid, order, device=DEV, alpha=ALPHA, box_grad=True):
    mods = [bspline_moduli(k, order).to(device) for k in grid]
    tp = torch.tensor(pos, device=device, requires_grad=True)
    tq = torch.tensor(q, device=device, requires_grad=True)
    tb = torch.tensor(box, device=device, requires_grad=box_grad)
    e = torch.ops.pme.pme_reciprocal(tp, tq, tb, *grid, order, alpha, COULOMB, *mods)
    return (e.detach(),) + torch.autograd.grad(e, (tp, tq, tb) if box_grad else (tp, tq))


@pytest.mark.parametrize("triclinic", [False, True])
def test_direct_box_gradient_matches_the_float64_restatement(triclinic):
    pos, q, box = f64.system(triclinic)
    ex = f64.exclusion_table(len(q))
    gb = direct_step(pos, q, box, ex)[3]
    assert gb.dtype == torch.float32 and gb.device.type == "cuda"
    tb32 = torch.tensor(box)
    neighbors, deltas, _, _ = getNeighborPairs(torch.tensor(pos), CUTOFF, -1, tb32)
    pairs = f64.listed_pairs_box(neighbors, deltas, torch.tensor(pos), tb32, ex)
    assert int((pairs[2] != 0).any(dim=1).sum()) > 10
    b64 = torch.tensor(box, dtype=torch.float64, requires_grad=True)
    e = f64.direct_energy_box(torch.tensor(pos, dtype=torch.float64), torch.tensor(q, dtype=torch.float64), b64, pairs, ALPHA, COULOMB)
    (ref,) = torch.autograd.grad(e, b64)
    # (measured on an MI355X: at most 8.9e-7 of the largest entry)
    torch.testing.assert_close(gb.double().cpu(), ref, rtol=0, atol=1e-5 * float(ref.abs().max()))


@pytest.mark.parametrize("triclinic,order,grid", [(False, 4, (20, 22, 18)), (True, 5, (24, 25, 21)), (True, 4, (9, 10, 11))])
def test_reciprocal_box_gradient_matches_the_float64_restatement(triclinic, order, grid):
    pos, q, box = f64.system(triclinic)
    e, gp, _, gb = recip_step(pos, q, box, grid, order)
    mods = [bspline_moduli(k, order) for k in grid]
    b64 = torch.tensor(box, dtype=torch.float64, requires_grad=True)
    e64 = f64.spme_energy(torch.tensor(pos, dtype=torch.float64), torch.tensor(q, dtype=torch.float64), b64, grid, order, ALPHA, COULOMB, mods)
    (ref,) = torch.autograd.grad(e64, b64)
    assert abs(float(e) - float(e64)) <= 1e-5 * abs(float(e64))
    # (measured on an MI355X: at most 2.3e-6 of the largest entry, the cubic order-4 case)
    torch.testing.assert_close(gb.double().cpu(), ref, rtol=0, atol=2e-5 * float(ref.abs().max()))


def test_device_matches_the_cpu_key():
    pos, q, box = f64.system(True, n=300, seed=12)
    ex = f64.exclusion_table(len(q))
    for fn in (lambda d: direct_step(pos, q, box, ex, device=d), lambda d: recip_step(pos, q, box, (24, 24, 24), 5, device=d)):
        host, dev = fn("cpu"), fn(DEV)
        for h, d in zip(host[1:], dev[1:]):              # (measured: at most 1.1e-6 of the largest entry)
            torch.testing.assert_close(d.cpu(), h, rtol=0, atol=1e-5 * float(h.abs().max()))


def test_total_box_gradient_converges_to_the_ewald_sum():
    pos, q, box = f64.system(True, n=24, seed=3, outside=True)
    alpha = 4.0
    b64 = torch.tensor(box, dtype=torch.float64, requires_grad=True)
    (ref,) = torch.autograd.grad(f64.ewald_energy(torch.tensor(pos, dtype=torch.float64), torch.tensor(q, dtype=torch.float64), b64,
                                                  alpha, COULOMB), b64)
    errs = []
    for grid in (12, 24, 48):
        pme = PME(grid, grid, grid, 5, alpha, COULOMB, torch.zeros(len(q), 0, dtype=torch.int32), reciprocal=True)
        tb = torch.tensor(box, device=DEV, requires_grad=True)
        tp, tq = torch.tensor(pos, device=DEV), torch.tensor(q, device=DEV)
        e = pme.compute_direct(tp, tq, 0.95, tb) + pme.compute_reciprocal(tp, tq, tb)
        (g,) = torch.autograd.grad(e, tb)
        errs.append(float((g.double().cpu() - ref).abs().max()) / float(ref.abs().max()))
    # (measured on an MI355X: 1.7e-1, 2.3e-3, 1.1e-4 -- the grid's discretisation error, deterministic; 1.5e-5 at 64^3)
    assert errs[0] > errs[1] > errs[2] and errs[2] < 2e-4, errs


def test_virial_is_symmetric_small_and_at_100k_atoms():
    pos, q, box = f64.system(True, n=200, seed=9)
    ex = f64.exclusion_table(len(q))
    # (asymmetry measured on an MI355X, relative to the largest entry: 9.0e-7 direct and 4.1e-7 reciprocal at 200 atoms, 2.1e-6
    #  and 1.6e-8 at 100 000)
    _, gp, _, gb = direct_step(pos, q, box, ex)
    W = f64.virial(box, gb, pos, gp)
    assert float((W - W.T).abs().max()) <= 1e-5 * float(W.abs().max()), W
    _, gp, _, gb = recip_step(pos, q, box, (32, 32, 32), 5)
    W = f64.virial(box, gb, pos, gp)
    assert float((W - W.T).abs().max()) <= 1e-5 * float(W.abs().max()), W
    # config 5: 100 000 atoms, cutoff 5.2, a 3.2 M-slot list (indexed path), reciprocal at 192^3, order 5
    pos, _, box = workloads.random_box(100000, density=0.1, seed=6)
    q = np.random.default_rng(6).normal(0, 0.4, len(pos)).astype(np.float32)
    q -= q.mean()
    ex = torch.zeros(len(pos), 0, dtype=torch.int32)
    _, gp, _, gb = direct_step(pos, q, box, ex, max_num_pairs=3_200_000, cutoff=5.2, alpha=0.6)
    W = f64.virial(box, gb, pos, gp)
    assert float((W - W.T).abs().max()) <= 2e-5 * float(W.abs().max()), W
    _, gp, _, gb = recip_step(pos, q, box, (192, 192, 192), 5, alpha=0.6)
    W = f64.virial(box, gb, pos, gp)
    assert float((W - W.T).abs().max()) <= 2e-5 * float(W.abs().max()), W


def test_indexed_direct_path_matches_the_plain_path():
    pos, _, box = workloads.random_box(20000, density=0.1, seed=3)
    q = np.random.default_rng(3).normal(0, 0.4, len(pos)).astype(np.float32)
    ex = f64.exclusion_table(len(pos))
    from nnpops_amd import capi
    exs = PME(16, 16, 16, 5, 0.6, COULOMB, ex).exclusions.to(DEV)
    out = []
    for plain in (False, True):
        tp = torch.tensor(pos, device=DEV, requires_grad=True)
        tq = torch.tensor(q, device=DEV, requires_grad=True)
        tb = torch.tensor(box, device=DEV, requires_grad=True)
        # positions that require grad: getNeighborPairs builds the transposed index and leaves it in the pair-index cache
        nb, d, r, found = getNeighborPairs(tp, 5.0, 700_000, tb.detach())
        assert 0 < int(found) < 700_000
        if plain:                                           # a copy is not the list the pair-index cache knows: the atomic path
            nb = nb.clone()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            e = torch.ops.pme.pme_direct_box(tp, tq, nb, d.detach(), r.detach(), exs, tb, 0.6, COULOMB)
            torch.cuda.synchronize()
        kernels = " ".join(ev.key for ev in prof.key_averages())
        # which path it took: the indexed kernels or the atomic ones (both round to the same float32 bits almost everywhere)
        assert ("pme_direct_gather_indexed" in kernels) != plain and ("pme_direct_pairs" in kernels) == plain, (plain, kernels)
        assert "pme_direct_box_partials" in kernels
        out.append((e.detach(),) + torch.autograd.grad(e, (tp, tq, tb)))
        # and bit for bit what the C ABI's indexed entry (an index built afresh) or its plain one gives
        index = capi.neighbor_pairs_build_index(len(pos), nb) if not plain else None
        ce, cp, cq = capi.pme_direct(tp.detach(), tq.detach(), nb, d.detach(), r.detach(), exs, 0.6, COULOMB, index=index)
        torch.cuda.synchronize()
        assert torch.equal(out[-1][0].reshape(1), ce) and torch.equal(out[-1][1], cp) and torch.equal(out[-1][2], cq), plain
    (e0, p0, q0, b0), (e1, p1, q1, b1) = out
    assert torch.equal(b0, b1)                              # the box pass reads the list only: the same on both
    assert abs(float(e0) - float(e1)) <= 1e-6 * abs(float(e0))
    torch.testing.assert_close(p1, p0, rtol=0, atol=1e-5 * float(p0.abs().max()))
    torch.testing.assert_close(q1, q0, rtol=0, atol=1e-5 * float(q0.abs().max()))


def test_bitwise_repeatable_and_outputs_unchanged():
    pos, q, box = f64.system(True, n=300, seed=5)
    ex = f64.exclusion_table(len(q))
    pme = PME(24, 24, 24, 5, ALPHA, COULOMB, ex, reciprocal=True)
    runs = []
    for box_grad in (False, True, True):
        tp = torch.tensor(pos, device=DEV, requires_grad=True)
        tq = torch.tensor(q, device=DEV, requires_grad=True)
        tb = torch.tensor(box, device=DEV, requires_grad=box_grad)
        ed = pme.compute_direct(tp, tq, CUTOFF, tb, 30000)
        er = pme.compute_reciprocal(tp, tq, tb)
        wrt = (tp, tq, tb) if box_grad else (tp, tq)
        runs.append([ed.detach(), er.detach()] + list(torch.autograd.grad(ed, wrt)) + list(torch.autograd.grad(er, wrt)))
    plain, first, second = runs
    for a, b in zip(first, second):                            # box gradients included
        assert torch.equal(a, b)
    same = [first[i] for i in (0, 1, 2, 3, 5, 6)]              # energies, dE/dx, dE/dq without the box entries
    for a, b in zip(plain, same):
        assert torch.equal(a, b)


def test_graph_capture_follows_a_box_written_in_place():
    pos, q, box = f64.system(True, n=120, seed=7, outside=False)
    pme = PME(24, 24, 24, 5, ALPHA, COULOMB, f64.exclusion_table(len(q)), reciprocal=True)
    tq = torch.tensor(q, device=DEV)
    static_pos = torch.tensor(pos, device=DEV, requires_grad=True)
    static_box = torch.tensor(box, device=DEV, requires_grad=True)

    def step():
        e = pme.compute_direct(static_pos, tq, CUTOFF, static_box, 4000) + pme.compute_reciprocal(static_pos, tq, static_box)
        e.backward()
        return e

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
            static_pos.grad = None
            static_box.grad = None
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e = step()
    new_box = torch.tensor(box, device=DEV) * 1.03
    with torch.no_grad():
        static_box.copy_(new_box)
    graph.replay()
    torch.cuda.synchronize()
    rp = torch.tensor(pos, device=DEV, requires_grad=True)
    rb = new_box.clone().requires_grad_()
    e_ref = pme.compute_direct(rp, tq, CUTOFF, rb, 4000) + pme.compute_reciprocal(rp, tq, rb)
    e_ref.backward()
    assert torch.allclose(e, e_ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(static_pos.grad, rp.grad, rtol=0, atol=1e-5 * float(rp.grad.abs().max()))
    torch.testing.assert_close(static_box.grad, rb.grad, rtol=0, atol=1e-5 * float(rb.grad.abs().max()))


def test_create_graph_is_refused_with_the_box():
    pos, q, box = f64.system(False)
    pme = PME(16, 16, 16, 4, ALPHA, COULOMB, f64.exclusion_table(len(q)), reciprocal=True)
    for term in ("direct", "reciprocal"):
        tp = torch.tensor(pos, device=DEV, requires_grad=True)
        tb = torch.tensor(box, device=DEV, requires_grad=True)
        tq = torch.tensor(q, device=DEV)
        e = pme.compute_direct(tp, tq, CUTOFF, tb) if term == "direct" else pme.compute_reciprocal(tp, tq, tb)
        with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
            torch.autograd.grad(e, (tp, tb), create_graph=True)


def test_c_abi_box_gradients():
    from nnpops_amd import capi
    pos, q, box = f64.system(True, n=300, seed=8)
    ex = f64.exclusion_table(len(q))
    exs = PME(8, 8, 8, 4, ALPHA, COULOMB, ex).exclusions.to(DEV)
    tp, tq, tb = (torch.tensor(a, device=DEV) for a in (pos, q, box))
    nb, d, r, _ = getNeighborPairs(tp, CUTOFF, -1, tb)
    gb = capi.pme_direct_box(tp, tq, nb, d, r, exs, tb, ALPHA, COULOMB)
    ref = direct_step(pos, q, box, ex)[3]
    assert torch.equal(gb, ref)
    grid = (20, 24, 28)
    mods = [bspline_moduli(k, 5).to(DEV) for k in grid]
    e, pd, cd, gb = capi.pme_reciprocal_box(tp, tq, tb, *grid, 5, ALPHA, COULOMB, *mods)
    e0, pd0, cd0 = capi.pme_reciprocal(tp, tq, tb, *grid, 5, ALPHA, COULOMB, *mods)
    torch.cuda.synchronize()
    assert torch.equal(e, e0) and torch.equal(pd, pd0) and torch.equal(cd, cd0)
    assert torch.equal(gb, recip_step(pos, q, box, grid, 5)[3])
