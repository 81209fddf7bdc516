"""Second derivatives of PME with respect to positions and charges on the MI355X: pme::pme_direct_twice, pme::pme_reciprocal_twice,
PME(..., twice_differentiable=True) and the C entries behind them against autograd of the float64 pure-torch restatement of
tests/pme_float64.py (the one tests/test_pme_second_order_cpu.py uses), against the CPU key, bit for bit between runs and against
the existing ops' first-order outputs, on both kinds of pair list, at 100 000 atoms, and through a captured graph.

Every comparison prints its figure before it asserts: max|op - ref| / max|ref| against the float64 restatement.  A bar is the worst
figure measured on the MI355X over the test's cases x 10, rounded to one digit; device against CPU key: that bar plus the CPU key's
own measured error (tests/test_pme_second_order_cpu.py).  DESIGN.md s8d lists the measurements."""
import math

import numpy as np
import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
import pme_float64 as f64
from NNPOps.neighbors import getNeighborPairs
from NNPOps.pme import PME
from nnpops_amd import capi, workloads
from nnpops_amd.pme.pme import bspline_moduli

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ALPHA, COULOMB, CUTOFF = 3.0, 138.935, 1.0

# bars: worst figure measured on the MI355X over the test's cases (in the comment) x 10, one digit
BAR_DIRECT = (4e-6, 3e-6, 5e-6)          # dL/dx, dL/dq, dL/dg: measured 3.7e-7, 2.7e-7, 4.6e-7
BAR_RECIPROCAL = (4e-5, 7e-6, 9e-5)      # measured 4.4e-6, 6.9e-7, 9.1e-6
BAR_MATCH = (4e-6, 5e-6)                 # d loss/dq, d loss/dx of the force-matching step: measured 4.5e-7, 5.1e-7
BAR_C_DIRECT = (1e-6, 2e-6)              # the C entries alone, dL/dx, dL/dq: measured 1.3e-7, 2.4e-7
BAR_C_RECIPROCAL = (2e-5, 6e-6)          # measured 1.8e-6, 6.3e-7
CPU_DIRECT = (2.5e-7, 2.7e-7, 3.8e-7)    # the CPU key's own measured errors (tests/test_pme_second_order_cpu.py)
CPU_RECIPROCAL = (2.1e-6, 6.3e-7, 3.2e-6)
BAR_NEWTON = 2e-6                        # |sum_j dL/dx_j| / largest row, direct term at 100 000 atoms: measured 2.0e-7
# A rigid translation (all v_i equal, w = 0) is annihilated EXACTLY, not to rounding: every pair's v_i - v_j, s = u . (v_i - v_j) and
# c = w_i q_j + w_j q_i are exact float zeros, so every per-slot record is zero and so is every sum.  Measured 0; the bar is 0.
BAR_TRANSLATION = (0.0, 0.0)
BAR_BILINEAR = {"direct": 3e-9, "reciprocal": 2e-8}      # |u.Hv - v.Hu| / sum |u_i (Hv)_i|: measured 3.2e-10, 1.5e-9


def device_list(pos, box, indexed):
    """the op's list on the device: from a differentiable call with a slot budget (the transposed index is built and cached) or from a
    plain call with one slot per candidate pair (-1 slots among the pairs, no index)"""
    tb = torch.tensor(box, device=DEV)
    if indexed:
        nb, dl, ds, _ = getNeighborPairs(torch.tensor(pos, device=DEV, requires_grad=True), CUTOFF, 4000, tb)
        return nb, dl.detach(), ds.detach()
    nb, dl, ds, _ = getNeighborPairs(torch.tensor(pos, device=DEV), CUTOFF, -1, tb)
    return nb, dl, ds


def direct_reference(pos, q, nb, dl, ex, v, w):
    pairs = f64.listed_pairs_frozen(nb, dl, torch.tensor(pos), ex)
    assert len(pairs[3]) > 5 and len(pairs[0]) > 100
    x, c, g = f64.leaves(pos, q, torch.float64, "cpu")
    ref = f64.second_order(lambda a, b: f64.direct_energy_frozen(a, b, pairs, ALPHA, COULOMB), x, c, g, v, w)
    return ref, float(f64.direct_energy_frozen(x.detach(), c.detach(), pairs, ALPHA, COULOMB, magnitude=True))


# ---- 7 + 9: against the restatement and the CPU key, both kinds of list ------------------------------------------------------------------
@pytest.mark.parametrize("triclinic", [False, True])
def test_direct_double_backward_on_both_kinds_of_list(triclinic):
    pos, q, box = f64.system(triclinic)
    n = len(q)
    ex = PME(8, 8, 8, 4, ALPHA, COULOMB, f64.exclusion_table(n)).exclusions
    v, w = f64.cotangents(n, 11)
    vd, wd = v.float().to(DEV), w.float().to(DEV)
    results = {}
    for kind in ("indexed", "plain", "shuffled"):
        nb, dl, ds = device_list(pos, box, kind == "indexed")
        if kind == "shuffled":                                      # of unknown origin: any order, -1 slots anywhere
            perm = torch.randperm(nb.shape[1], generator=torch.Generator().manual_seed(5)).to(DEV)
            nb, dl, ds = nb[:, perm].contiguous(), dl[perm].contiguous(), ds[perm].contiguous()
        ref, terms = direct_reference(pos, q, nb, dl, ex, v, w)
        x, c, g = f64.leaves(pos, q, torch.float32, DEV)
        exd = ex.to(DEV)
        op = f64.second_order(lambda a, b: torch.ops.pme.pme_direct_twice(a, b, nb, dl, ds, exd, ALPHA, COULOMB), x, c, g, vd, wd)
        figures = f64.compare(f"direct triclinic={triclinic} list={kind}", op, ref, terms)
        assert all(f <= bar for f, bar in zip(figures, BAR_DIRECT)), figures
        results[kind] = op
        # the CPU key on the same list
        xc, cc, gc = f64.leaves(pos, q, torch.float32, "cpu")
        host = f64.second_order(lambda a, b: torch.ops.pme.pme_direct_twice(a, b, nb.cpu(), dl.cpu(), ds.cpu(), ex, ALPHA, COULOMB), xc, cc, gc,
                            v.float(), w.float())
        for k, name in ((3, "dL/dx"), (4, "dL/dq"), (5, "dL/dg")):
            f = f64.rel(op[k], host[k])
            print(f"  device against the CPU key, {name}: {f:.2e}")
            assert f <= BAR_DIRECT[k - 3] + CPU_DIRECT[k - 3]
    # the kinds of list hold the same pairs: the same result to rounding (each within its bar of the restatement: twice the bar)
    for kind in ("plain", "shuffled"):
        for k in (3, 4, 5):
            assert f64.rel(results[kind][k], results["indexed"][k]) <= 2 * BAR_DIRECT[k - 3]


RECIPROCAL_CASES = [(False, 4, (20, 22, 18)), (True, 5, (24, 25, 21)), (True, 4, (9, 10, 11)), (False, 5, (12, 3, 14)),
                    (True, 5, (40, 36, 48))]       # (the fourth: a grid smaller than the order along y, the stencil folds)


@pytest.mark.parametrize("triclinic,order,grid", RECIPROCAL_CASES)
def test_reciprocal_double_backward_matches_the_float64_restatement_and_the_cpu_key(triclinic, order, grid):
    pos, q, box = f64.system(triclinic)
    mods = [bspline_moduli(k, order) for k in grid]
    v, w = f64.cotangents(len(q), 12)
    x, c, g = f64.leaves(pos, q, torch.float64, "cpu")
    b64 = torch.tensor(box, dtype=torch.float64)
    ref = f64.second_order(lambda a, b: f64.spme_energy(a, b, b64, grid, order, ALPHA, COULOMB, mods), x, c, g, v, w)
    x, c, g = f64.leaves(pos, q, torch.float32, DEV)
    tb = torch.tensor(box, device=DEV)
    dm = [m.to(DEV) for m in mods]
    op = f64.second_order(lambda a, b: torch.ops.pme.pme_reciprocal_twice(a, b, tb, *grid, order, ALPHA, COULOMB, *dm), x, c, g,
                      v.float().to(DEV), w.float().to(DEV))
    figures = f64.compare(f"reciprocal triclinic={triclinic} order={order} grid={grid}", op, ref)
    assert all(f <= bar for f, bar in zip(figures, BAR_RECIPROCAL)), figures
    xc, cc, gc = f64.leaves(pos, q, torch.float32, "cpu")
    host = f64.second_order(lambda a, b: torch.ops.pme.pme_reciprocal_twice(a, b, torch.tensor(box), *grid, order, ALPHA, COULOMB, *mods), xc, cc, gc,
                        v.float(), w.float())
    for k, name in ((3, "dL/dx"), (4, "dL/dq"), (5, "dL/dg")):
        f = f64.rel(op[k], host[k])
        print(f"  device against the CPU key, {name}: {f:.2e}")
        assert f <= BAR_RECIPROCAL[k - 3] + CPU_RECIPROCAL[k - 3]


def force_matching_step(pme, x, c, tb, f_ref, max_num_pairs=-1):
    e = pme.compute_direct(x, c, CUTOFF, tb, max_num_pairs) + pme.compute_reciprocal(x, c, tb)
    (dx,) = torch.autograd.grad(e, x, create_graph=True)
    loss = ((-dx - f_ref) ** 2).sum()
    loss.backward()
    return loss.detach()


def force_matching_setup():
    pos, q, box = f64.system(True, n=48, seed=7)
    n = len(q)
    grid, order = (20, 21, 22), 5
    pme = PME(*grid, order, ALPHA, COULOMB, f64.exclusion_table(n), reciprocal=True, twice_differentiable=True)
    f_ref = 50.0 * torch.randn(n, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    return pos, q, box, pme, grid, order, f_ref


def force_matching_reference(pos, q, box, pme, grid, order, f_ref):
    tb = torch.tensor(box, device=DEV)
    nb, dl, _, _ = getNeighborPairs(torch.tensor(pos, device=DEV), CUTOFF, -1, tb)
    pairs = f64.listed_pairs_frozen(nb, dl, torch.tensor(pos), pme.exclusions)
    b64 = torch.tensor(box, dtype=torch.float64)
    x = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    e = (f64.direct_energy_frozen(x, c, pairs, ALPHA, COULOMB) + f64.spme_energy(x, c, b64, grid, order, ALPHA, COULOMB, pme.moduli)
         - torch.sum(c ** 2) * (COULOMB * ALPHA / math.sqrt(math.pi)))
    (dx,) = torch.autograd.grad(e, x, create_graph=True)
    loss = ((-dx - f_ref) ** 2).sum()
    ref_q, ref_x = torch.autograd.grad(loss, (c, x))
    return float(loss.detach()), ref_q, ref_x


def test_force_matching_gradient_through_the_class():
    pos, q, box, pme, grid, order, f_ref = force_matching_setup()
    ref_loss, ref_q, ref_x = force_matching_reference(pos, q, box, pme, grid, order, f_ref)
    for max_num_pairs in (-1, 4000):                                # a list without and with the cached index
        x = torch.tensor(pos, device=DEV, requires_grad=True)
        c = torch.tensor(q, device=DEV, requires_grad=True)
        loss = force_matching_step(pme, x, c, torch.tensor(box, device=DEV), f_ref.float().to(DEV), max_num_pairs)
        assert abs(float(loss) - ref_loss) <= 1e-4 * ref_loss
        fq, fx = f64.rel(c.grad, ref_q), f64.rel(x.grad, ref_x)
        print(f"force matching, max_num_pairs={max_num_pairs}: dloss/dq {fq:.2e}  dloss/dx {fx:.2e}")
        assert fq <= BAR_MATCH[0] and fx <= BAR_MATCH[1]


# ---- 8: bit for bit ----------------------------------------------------------------------------------------------------------------
def test_double_backward_is_repeatable_and_first_order_bits_are_the_existing_ops():
    pos, q, box = f64.system(True, n=200, seed=8)
    n = len(q)
    ex = PME(8, 8, 8, 4, ALPHA, COULOMB, f64.exclusion_table(n)).exclusions.to(DEV)
    v, w = f64.cotangents(n, 13)
    vd, wd = v.float().to(DEV), w.float().to(DEV)
    tb = torch.tensor(box, device=DEV)
    grid, order = (30, 32, 28), 5
    dm = [bspline_moduli(k, order).to(DEV) for k in grid]
    for indexed in (True, False):
        nb, dl, ds = device_list(pos, box, indexed)
        runs = []
        for _ in range(2):
            x, c, g = f64.leaves(pos, q, torch.float32, DEV)
            runs.append(f64.second_order(lambda a, b: torch.ops.pme.pme_direct_twice(a, b, nb, dl, ds, ex, ALPHA, COULOMB), x, c, g, vd, wd))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        # forward and first order: the existing op's bits (with the index both take the indexed kernels, without it neither)
        out = []
        for op in (torch.ops.pme.pme_direct, torch.ops.pme.pme_direct_twice):
            x, c, _ = f64.leaves(pos, q, torch.float32, DEV)
            e = op(x, c, nb, dl, ds, ex, ALPHA, COULOMB)
            (1.3 * e).backward()
            out.append((e.detach(), x.grad, c.grad))
        for a, b in zip(*out):
            assert torch.equal(a, b)
    runs = []
    for _ in range(2):
        x, c, g = f64.leaves(pos, q, torch.float32, DEV)
        runs.append(f64.second_order(lambda a, b: torch.ops.pme.pme_reciprocal_twice(a, b, tb, *grid, order, ALPHA, COULOMB, *dm), x, c, g, vd, wd))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    out = []
    for op in (torch.ops.pme.pme_reciprocal, torch.ops.pme.pme_reciprocal_twice):
        x, c, _ = f64.leaves(pos, q, torch.float32, DEV)
        e = op(x, c, tb, *grid, order, ALPHA, COULOMB, *dm)
        (1.3 * e).backward()
        out.append((e.detach(), x.grad, c.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_saved_index_survives_a_later_pair_list():
    """the forward pass keeps the index it used: another differentiable getNeighborPairs call replaces the cache before the double
    backward runs"""
    pos, q, box = f64.system(True, n=200, seed=8)
    ex = torch.zeros(len(q), 0, dtype=torch.int32, device=DEV)
    v, w = f64.cotangents(len(q), 13)
    vd, wd = v.float().to(DEV), w.float().to(DEV)
    nb, dl, ds = device_list(pos, box, True)
    out = []
    for disturb in (False, True):
        x, c, _ = f64.leaves(pos, q, torch.float32, DEV)
        e = torch.ops.pme.pme_direct_twice(x, c, nb, dl, ds, ex, ALPHA, COULOMB)
        P, C = torch.autograd.grad(e, (x, c), create_graph=True)
        if disturb:
            other, _, _ = f64.system(False, n=77, seed=1)
            getNeighborPairs(torch.tensor(other, device=DEV, requires_grad=True), CUTOFF, 3000, torch.tensor(np.diag([2.4, 2.64, 2.16]).astype(np.float32), device=DEV))
        out.append(torch.autograd.grad((vd * P).sum() + (wd * C).sum(), (x, c)))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---- 10: the C entries alone ---------------------------------------------------------------------------------------------------------
def test_c_entries_against_float64():
    pos, q, box = f64.system(True)
    n = len(q)
    ex = PME(8, 8, 8, 4, ALPHA, COULOMB, f64.exclusion_table(n)).exclusions
    v, w = f64.cotangents(n, 14)
    tp, tq = torch.tensor(pos, device=DEV), torch.tensor(q, device=DEV)
    vd, wd = v.float().to(DEV), w.float().to(DEV)
    for indexed in (True, False):
        nb, dl, ds = device_list(pos, box, indexed)
        index = capi.neighbor_pairs_build_index(n, nb) if indexed else None
        gx, gq = capi.pme_direct_double_backward(tp, tq, nb, dl, ds, ex, vd, wd, ALPHA, COULOMB, index=index)
        ref, _ = direct_reference(pos, q, nb, dl, ex, v, w)        # (g = 0.7 multiplies the reference's outputs)
        fx, fq = f64.rel(gx * 0.7, ref[3]), f64.rel(gq * 0.7, ref[4])
        print(f"C entry direct, index given={indexed}: dL/dx {fx:.2e}  dL/dq {fq:.2e}")
        assert fx <= BAR_C_DIRECT[0] and fq <= BAR_C_DIRECT[1]
    for order, grid in ((4, (20, 22, 18)), (5, (24, 25, 21))):
        mods = [bspline_moduli(k, order) for k in grid]
        gx, gq = capi.pme_reciprocal_double_backward(tp, tq, torch.tensor(box, device=DEV), *grid, order, ALPHA, COULOMB, *mods, vd, wd)
        x, c, g = f64.leaves(pos, q, torch.float64, "cpu")
        b64 = torch.tensor(box, dtype=torch.float64)
        ref = f64.second_order(lambda a, b: f64.spme_energy(a, b, b64, grid, order, ALPHA, COULOMB, mods), x, c, g, v, w)
        fx, fq = f64.rel(gx * 0.7, ref[3]), f64.rel(gq * 0.7, ref[4])
        print(f"C entry reciprocal order={order}: dL/dx {fx:.2e}  dL/dq {fq:.2e}")
        assert fx <= BAR_C_RECIPROCAL[0] and fq <= BAR_C_RECIPROCAL[1]


# ---- 11: full size ---------------------------------------------------------------------------------------------------------------------
def test_full_size_identities_and_repeatability():
    """100 000 atoms (the benchmark's PME system and list: cutoff 5.2, alpha 0.6, 192^3, order 5).  Newton's third law and the rigid
    translation hold for the direct term alone: its pairs see positions through differences only.  The bilinear identity
    u . (H v) = v . (H u) holds for both terms; its scale is the sum of the magnitudes of the terms u_i (H v)_i, as the signed terms cancel."""
    alpha, cutoff, grid, order = 0.6, 5.2, 192, 5
    pos, _, box = workloads.random_box(100000, density=0.1, seed=6)
    n = len(pos)
    q = np.random.default_rng(6).normal(0, 0.4, n).astype(np.float32)
    tb = torch.tensor(box, device=DEV)
    x = torch.tensor(pos, device=DEV, requires_grad=True)
    c = torch.tensor(q, device=DEV, requires_grad=True)
    ex = torch.zeros(n, 0, dtype=torch.int32, device=DEV)
    nb, dl, ds, _ = getNeighborPairs(x, cutoff, 3_200_000, tb)
    dl, ds = dl.detach(), ds.detach()
    dm = [bspline_moduli(grid, order).to(DEV)] * 3
    gen = torch.Generator().manual_seed(21)
    u = (torch.randn(n, 3, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV))
    v = (torch.randn(n, 3, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV))
    shift = (torch.tensor([0.3, -1.1, 0.7], device=DEV).expand(n, 3).contiguous(), torch.zeros(n, device=DEV))
    terms = {"direct": lambda: torch.ops.pme.pme_direct_twice(x, c, nb, dl, ds, ex, alpha, COULOMB),
             "reciprocal": lambda: torch.ops.pme.pme_reciprocal_twice(x, c, tb, grid, grid, grid, order, alpha, COULOMB, *dm)}
    for name, energy in terms.items():
        P, C = torch.autograd.grad(energy(), (x, c), create_graph=True)

        def hvp(d):
            return torch.autograd.grad((d[0] * P).sum() + (d[1] * C).sum(), (x, c), retain_graph=True)
        hv, hu = hvp(v), hvp(u)
        again = hvp(v)
        assert torch.equal(hv[0], again[0]) and torch.equal(hv[1], again[1])
        assert bool(torch.isfinite(hv[0]).all()) and bool(torch.isfinite(hv[1]).all()) and float(hv[0].abs().max()) > 0
        a = float((u[0].double() * hv[0].double()).sum() + (u[1].double() * hv[1].double()).sum())
        b = float((v[0].double() * hu[0].double()).sum() + (v[1].double() * hu[1].double()).sum())
        scale = float((u[0].double() * hv[0].double()).abs().sum() + (u[1].double() * hv[1].double()).abs().sum())
        print(f"full size {name}: u.Hv {a:.6e}  v.Hu {b:.6e}  |difference| / sum of magnitudes {abs(a - b) / scale:.2e}")
        assert abs(a - b) <= BAR_BILINEAR[name] * scale
        if name == "direct":
            newton = float(hv[0].double().sum(0).abs().max()) / float(hv[0].double().norm(dim=1).max())
            ht = hvp(shift)
            fx = float(ht[0].abs().max()) / float(hv[0].abs().max())
            fq = float(ht[1].abs().max()) / float(hv[1].abs().max())
            print(f"full size direct: Newton {newton:.2e}  rigid translation dL/dx {fx:.2e}  dL/dq {fq:.2e}")
            assert newton <= BAR_NEWTON and fx <= BAR_TRANSLATION[0] and fq <= BAR_TRANSLATION[1]


# ---- 12: one captured graph of the force-loss step ----------------------------------------------------------------------------------------
def test_force_loss_step_replays_as_a_graph():
    pos, q, box, pme, _, _, f_ref = force_matching_setup()
    tb = torch.tensor(box, device=DEV)
    fr = f_ref.float().to(DEV)
    static_pos = torch.tensor(pos, device=DEV, requires_grad=True)
    static_q = torch.tensor(q, device=DEV, requires_grad=True)

    def step(x, c):
        return force_matching_step(pme, x, c, tb, fr, 4000)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                      # warm-up outside the capture
        for _ in range(2):
            step(static_pos, static_q)
            static_pos.grad = None
            static_q.grad = None
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step(static_pos, static_q)
    moved = torch.tensor(pos, device=DEV) + 0.03
    charges = torch.tensor(q, device=DEV) * 1.1
    with torch.no_grad():
        static_pos.copy_(moved)
        static_q.copy_(charges)
    graph.replay()
    torch.cuda.synchronize()
    rp, rq = moved.clone().requires_grad_(), charges.clone().requires_grad_()
    ref_loss = step(rp, rq)
    assert torch.equal(loss, ref_loss)
    assert torch.equal(static_pos.grad, rp.grad) and torch.equal(static_q.grad, rq.grad)
