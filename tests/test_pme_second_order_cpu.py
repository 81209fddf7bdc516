"""Second derivatives of PME with respect to positions and charges on the CPU key: pme::pme_direct_twice, pme::pme_reciprocal_twice
and PME(..., twice_differentiable=True) against autograd of the float64 pure-torch restatement of tests/pme_float64.py (SPME with
differentiable B-spline weights; the direct sum over the op's own pairs with the image shifts x_i - x_j - delta frozen, exclusions
included), Hessian symmetry, a force-matching gradient, unchanged first-order bits, the refusals and TorchScript.

Every comparison prints its figure, max|op - ref| / max|ref| against the float64 restatement, before it asserts.  The bars are the
worst figure measured over the test's cases on the CPU key x 10, rounded to one digit (DESIGN.md s8d lists the measurements)."""
import math

import numpy as np
import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
import pme_float64 as f64
from NNPOps.neighbors import getNeighborPairs
from NNPOps.pme import PME
from nnpops_amd.pme.pme import bspline_moduli

ALPHA, COULOMB, CUTOFF = 3.0, 138.935, 1.0

# bars: the worst figure measured over the test's cases on the CPU key (in the comment) x 10, one digit
BAR_DIRECT = (3e-6, 3e-6, 4e-6)          # dL/dx, dL/dq, dL/dg: measured 2.5e-7, 2.7e-7, 3.8e-7
BAR_RECIPROCAL = (2e-5, 6e-6, 3e-5)      # measured 2.1e-6, 6.3e-7, 3.2e-6
BAR_SYMMETRY = {"direct": 5e-7, "reciprocal": 3e-6}      # |H - H^T|max / |H|max: measured 4.7e-8, 2.7e-7
BAR_MATCH = (6e-6, 5e-6)                 # d loss/dq, d loss/dx of the force-matching step: measured 6.5e-7, 4.7e-7


def direct_case(triclinic, device="cpu", max_num_pairs=-1):
    pos, q, box = f64.system(triclinic)
    n = len(q)
    ex = PME(8, 8, 8, 4, ALPHA, COULOMB, f64.exclusion_table(n)).exclusions
    tb = torch.tensor(box, device=device)
    nb, dl, ds, _ = getNeighborPairs(torch.tensor(pos, device=device), CUTOFF, max_num_pairs, tb)
    pairs = f64.listed_pairs_frozen(nb, dl, torch.tensor(pos), ex)
    assert len(pairs[3]) > 5 and len(pairs[0]) > 100
    v, w = f64.cotangents(n, 11, torch.float32)
    x, c, g = f64.leaves(pos, q, torch.float64)
    ref = f64.second_order(lambda a, b: f64.direct_energy_frozen(a, b, pairs, ALPHA, COULOMB), x, c, g, v.double(), w.double())
    terms = float(f64.direct_energy_frozen(x.detach(), c.detach(), pairs, ALPHA, COULOMB, magnitude=True))
    return pos, q, box, ex, (nb, dl, ds), v, w, ref + (terms,)


# ---- 1 + 2: the double backward against autograd of the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("triclinic", [False, True])
def test_direct_double_backward_matches_the_float64_restatement(triclinic):
    pos, q, _, ex, (nb, dl, ds), v, w, ref = direct_case(triclinic)
    x, c, g = f64.leaves(pos, q, torch.float32)
    op = f64.second_order(lambda a, b: torch.ops.pme.pme_direct_twice(a, b, nb, dl, ds, ex, ALPHA, COULOMB), x, c, g, v, w)
    figures = f64.compare(f"direct triclinic={triclinic}", op, ref, terms=ref[6])
    assert all(f <= bar for f, bar in zip(figures, BAR_DIRECT)), figures


RECIPROCAL_CASES = [(False, 4, (20, 22, 18)), (True, 5, (24, 25, 21)), (True, 6, (16, 18, 20)), (True, 4, (9, 10, 11)),
                    (False, 5, (12, 3, 14))]          # (the last: a grid smaller than the order along y, the stencil folds)


def reciprocal_case(triclinic, order, grid):
    pos, q, box = f64.system(triclinic)
    mods = [bspline_moduli(k, order) for k in grid]
    v, w = f64.cotangents(len(q), 12, torch.float32)
    x, c, g = f64.leaves(pos, q, torch.float64)
    b64 = torch.tensor(box, dtype=torch.float64)
    ref = f64.second_order(lambda a, b: f64.spme_energy(a, b, b64, grid, order, ALPHA, COULOMB, mods), x, c, g, v.double(), w.double())
    return pos, q, box, mods, v, w, ref


@pytest.mark.parametrize("triclinic,order,grid", RECIPROCAL_CASES)
def test_reciprocal_double_backward_matches_the_float64_restatement(triclinic, order, grid):
    pos, q, box, mods, v, w, ref = reciprocal_case(triclinic, order, grid)
    x, c, g = f64.leaves(pos, q, torch.float32)
    tb = torch.tensor(box)
    op = f64.second_order(lambda a, b: torch.ops.pme.pme_reciprocal_twice(a, b, tb, *grid, order, ALPHA, COULOMB, *mods), x, c, g, v, w)
    figures = f64.compare(f"reciprocal triclinic={triclinic} order={order} grid={grid}", op, ref)
    assert all(f <= bar for f, bar in zip(figures, BAR_RECIPROCAL)), figures


# ---- 3: Hessian symmetry, no restatement ---------------------------------------------------------------------------------------------
def hessian(energy, pos, q):
    x = torch.tensor(pos, requires_grad=True)
    c = torch.tensor(q, requires_grad=True)
    P, C = torch.autograd.grad(energy(x, c), (x, c), create_graph=True)
    z = torch.cat([P.reshape(-1), C])
    rows = []
    for k in range(z.numel()):
        gx, gq = torch.autograd.grad(z[k], (x, c), retain_graph=True)
        rows.append(torch.cat([gx.reshape(-1), gq]))
    return torch.stack(rows).double()


@pytest.mark.parametrize("term", ["direct", "reciprocal"])
def test_hessian_is_symmetric(term):
    pos, q, box = f64.system(True, n=12, seed=5)
    tb = torch.tensor(box)
    if term == "direct":
        ex = PME(8, 8, 8, 4, ALPHA, COULOMB, f64.exclusion_table(12)).exclusions
        nb, dl, ds, _ = getNeighborPairs(torch.tensor(pos), CUTOFF, -1, tb)
        H = hessian(lambda a, b: torch.ops.pme.pme_direct_twice(a, b, nb, dl, ds, ex, ALPHA, COULOMB), pos, q)
    else:
        grid = (14, 15, 16)
        mods = [bspline_moduli(k, 5) for k in grid]
        H = hessian(lambda a, b: torch.ops.pme.pme_reciprocal_twice(a, b, tb, *grid, 5, ALPHA, COULOMB, *mods), pos, q)
    assert H.shape == (48, 48) and float(H.abs().max()) > 0
    figure = float((H - H.T).abs().max()) / float(H.abs().max())
    print(f"hessian symmetry {term}: {figure:.2e}")
    assert figure <= BAR_SYMMETRY[term]


# ---- 4: a force-matching gradient through the class -------------------------------------------------------------------------------------
def force_matching_case(device="cpu"):
    pos, q, box = f64.system(True, n=48, seed=7)
    n = len(q)
    grid, order = (20, 21, 22), 5
    table = f64.exclusion_table(n)
    pme = PME(*grid, order, ALPHA, COULOMB, table, reciprocal=True, twice_differentiable=True)
    gen = torch.Generator().manual_seed(3)
    f_ref = 50.0 * torch.randn(n, 3, generator=gen, dtype=torch.float64)
    tb = torch.tensor(box, device=device)
    nb, dl, _, _ = getNeighborPairs(torch.tensor(pos, device=device), CUTOFF, -1, tb)
    pairs = f64.listed_pairs_frozen(nb, dl, torch.tensor(pos), pme.exclusions)
    b64 = torch.tensor(box, dtype=torch.float64)
    x = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    e = (f64.direct_energy_frozen(x, c, pairs, ALPHA, COULOMB) + f64.spme_energy(x, c, b64, grid, order, ALPHA, COULOMB, pme.moduli)
         - torch.sum(c ** 2) * (COULOMB * ALPHA / math.sqrt(math.pi)))
    (dx,) = torch.autograd.grad(e, x, create_graph=True)
    loss = ((-dx - f_ref) ** 2).sum()
    ref_q, ref_x = torch.autograd.grad(loss, (c, x))
    return pos, q, box, pme, f_ref, (float(loss.detach()), ref_q, ref_x)


def force_matching_step(pme, x, c, tb, f_ref):
    e = pme.compute_direct(x, c, CUTOFF, tb) + pme.compute_reciprocal(x, c, tb)
    (dx,) = torch.autograd.grad(e, x, create_graph=True)
    loss = ((-dx - f_ref) ** 2).sum()
    loss.backward()
    return loss.detach()


def test_force_matching_gradient_through_the_class():
    pos, q, box, pme, f_ref, (ref_loss, ref_q, ref_x) = force_matching_case()
    x = torch.tensor(pos, requires_grad=True)
    c = torch.tensor(q, requires_grad=True)
    loss = force_matching_step(pme, x, c, torch.tensor(box), f_ref.float())
    assert abs(float(loss) - ref_loss) <= 1e-4 * ref_loss
    fq, fx = f64.rel(c.grad, ref_q), f64.rel(x.grad, ref_x)
    print(f"force matching: dloss/dq {fq:.2e}  dloss/dx {fx:.2e}")
    assert fq <= BAR_MATCH[0] and fx <= BAR_MATCH[1]


# ---- 5: forward and first order are the existing ops', bit for bit --------------------------------------------------------------------
def test_twice_ops_keep_the_bits_of_the_existing_ops(golden_dir):
    g = np.load(f"{golden_dir}/pme_ref.npz")
    for k in range(int(g["num_cases"])):
        c = {name[len(f"c{k}_"):]: g[name] for name in g.files if name.startswith(f"c{k}_")}
        ex, _ = torch.sort(torch.tensor(c["exclusions"]), descending=True)
        out = []
        for op in (torch.ops.pme.pme_direct, torch.ops.pme.pme_direct_twice):
            x = torch.tensor(c["positions"], requires_grad=True)
            q = torch.tensor(c["charges"], requires_grad=True)
            e = op(x, q, torch.tensor(c["neighbors"]), torch.tensor(c["deltas"]), torch.tensor(c["distances"]), ex, float(c["alpha"]),
                   float(c["coulomb"]))
            (1.3 * e).backward()
            out.append((e.detach(), x.grad, q.grad))
        for a, b in zip(*out):
            assert torch.equal(a, b)
    g = np.load(f"{golden_dir}/pme_recip_ref.npz")
    checked = 0
    for k in range(int(g["num_cases"])):
        c = {name[len(f"c{k}_"):]: g[name] for name in g.files if name.startswith(f"c{k}_")}
        if int(c["order"]) < 4:
            continue
        out = []
        for op in (torch.ops.pme.pme_reciprocal, torch.ops.pme.pme_reciprocal_twice):
            x = torch.tensor(c["positions"], requires_grad=True)
            q = torch.tensor(c["charges"], requires_grad=True)
            e = op(x, q, torch.tensor(c["box"]), *[int(s) for s in c["grid"]], int(c["order"]), float(c["alpha"]), float(c["coulomb"]),
                   torch.tensor(c["xmoduli"]), torch.tensor(c["ymoduli"]), torch.tensor(c["zmoduli"]))
            (1.3 * e).backward()
            out.append((e.detach(), x.grad, q.grad))
        for a, b in zip(*out):
            assert torch.equal(a, b)
        checked += 1
    assert checked >= 3


# ---- 6: refusals, TorchScript ----------------------------------------------------------------------------------------------------------
def test_third_derivative_is_refused():
    pos, q, box, ex, (nb, dl, ds), v, w, _ = direct_case(False)
    tb = torch.tensor(box)
    mods = [bspline_moduli(16, 4)] * 3
    for name, energy in (("pme_direct_twice", lambda a, b: torch.ops.pme.pme_direct_twice(a, b, nb, dl, ds, ex, ALPHA, COULOMB)),
                         ("pme_reciprocal_twice", lambda a, b: torch.ops.pme.pme_reciprocal_twice(a, b, tb, 16, 16, 16, 4, ALPHA, COULOMB, *mods))):
        x, c, _ = f64.leaves(pos, q, torch.float32)
        P, C = torch.autograd.grad(energy(x, c), (x, c), create_graph=True)
        (gx,) = torch.autograd.grad((v * P).sum() + (w * C).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError, match=f"{name}: third derivatives are not implemented"):
            torch.autograd.grad(gx.sum(), c)


def test_box_gradient_and_low_order_are_refused():
    pos, q, box = f64.system(False)
    n = len(q)
    x, c = torch.tensor(pos, requires_grad=True), torch.tensor(q)
    tb = torch.tensor(box, requires_grad=True)
    mods = [bspline_moduli(16, 4)] * 3
    with pytest.raises(RuntimeError, match="box gradients need the default ops"):
        torch.ops.pme.pme_reciprocal_twice(x, c, tb, 16, 16, 16, 4, ALPHA, COULOMB, *mods)
    with torch.no_grad():                                               # nothing is recorded: nothing to refuse
        torch.ops.pme.pme_reciprocal_twice(x, c, tb, 16, 16, 16, 4, ALPHA, COULOMB, *mods)
    pme = PME(16, 16, 16, 4, ALPHA, COULOMB, f64.exclusion_table(n), reciprocal=True, twice_differentiable=True)
    with pytest.raises(RuntimeError, match="box gradients need the default ops"):
        pme.compute_direct(x, c, CUTOFF, tb)
    with pytest.raises(RuntimeError, match="box gradients need the default ops"):
        pme.compute_reciprocal(x, c, tb)
    mods3 = [bspline_moduli(16, 3)] * 3
    with pytest.raises(RuntimeError, match="order must be at least 4"):
        torch.ops.pme.pme_reciprocal_twice(x, c, tb.detach(), 16, 16, 16, 3, ALPHA, COULOMB, *mods3)
    with pytest.raises(TypeError):
        PME(16, 16, 16, 4, ALPHA, COULOMB, f64.exclusion_table(n), False, True)
    # the default object still refuses second derivatives
    e = PME(16, 16, 16, 4, ALPHA, COULOMB, f64.exclusion_table(n)).compute_direct(x, c, CUTOFF, tb.detach())
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(e, x, create_graph=True)


class BothTerms(torch.nn.Module):
    def forward(self, pos, q, nb, d, r, ex, box, xm, ym, zm):
        return (torch.ops.pme.pme_direct_twice(pos, q, nb, d, r, ex, 3.0, 138.935) +
                torch.ops.pme.pme_reciprocal_twice(pos, q, box, 20, 22, 18, 4, 3.0, 138.935, xm, ym, zm))


def test_torchscript_module_with_a_double_backward():
    pos, q, box, ex, (nb, dl, ds), v, w, _ = direct_case(False)
    mods = [bspline_moduli(k, 4) for k in (20, 22, 18)]
    tb = torch.tensor(box)
    scripted = torch.jit.script(BothTerms())
    out = []
    for module in (BothTerms(), scripted):
        x, c, g = f64.leaves(pos, q, torch.float32)
        out.append(f64.second_order(lambda a, b: module(a, b, nb, dl, ds, ex, tb, *mods), x, c, g, v, w))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert float(out[1][3].abs().max()) > 0 and float(out[1][4].abs().max()) > 0
