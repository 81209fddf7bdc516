"""Second derivatives of PME with respect to positions and charges on the CPU key: pme::pme_direct_twice, pme::pme_reciprocal_twice
and PME(..., twice_differentiable=True) against autograd of a float64 pure-torch restatement held in this file (SPME with
differentiable B-spline weights; the direct sum over the op's own pairs with the image shifts x_i - x_j - delta frozen, exclusions
included), Hessian symmetry, a force-matching gradient, unchanged first-order bits, the refusals and TorchScript.

Every comparison prints its figure, max|op - ref| / max|ref| against the float64 restatement, before it asserts.  The bars are the
worst figure measured over the test's cases on the CPU key x 10, rounded to one digit (DESIGN.md s8d lists the measurements)."""
import math

import numpy as np
import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
from NNPOps.neighbors import getNeighborPairs
from NNPOps.pme import PME
from nnpops_amd.pme.pme import bspline_moduli

ALPHA, COULOMB, CUTOFF = 3.0, 138.935, 1.0

# bars: the worst figure measured over the test's cases on the CPU key (in the comment) x 10, one digit
BAR_DIRECT = (3e-6, 3e-6, 4e-6)          # dL/dx, dL/dq, dL/dg: measured 2.5e-7, 2.7e-7, 3.8e-7
BAR_RECIPROCAL = (2e-5, 6e-6, 3e-5)      # measured 2.1e-6, 6.3e-7, 3.2e-6
BAR_SYMMETRY = {"direct": 5e-7, "reciprocal": 3e-6}      # |H - H^T|max / |H|max: measured 4.7e-8, 2.7e-7
BAR_MATCH = (6e-6, 5e-6)                 # d loss/dq, d loss/dx of the force-matching step: measured 6.5e-7, 4.7e-7


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------
def bspline_weights(dr, order):
    """The kernels' recursion (pme_recip_spline) on float64 tensors, differentiable in dr: weight i belongs to grid point base + i."""
    w = [None] * order
    w[order - 1] = torch.zeros_like(dr)
    w[1] = dr
    w[0] = 1 - dr
    for j in range(3, order):
        div = 1.0 / (j - 1)
        w[j - 1] = div * dr * w[j - 2]
        for k in range(1, j - 1):
            w[j - k - 1] = div * ((dr + k) * w[j - k - 2] + (j - k - dr) * w[j - k - 1])
        w[0] = div * (1 - dr) * w[0]
    scale = 1.0 / (order - 1)
    w[order - 1] = scale * dr * w[order - 2]
    for j in range(1, order - 1):
        w[order - j - 1] = scale * ((dr + j) * w[order - j - 2] + (order - j - dr) * w[order - j - 1])
    w[0] = scale * (1 - dr) * w[0]
    return w


def spme_energy(pos, q, box, grid, order, alpha, coulomb, moduli):
    """0.5 sum_k w eterm |S(k)|^2 of the op (no self energy), float64, differentiable in pos and q (box: a float64 constant)."""
    K = list(grid)
    inv = torch.linalg.inv(box)
    s = pos @ inv
    u = (s - torch.floor(s.detach())) * torch.tensor(K, dtype=torch.float64)
    base = torch.floor(u.detach())
    dr = u - base
    base = base.long()
    th = [bspline_weights(dr[:, a], order) for a in range(3)]
    Q = torch.zeros(K[0] * K[1] * K[2], dtype=torch.float64)
    qs = q * math.sqrt(coulomb)
    for i in range(order):
        for j in range(order):
            for l in range(order):
                idx = (((base[:, 0] + i) % K[0]) * K[1] + (base[:, 1] + j) % K[1]) * K[2] + (base[:, 2] + l) % K[2]
                Q = Q.index_add(0, idx, qs * th[0][i] * th[1][j] * th[2][l])
    S = torch.fft.rfftn(Q.view(K[0], K[1], K[2]))
    kz_n = K[2] // 2 + 1

    def signed(k, n):
        return torch.where(k < (n + 1) // 2, k, k - n).to(torch.float64)
    mx, my, mz = signed(torch.arange(K[0]), K[0]), signed(torch.arange(K[1]), K[1]), signed(torch.arange(kz_n), K[2])
    kvec = torch.stack(torch.meshgrid(mx, my, mz, indexing="ij"), -1)
    m = kvec @ inv.T
    m2 = (m * m).sum(-1)
    zero = m2 == 0
    m2 = torch.where(zero, torch.ones_like(m2), m2)
    V = torch.linalg.det(box)
    mod = moduli[0].double()[:, None, None] * moduli[1].double()[None, :, None] * moduli[2].double()[None, None, :kz_n]
    eterm = torch.where(zero, torch.zeros_like(m2), torch.exp(-(math.pi / alpha) ** 2 * m2) / (math.pi * V * m2 * mod))
    kz = torch.arange(kz_n)
    w = torch.where((kz > 0) & (kz <= (K[2] - 1) // 2), 2.0, 1.0).to(torch.float64)
    return 0.5 * torch.sum(w * eterm * (S.real ** 2 + S.imag ** 2))


def listed_pairs(neighbors, deltas, pos, exclusions):
    """(i, j, shift) of the slots the direct op includes -- shift = x_i - x_j - delta, frozen, float64 -- and the excluded pairs (a < b)"""
    nb = neighbors.cpu().numpy()
    ex = exclusions.cpu().numpy()
    excluded = {(a, int(b)) for a in range(ex.shape[0]) for b in ex[a] if b >= 0}
    keep = np.array([a >= 0 and b >= 0 and (a, b) not in excluded for a, b in zip(nb[0], nb[1])], dtype=bool)
    i, j = torch.tensor(nb[0][keep]).long(), torch.tensor(nb[1][keep]).long()
    p = pos.detach().double().cpu()
    shift = p[i] - p[j] - deltas.detach().double().cpu()[torch.tensor(keep)]
    once = sorted((a, b) for a, b in excluded if a < b)
    ea = torch.tensor([a for a, _ in once], dtype=torch.long)
    eb = torch.tensor([b for _, b in once], dtype=torch.long)
    return i, j, shift, ea, eb


def direct_energy(pos, q, pairs, alpha, coulomb, magnitude=False):
    """sum over the included pairs of k q_i q_j erfc(alpha r) / r, r = |x_i - x_j - shift|, minus the excluded pairs' k q_i q_j erf(alpha r) / r
    on the un-wrapped difference (magnitude: the sum of the terms' absolute values, the scale of the energy's rounding error)"""
    i, j, shift, ea, eb = pairs
    size = torch.abs if magnitude else (lambda t: t)
    r = torch.linalg.norm(pos[i] - pos[j] - shift, dim=1)
    e = torch.sum(size(coulomb * q[i] * q[j] * torch.erfc(alpha * r) / r))
    if len(ea):
        r = torch.linalg.norm(pos[ea] - pos[eb], dim=1)
        e = e + torch.sum(size(-coulomb * q[ea] * q[eb] * torch.erf(alpha * r) / r))
    return e


def system(triclinic, n=40, seed=2, outside=True):
    rng = np.random.default_rng(seed)
    L = 2.4
    box = np.array([[L, 0, 0], [0.3 * L, 1.05 * L, 0], [-0.25 * L, 0.2 * L, 0.95 * L]]) if triclinic else np.diag([L, 1.1 * L, 0.9 * L])
    frac = rng.random((n, 3))
    if outside:                                                    # a third of the atoms one or two box lengths away
        frac[: n // 3] += rng.integers(-2, 3, (n // 3, 3))
    pos = frac @ box
    q = rng.normal(0, 0.5, n)
    q -= q.mean()
    return pos.astype(np.float32), q.astype(np.float32), box.astype(np.float32)


def exclusion_table(n, seed=4):
    """symmetric, rows padded with -1: a few bonded-like pairs"""
    rng = np.random.default_rng(seed)
    rows = [set() for _ in range(n)]
    for a in range(0, n - 1, 3):
        b = int(rng.integers(a + 1, n))
        rows[a].add(b)
        rows[b].add(a)
    width = max(len(r) for r in rows)
    ex = -np.ones((n, width), np.int32)
    for a, r in enumerate(rows):
        ex[a, : len(r)] = sorted(r)
    return torch.tensor(ex)


def cotangents(n, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=gen, dtype=torch.float64).to(dtype), torch.randn(n, generator=gen, dtype=torch.float64).to(dtype)


def second_order(energy, x, q, g, v, w):
    """energy, first gradients of g E, and the gradients of L = sum v . d(gE)/dx + sum w d(gE)/dq with respect to x, q, g"""
    e = energy(x, q)
    P, C = torch.autograd.grad(g * e, (x, q), create_graph=True)
    L = (v * P).sum() + (w * C).sum()
    gx, gq, gg = torch.autograd.grad(L, (x, q, g))
    return e.detach(), P.detach(), C.detach(), gx, gq, gg


def rel(a, ref):
    return float((a.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def compare(label, op, ref, terms=0.0):
    """ties the restatement to the op by the project's existing bars -- energy 1e-5 of max(sum of the terms' magnitudes, |energy|) as
    tests/test_pme_gpu.py takes it for the direct term (signed pair terms cancel), first gradients 1e-4 of the largest component --
    then returns the second-order figures"""
    assert abs(float(op[0]) - float(ref[0])) <= 1e-5 * max(terms, abs(float(ref[0]))), (label, float(op[0]), float(ref[0]))
    assert rel(op[1], ref[1]) <= 1e-4 and rel(op[2], ref[2]) <= 1e-4, (label, rel(op[1], ref[1]), rel(op[2], ref[2]))
    figures = tuple(rel(op[k], ref[k]) for k in (3, 4, 5))
    print(f"{label}: dL/dx {figures[0]:.2e}  dL/dq {figures[1]:.2e}  dL/dg {figures[2]:.2e}")
    return figures


def leaves(pos, q, dtype, device="cpu"):
    x = torch.tensor(pos, dtype=dtype, device=device, requires_grad=True)
    c = torch.tensor(q, dtype=dtype, device=device, requires_grad=True)
    g = torch.tensor(0.7, dtype=dtype, device=device, requires_grad=True)
    return x, c, g


def direct_case(triclinic, device="cpu", max_num_pairs=-1):
    pos, q, box = system(triclinic)
    n = len(q)
    ex = PME(8, 8, 8, 4, ALPHA, COULOMB, exclusion_table(n)).exclusions
    tb = torch.tensor(box, device=device)
    nb, dl, ds, _ = getNeighborPairs(torch.tensor(pos, device=device), CUTOFF, max_num_pairs, tb)
    pairs = listed_pairs(nb, dl, torch.tensor(pos), ex)
    assert len(pairs[3]) > 5 and len(pairs[0]) > 100
    v, w = cotangents(n, 11)
    x, c, g = leaves(pos, q, torch.float64)
    ref = second_order(lambda a, b: direct_energy(a, b, pairs, ALPHA, COULOMB), x, c, g, v.double(), w.double())
    terms = float(direct_energy(x.detach(), c.detach(), pairs, ALPHA, COULOMB, magnitude=True))
    return pos, q, box, ex, (nb, dl, ds), v, w, ref + (terms,)


# ---- 1 + 2: the double backward against autograd of the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("triclinic", [False, True])
def test_direct_double_backward_matches_the_float64_restatement(triclinic):
    pos, q, _, ex, (nb, dl, ds), v, w, ref = direct_case(triclinic)
    x, c, g = leaves(pos, q, torch.float32)
    op = second_order(lambda a, b: torch.ops.pme.pme_direct_twice(a, b, nb, dl, ds, ex, ALPHA, COULOMB), x, c, g, v, w)
    figures = compare(f"direct triclinic={triclinic}", op, ref, terms=ref[6])
    assert all(f <= bar for f, bar in zip(figures, BAR_DIRECT)), figures


RECIPROCAL_CASES = [(False, 4, (20, 22, 18)), (True, 5, (24, 25, 21)), (True, 6, (16, 18, 20)), (True, 4, (9, 10, 11)),
                    (False, 5, (12, 3, 14))]          # (the last: a grid smaller than the order along y, the stencil folds)


def reciprocal_case(triclinic, order, grid):
    pos, q, box = system(triclinic)
    mods = [bspline_moduli(k, order) for k in grid]
    v, w = cotangents(len(q), 12)
    x, c, g = leaves(pos, q, torch.float64)
    b64 = torch.tensor(box, dtype=torch.float64)
    ref = second_order(lambda a, b: spme_energy(a, b, b64, grid, order, ALPHA, COULOMB, mods), x, c, g, v.double(), w.double())
    return pos, q, box, mods, v, w, ref


@pytest.mark.parametrize("triclinic,order,grid", RECIPROCAL_CASES)
def test_reciprocal_double_backward_matches_the_float64_restatement(triclinic, order, grid):
    pos, q, box, mods, v, w, ref = reciprocal_case(triclinic, order, grid)
    x, c, g = leaves(pos, q, torch.float32)
    tb = torch.tensor(box)
    op = second_order(lambda a, b: torch.ops.pme.pme_reciprocal_twice(a, b, tb, *grid, order, ALPHA, COULOMB, *mods), x, c, g, v, w)
    figures = compare(f"reciprocal triclinic={triclinic} order={order} grid={grid}", op, ref)
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
    pos, q, box = system(True, n=12, seed=5)
    tb = torch.tensor(box)
    if term == "direct":
        ex = PME(8, 8, 8, 4, ALPHA, COULOMB, exclusion_table(12)).exclusions
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
    pos, q, box = system(True, n=48, seed=7)
    n = len(q)
    grid, order = (20, 21, 22), 5
    table = exclusion_table(n)
    pme = PME(*grid, order, ALPHA, COULOMB, table, reciprocal=True, twice_differentiable=True)
    gen = torch.Generator().manual_seed(3)
    f_ref = 50.0 * torch.randn(n, 3, generator=gen, dtype=torch.float64)
    tb = torch.tensor(box, device=device)
    nb, dl, _, _ = getNeighborPairs(torch.tensor(pos, device=device), CUTOFF, -1, tb)
    pairs = listed_pairs(nb, dl, torch.tensor(pos), pme.exclusions)
    b64 = torch.tensor(box, dtype=torch.float64)
    x = torch.tensor(pos, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    e = (direct_energy(x, c, pairs, ALPHA, COULOMB) + spme_energy(x, c, b64, grid, order, ALPHA, COULOMB, pme.moduli)
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
    fq, fx = rel(c.grad, ref_q), rel(x.grad, ref_x)
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
        x, c, _ = leaves(pos, q, torch.float32)
        P, C = torch.autograd.grad(energy(x, c), (x, c), create_graph=True)
        (gx,) = torch.autograd.grad((v * P).sum() + (w * C).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError, match=f"{name}: third derivatives are not implemented"):
            torch.autograd.grad(gx.sum(), c)


def test_box_gradient_and_low_order_are_refused():
    pos, q, box = system(False)
    n = len(q)
    x, c = torch.tensor(pos, requires_grad=True), torch.tensor(q)
    tb = torch.tensor(box, requires_grad=True)
    mods = [bspline_moduli(16, 4)] * 3
    with pytest.raises(RuntimeError, match="box gradients need the default ops"):
        torch.ops.pme.pme_reciprocal_twice(x, c, tb, 16, 16, 16, 4, ALPHA, COULOMB, *mods)
    with torch.no_grad():                                               # nothing is recorded: nothing to refuse
        torch.ops.pme.pme_reciprocal_twice(x, c, tb, 16, 16, 16, 4, ALPHA, COULOMB, *mods)
    pme = PME(16, 16, 16, 4, ALPHA, COULOMB, exclusion_table(n), reciprocal=True, twice_differentiable=True)
    with pytest.raises(RuntimeError, match="box gradients need the default ops"):
        pme.compute_direct(x, c, CUTOFF, tb)
    with pytest.raises(RuntimeError, match="box gradients need the default ops"):
        pme.compute_reciprocal(x, c, tb)
    mods3 = [bspline_moduli(16, 3)] * 3
    with pytest.raises(RuntimeError, match="order must be at least 4"):
        torch.ops.pme.pme_reciprocal_twice(x, c, tb.detach(), 16, 16, 16, 3, ALPHA, COULOMB, *mods3)
    with pytest.raises(TypeError):
        PME(16, 16, 16, 4, ALPHA, COULOMB, exclusion_table(n), False, True)
    # the default object still refuses second derivatives
    e = PME(16, 16, 16, 4, ALPHA, COULOMB, exclusion_table(n)).compute_direct(x, c, CUTOFF, tb.detach())
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
        x, c, g = leaves(pos, q, torch.float32)
        out.append(second_order(lambda a, b: module(a, b, nb, dl, ds, ex, tb, *mods), x, c, g, v, w))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert float(out[1][3].abs().max()) > 0 and float(out[1][4].abs().max()) > 0
