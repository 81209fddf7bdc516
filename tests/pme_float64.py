"""The float64 judges of the PME tests (no GPU code, no tests; importable anywhere): smooth PME with differentiable B-spline weights
(spme_energy), the direct sum over the op's own pairs in its two statements -- with the box as a leaf (listed_pairs_box,
direct_energy_box) and with the image shifts frozen and the exclusions included (listed_pairs_frozen, direct_energy_frozen) -- the
exact Ewald sum, the virial, the second-order driver and its comparison, and the small input builders.  Everything is pure torch /
numpy on the host; tensors that come from a device are brought over.

tests/pme_direct_reference.py is a different statement (the pair list as data, per-atom magnitudes) and stays on its own."""
import math

import numpy as np
import torch


# ---- reciprocal space -----------------------------------------------------------------------------------------------------------
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
    """0.5 sum_k w eterm |S(k)|^2 of the op (no self energy), float64 on the host, differentiable (twice) in pos, q and box: the box
    enters through B^-1 (fractional coordinates, m = B^-1 k) and det(B).  The floors are piecewise constant and detached.  moduli:
    on any device."""
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
    m = kvec @ inv.T                                                    # m = B^-1 k
    m2 = (m * m).sum(-1)
    zero = m2 == 0
    m2 = torch.where(zero, torch.ones_like(m2), m2)
    V = torch.linalg.det(box)
    mod = moduli[0].double().cpu()[:, None, None] * moduli[1].double().cpu()[None, :, None] * moduli[2].double().cpu()[None, None, :kz_n]
    eterm = torch.where(zero, torch.zeros_like(m2), torch.exp(-(math.pi / alpha) ** 2 * m2) / (math.pi * V * m2 * mod))
    kz = torch.arange(kz_n)
    w = torch.where((kz > 0) & (kz <= (K[2] - 1) // 2), 2.0, 1.0).to(torch.float64)
    return 0.5 * torch.sum(w * eterm * (S.real ** 2 + S.imag ** 2))


# ---- direct space, the box a leaf: the box gradient's judge -----------------------------------------------------------------------
def listed_pairs_box(neighbors, deltas, pos, box, exclusions):
    """(i, j, n) of the slots the direct op includes, n the integer image shift recovered in float64."""
    nb = neighbors.cpu().numpy()
    used = nb[0] >= 0
    ex = exclusions.cpu().numpy()
    excluded = {(a, b) for a in range(ex.shape[0]) for b in ex[a] if b >= 0}
    keep = np.array([u and (a, b) not in excluded for u, a, b in zip(used, nb[0], nb[1])], dtype=bool)
    i, j = nb[0][keep], nb[1][keep]
    p = pos.detach().double().cpu().numpy()
    D = p[i] - p[j] - deltas.detach().double().cpu().numpy()[keep]
    n = np.rint(D @ np.linalg.inv(box.detach().double().cpu().numpy()))
    return torch.tensor(i), torch.tensor(j), torch.tensor(n)


def direct_energy_box(pos, q, box, pairs, alpha, coulomb):
    """sum over the included pairs of coulomb q_i q_j erfc(alpha r) / r, r = |x_i - x_j - n B| (the excluded pairs' correction is
    box independent and left out)"""
    i, j, n = pairs
    d = pos[i] - pos[j] - n @ box
    r = torch.linalg.norm(d, dim=1)
    return coulomb * torch.sum(q[i] * q[j] * torch.erfc(alpha * r) / r)


# ---- direct space, the shifts frozen: the second derivatives' judge ---------------------------------------------------------------
def listed_pairs_frozen(neighbors, deltas, pos, exclusions):
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


def direct_energy_frozen(pos, q, pairs, alpha, coulomb, magnitude=False):
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


# ---- the exact Ewald sum, the virial ----------------------------------------------------------------------------------------------
def ewald_energy(pos, q, box, alpha, coulomb, images=2):
    """real-space images + full k-space + self, float64, differentiable in the box (positions fixed)"""
    inv = torch.linalg.inv(box)
    V = torch.linalg.det(box)
    mmax = 8.0 * alpha / math.pi
    bn = box.detach().numpy()
    kmax = [int(np.ceil(mmax * np.linalg.norm(bn[i]))) + 1 for i in range(3)]
    ks = np.stack(np.meshgrid(*[np.arange(-k, k + 1) for k in kmax], indexing="ij"), -1).reshape(-1, 3)
    ks = torch.tensor(ks[np.any(ks != 0, axis=1)], dtype=torch.float64)
    m = ks @ inv.T
    m2 = (m * m).sum(1)
    keep = m2.detach() <= mmax * mmax
    m, m2 = m[keep], m2[keep]
    phase = 2 * math.pi * (pos @ m.T)
    S2 = (q @ torch.cos(phase)) ** 2 + (q @ torch.sin(phase)) ** 2
    e_k = coulomb / (2 * math.pi * V) * torch.sum(torch.exp(-(math.pi / alpha) ** 2 * m2) / m2 * S2)
    # images around each pair's nearest one (atoms may lie boxes away from each other); the shifts are integer constants
    rng = torch.arange(-images, images + 1, dtype=torch.float64)
    cells = torch.stack(torch.meshgrid(rng, rng, rng, indexing="ij"), -1).reshape(-1, 3)
    x = pos[:, None, :] - pos[None, :, :]
    n0 = torch.round(x.detach() @ inv.detach())
    d = x[:, :, None, :] - (n0[:, :, None, :] + cells[None, None, :, :]) @ box
    r = torch.linalg.norm(d, dim=-1)
    same = r.detach() < 1e-12
    r = torch.where(same, torch.ones_like(r), r)
    t = torch.where(same, torch.zeros_like(r), torch.erfc(alpha * r) / r)
    e_r = 0.5 * coulomb * torch.sum(q[:, None, None] * q[None, :, None] * t)
    return e_r + e_k - coulomb * alpha / math.sqrt(math.pi) * torch.sum(q * q)


def virial(box, grad_box, pos, grad_pos):
    """W = -(B^T dE/dB + sum_j x_j (x) dE/dx_j), float64 on the host (arrays and tensors of any device)"""
    box, grad_box, pos, grad_pos = (torch.as_tensor(t).double().cpu() for t in (box, grad_box, pos, grad_pos))
    return -(box.T @ grad_box + pos.T @ grad_pos)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
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


def sorted_excl(excl):
    """an exclusion table (numpy) with every row in descending order, the -1 padding last, as the ops expect it"""
    return -np.sort(-excl.astype(np.int64), axis=1) if excl.shape[1] else excl.astype(np.int64)


def cotangents(n, seed, dtype=torch.float64):
    """(v [n, 3], w [n]) drawn in float64; another dtype: those values rounded to it"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=gen, dtype=torch.float64).to(dtype), torch.randn(n, generator=gen, dtype=torch.float64).to(dtype)


def leaves(pos, q, dtype, device="cpu"):
    x = torch.tensor(pos, dtype=dtype, device=device, requires_grad=True)
    c = torch.tensor(q, dtype=dtype, device=device, requires_grad=True)
    g = torch.tensor(0.7, dtype=dtype, device=device, requires_grad=True)
    return x, c, g


# ---- second order -----------------------------------------------------------------------------------------------------------------
def second_order(energy, x, q, g, v, w):
    """energy, first gradients of g E, and the gradients of L = sum v . d(gE)/dx + sum w d(gE)/dq with respect to x, q, g"""
    e = energy(x, q)
    P, C = torch.autograd.grad(g * e, (x, q), create_graph=True)
    L = (v * P).sum() + (w * C).sum()
    gx, gq, gg = torch.autograd.grad(L, (x, q, g))
    return e.detach(), P.detach(), C.detach(), gx, gq, gg


def rel(a, ref):
    """max|a - ref| / max|ref| in float64 on the host"""
    ref = ref.detach().double().cpu()
    return float((a.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def compare(label, op, ref, terms=0.0):
    """ties the restatement to the op by the project's existing bars -- energy 1e-5 of max(sum of the terms' magnitudes, |energy|) as
    tests/test_pme_gpu.py takes it for the direct term (signed pair terms cancel), first gradients 1e-4 of the largest component --
    then prints and returns the second-order figures"""
    assert abs(float(op[0]) - float(ref[0])) <= 1e-5 * max(terms, abs(float(ref[0]))), (label, float(op[0]), float(ref[0]))
    assert rel(op[1], ref[1]) <= 1e-4 and rel(op[2], ref[2]) <= 1e-4, (label, rel(op[1], ref[1]), rel(op[2], ref[2]))
    figures = tuple(rel(op[k], ref[k]) for k in (3, 4, 5))
    print(f"{label}: dL/dx {figures[0]:.2e}  dL/dq {figures[1]:.2e}  dL/dg {figures[2]:.2e}")
    return figures
