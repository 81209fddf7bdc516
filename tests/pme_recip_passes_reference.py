"""The float64 judge of every pass of reciprocal-space PME (pme_recip.hip), and the cases at which the passes' loops repeat (no GPU
code, no tests; importable anywhere).

pme_recip.hip has five loops that only repeat above a certain size: the brick prefix (pme_recip_scan: 1024 bricks per pass, with a
carry), the rank sort (pme_recip_order: 64 atoms of a brick per pass), the LDS staging of the two gathers (256 atoms of a brick's
window per pass), the capped grid-stride of the convolution and of the box gradient's Pi (1024 workgroups x 256 lanes = 262 144
complex points per pass) and the per-atom kernels' workgroups of 256 atoms.  This module holds

  * the passes restated in float64 torch on the host -- spread64, convolve64, interpolate64 -- and brick_model, which restates the
    bricks and window_bins (which bricks a brick of grid points stages, in which order);
  * the cases (CASES, SWEEP): every one is built so that one of those loops repeats;
  * spread64_by_owner and the options of spread64 / convolve64 that build one of the loops' possible defects in.

spme_energy and second_order are those of tests/pme_float64.py.  tests/test_pme_reciprocal_passes_reference_cpu.py checks this
module on the host (the passes compose to autograd of spme_energy, every case reaches its loop, the bars would see each defect);
tests/test_pme_reciprocal_passes_gpu.py compares the device's passes with it.  All functions take float64 tensors; float32 inputs
are widened exactly (case64)."""
import functools
import math

import numpy as np
import torch

from nnpops_amd.pme.pme import bspline_moduli
from pme_float64 import bspline_weights, second_order, spme_energy  # noqa: F401  (part of this module's interface)

ALPHA, COULOMB = 3.0, 138.935
BX, BY, BZ = 4, 4, 16                       # pme_recip.hip's brick of grid points
BRICK = (BX, BY, BZ)
SCAN_PASS, SORT_PASS, STAGE_PASS, CONVOLVE_PASS = 1024, 64, 256, 1024 * 256
MARGIN = 0.05                               # every atom at least this far (in cells) from a cell edge: float32 finds the same base index

# The bars of tests/test_pme_reciprocal_passes_gpu.py (max error / max reference of one pass fed with the device's own input; that
# file lists the measurements and checks that these are the same numbers).  The sensitivity tests are stated in them.
BAR_SPREAD = 2e-4
BAR_SCALED = 2e-6
BAR_CONVOLVE_ENERGY = 2e-6
BAR_INTERPOLATE = (7e-5, 1e-5)              # dE/dpositions, dE/dcharges


# ---- the passes ---------------------------------------------------------------------------------------------------------------------
def bspline_weights_and_derivatives(dr, order):
    """bspline_weights, with the derivative weights pme_recip_spline takes from the recursion one order below: dtheta[i] =
    w[i - 1] - w[i] of the order - 1 weights"""
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
    dw = [-w[0]] + [w[j - 1] - w[j] for j in range(1, order)]
    return bspline_weights(dr, order), dw


def stencil(pos, box, grid, order):
    """base index [N, 3] (long), offset inside the cell [N, 3], weights and derivative weights [3][order] of [N]: spme_energy's
    fractional coordinates"""
    K = torch.tensor(list(grid), dtype=torch.float64)
    s = pos @ torch.linalg.inv(box)
    u = (s - torch.floor(s)) * K
    base = torch.floor(u)
    dr = u - base
    both = [bspline_weights_and_derivatives(dr[:, a], order) for a in range(3)]
    return base.long(), dr, [b[0] for b in both], [b[1] for b in both]


def spread64(pos, q, box, grid, order, coulomb, keep=None):
    """Q [Kx, Ky, Kz] = sum over atoms of q sqrt(coulomb) thx thy thz at (base + i) mod K: a grid smaller than the order folds onto
    itself.  keep: a mask of the atoms that are spread (the defective restatements leave some out)."""
    K = list(grid)
    base, _, th, _ = stencil(pos, box, grid, order)
    qs = q * math.sqrt(coulomb)
    if keep is not None:
        qs = torch.where(keep, qs, torch.zeros_like(qs))
    Q = torch.zeros(K[0] * K[1] * K[2], dtype=torch.float64)
    for i in range(order):
        for j in range(order):
            for l in range(order):
                idx = (((base[:, 0] + i) % K[0]) * K[1] + (base[:, 1] + j) % K[1]) * K[2] + (base[:, 2] + l) % K[2]
                Q.index_add_(0, idx, qs * th[0][i] * th[1][j] * th[2][l])
    return Q.view(K[0], K[1], K[2])


def convolve64(S, box, grid, alpha, moduli, scaled_points=None):
    """(S eterm, 0.5 sum w eterm |S|^2) for the complex grid S [Kx, Ky, Kz/2 + 1]: the signed indices, the zero term and the weights
    w of spme_energy.  scaled_points: only the first so many points (row-major) are scaled, the rest left as they came (the
    defective restatement)."""
    K = list(grid)
    inv = torch.linalg.inv(box)
    kz_n = K[2] // 2 + 1

    def signed(k, n):
        return torch.where(k < (n + 1) // 2, k, k - n).to(torch.float64)
    mx, my, mz = signed(torch.arange(K[0]), K[0]), signed(torch.arange(K[1]), K[1]), signed(torch.arange(kz_n), K[2])
    m = torch.stack(torch.meshgrid(mx, my, mz, indexing="ij"), -1) @ inv.T
    m2 = (m * m).sum(-1)
    zero = m2 == 0
    m2 = torch.where(zero, torch.ones_like(m2), m2)
    mod = (moduli[0].double().cpu()[:, None, None] * moduli[1].double().cpu()[None, :, None]
           * moduli[2].double().cpu()[None, None, :kz_n])
    eterm = torch.where(zero, torch.zeros_like(m2), torch.exp(-(math.pi / alpha) ** 2 * m2) / (math.pi * torch.linalg.det(box) * m2 * mod))
    kz = torch.arange(kz_n)
    w = torch.where((kz > 0) & (kz <= (K[2] - 1) // 2), 2.0, 1.0).to(torch.float64)
    energy = 0.5 * torch.sum(w * eterm * (S.real ** 2 + S.imag ** 2))
    scaled = S * eterm
    if scaled_points is not None:
        scaled = torch.cat([scaled.reshape(-1)[:scaled_points], S.reshape(-1)[scaled_points:]]).view_as(S)
    return scaled, energy


def interpolate64(phi, pos, q, box, grid, order, coulomb):
    """(dE/dpositions [N, 3], dE/dcharges [N]) from the potential grid phi = irfftn(scaled complex grid, norm="forward") = dE/dQ:
    dE/dq_j = sqrt(coulomb) sum_m W_j(m) phi(m), dE/dx_j = q_j sqrt(coulomb) sum_m grad W_j(m) phi(m); along axis a the gradient of
    W_j is dtheta_a K_a times column a of B^-1."""
    K = list(grid)
    base, _, th, dth = stencil(pos, box, grid, order)
    flat = phi.reshape(-1)
    n = pos.shape[0]
    g = [torch.zeros(n, dtype=torch.float64) for _ in range(3)]
    dq = torch.zeros(n, dtype=torch.float64)
    for i in range(order):
        for j in range(order):
            for l in range(order):
                idx = (((base[:, 0] + i) % K[0]) * K[1] + (base[:, 1] + j) % K[1]) * K[2] + (base[:, 2] + l) % K[2]
                p = flat[idx]
                g[0] += dth[0][i] * th[1][j] * th[2][l] * p
                g[1] += th[0][i] * dth[1][j] * th[2][l] * p
                g[2] += th[0][i] * th[1][j] * dth[2][l] * p
                dq += th[0][i] * th[1][j] * th[2][l] * p
    inv = torch.linalg.inv(box)
    sc = math.sqrt(coulomb)
    f = torch.stack([g[a] * K[a] for a in range(3)], 1)               # dE/d(grid coordinate) without the charge
    return (q * sc)[:, None] * (f @ inv.T), dq * sc


# ---- the bricks ---------------------------------------------------------------------------------------------------------------------
def window_bins(b, B, K, nb, order):
    """window_bins of pme_recip.hip: the bricks along one axis whose cells hold the base index of an atom that reaches a point of
    brick b -- the cyclic window [b B - (order - 1), b B + B - 1] mod K in window order, every brick once, and the whole axis when
    B + order - 1 >= K.  -> (bricks, whether the window came back to a brick it already held)"""
    length = B + order - 1
    if length >= K:
        return list(range(nb)), False
    out, again = [], False
    first = (b * B - (order - 1)) % K
    for j in range(length):
        brick = ((first + j) % K) // B
        if brick in out:
            again |= brick != out[-1]
        else:
            out.append(brick)
    return out, again


class BrickModel:
    """base [N, 3] and brick [N] of every atom, counts [nbins] per brick, staged [nbins]: the atoms a brick's workgroup stages
    (the sum of the counts over its window), windows[axis][b]: window_bins."""

    def __init__(self, pos, box, grid, order):
        K = list(grid)
        self.grid, self.order = K, order
        self.nb = [-(-K[a] // BRICK[a]) for a in range(3)]
        self.nbins = self.nb[0] * self.nb[1] * self.nb[2]
        base, dr, _, _ = stencil(pos, box, grid, order)
        self.base, self.offset = base, dr
        self.brick = ((base[:, 0] // BX) * self.nb[1] + base[:, 1] // BY) * self.nb[2] + base[:, 2] // BZ
        self.counts = torch.bincount(self.brick, minlength=self.nbins)
        both = [[window_bins(b, BRICK[a], K[a], self.nb[a], order) for b in range(self.nb[a])] for a in range(3)]
        self.windows = [[w for w, _ in axis] for axis in both]
        self.comes_back = [any(again for _, again in axis) for axis in both]
        member = []
        for a in range(3):
            m = torch.zeros(self.nb[a], self.nb[a], dtype=torch.long)
            for b, w in enumerate(self.windows[a]):
                m[b, w] = 1
            member.append(m)
        c3 = self.counts.view(*self.nb)
        self.staged = torch.einsum("ai,bj,ck,ijk->abc", member[0], member[1], member[2], c3).reshape(-1)

    def staged_bricks(self, b):
        """the bricks brick b's workgroup stages, in window order: x outermost, z innermost"""
        bz, by, bx = b % self.nb[2], (b // self.nb[2]) % self.nb[1], b // (self.nb[2] * self.nb[1])
        return [(i * self.nb[1] + j) * self.nb[2] + k for i in self.windows[0][bx] for j in self.windows[1][by]
                for k in self.windows[2][bz]]


def brick_model(pos, box, grid, order):
    return BrickModel(pos, box, grid, order)


def spread64_by_owner(pos, q, box, grid, order, coulomb, model, ranges=None, stage_limit=None):
    """The spread as pme_recip_gather does it, in float64: every brick of grid points adds up the atoms it stages (the ranges of the
    bricks of its window, one after the other in window order; inside a range ascending atom index), each with the weight of every
    stencil slot i with (base + i) mod K at the point.  Without the two options it equals spread64; they build the defects in:
      ranges       (array, start [nbins + 1]): the sorted-atom array and the brick ranges to read it by, instead of the true ones
      stage_limit  only the first so many staged atoms of a window are added"""
    K = list(grid)
    _, _, th, _ = stencil(pos, box, grid, order)
    th = [torch.stack(t, 1) for t in th]                                # [N, order] per axis
    qs = q * math.sqrt(coulomb)
    if ranges is None:
        array = torch.argsort(model.brick, stable=True)                 # by brick, ascending atom index inside a brick
        start = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(model.counts, 0)])
    else:
        array, start = ranges
    start = start.tolist()
    Q = torch.zeros(K[0], K[1], K[2], dtype=torch.float64)
    slot = torch.arange(order)

    def axis_weight(points, atoms, a):
        dd = (points[None, :] - model.base[atoms, a][:, None]) % K[a]               # [atoms, points]
        hit = (slot[None, None, :] % K[a] == dd[:, :, None] % K[a]) & (slot[None, None, :] >= dd[:, :, None])
        return (hit * th[a][atoms][:, None, :]).sum(-1)

    for b in range(model.nbins):
        atoms = torch.cat([array[start[s]:max(start[s], start[s + 1])] for s in model.staged_bricks(b)])
        if stage_limit is not None:
            atoms = atoms[:stage_limit]
        bz, by, bx = b % model.nb[2], (b // model.nb[2]) % model.nb[1], b // (model.nb[2] * model.nb[1])
        px = torch.arange(bx * BX, min(bx * BX + BX, K[0]))
        py = torch.arange(by * BY, min(by * BY + BY, K[1]))
        pz = torch.arange(bz * BZ, min(bz * BZ + BZ, K[2]))
        if len(atoms) == 0:
            continue
        wx = axis_weight(px, atoms, 0) * qs[atoms][:, None]
        Q[px[0]:px[-1] + 1, py[0]:py[-1] + 1, pz[0]:pz[-1] + 1] = torch.einsum("mx,my,mz->xyz", wx, axis_weight(py, atoms, 1),
                                                                               axis_weight(pz, atoms, 2))
    return Q


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
L_BOX = 2.4
BOX = np.array([[L_BOX, 0, 0], [0.3 * L_BOX, 1.05 * L_BOX, 0], [-0.25 * L_BOX, 0.2 * L_BOX, 0.95 * L_BOX]])      # system(True)'s


def charges(rng, n):
    """N(0, 0.5), neutral, then the small ones pushed to +-0.1: one atom missing from one point stays well above the spread's bar"""
    q = rng.normal(0, 0.5, n)
    q -= q.mean()
    return np.where(np.abs(q) < 0.1, np.where(q < 0, -0.1, 0.1), q)


def place(rng, n, grid, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), outside=True):
    """positions with the grid coordinates uniform in [lo K, hi K), kept MARGIN + 0.01 cells away from the cell edges; with
    `outside` a third of the atoms one or two box lengths away (system()'s shifts)"""
    K = np.array(grid, dtype=np.float64)
    u = rng.uniform(np.array(lo) * K, np.array(hi) * K, (n, 3))
    cell = np.floor(u)
    u = cell + np.clip(u - cell, MARGIN + 0.01, 1 - MARGIN - 0.01)
    frac = u / K
    if outside:
        frac[: n // 3] += rng.integers(-2, 3, (n // 3, 3))
    return frac @ BOX


def _case(name, n, grid, order, seed, **where):
    rng = np.random.default_rng(seed)
    pos = place(rng, n, grid, **where)
    return {"name": name, "pos": pos.astype(np.float32), "q": charges(rng, n).astype(np.float32), "box": BOX.astype(np.float32),
            "grid": tuple(grid), "order": order}


ONE_BRICK = {"lo": (4 / 16, 4 / 16, 0.0), "hi": (8 / 16, 8 / 16, 16 / 32), "outside": False}      # base index inside brick (1, 1, 0)
CASES = {
    "dense-4": lambda: _case("dense-4", 3000, (12, 12, 32), 4, 101),
    "dense-5": lambda: _case("dense-5", 3000, (12, 12, 32), 5, 102),
    "blob": lambda: _case("blob", 600, (20, 24, 40), 4, 103, lo=(0.02,) * 3, hi=(0.22,) * 3, outside=False),
    "one-brick-64": lambda: _case("one-brick-64", 64, (16, 16, 32), 5, 104, **ONE_BRICK),
    "one-brick-65": lambda: _case("one-brick-65", 65, (16, 16, 32), 5, 105, **ONE_BRICK),
    "one-brick-255": lambda: _case("one-brick-255", 255, (16, 16, 32), 5, 106, **ONE_BRICK),
    "one-brick-256": lambda: _case("one-brick-256", 256, (16, 16, 32), 5, 107, **ONE_BRICK),
    "one-brick-257": lambda: _case("one-brick-257", 257, (16, 16, 32), 5, 108, **ONE_BRICK),
    "big-4": lambda: _case("big-4", 6000, (72, 68, 120), 4, 109),
    "big-5": lambda: _case("big-5", 20000, (72, 68, 120), 5, 110),
    "scan-edge": lambda: _case("scan-edge", 2000, (20, 20, 656), 4, 111),
}
CASE_NAMES = list(CASES)
COPIED_LOOP_CASES = ["dense-5", "blob", "big-5"]                      # the second-order gather and the box gradient's Pi

SWEEP_XY = list(range(1, 14))
SWEEP_Z = [1, 2, 3] + list(range(15, 24)) + [31, 32, 33, 35]
SWEEP = [(0, (k, 8, 16)) for k in SWEEP_XY] + [(1, (8, k, 16)) for k in SWEEP_XY] + [(2, (8, 8, k)) for k in SWEEP_Z]      # (axis, grid)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def sweep_case(grid, order):
    return _case(f"sweep-{order}-{grid}", 60, grid, order, 200 + 7 * sum(grid) + order)


def case64(c):
    """(pos, q, box) of a case as float64 tensors: the float32 values, widened exactly"""
    return tuple(torch.tensor(c[k]).double() for k in ("pos", "q", "box"))


def moduli(c):
    return [bspline_moduli(k, c["order"]) for k in c["grid"]]


@functools.lru_cache(maxsize=None)
def model_of(name):
    c = case(name)
    pos, _, box = case64(c)
    return brick_model(pos, box, c["grid"], c["order"])


@functools.lru_cache(maxsize=None)
def spread_of(name):
    c = case(name)
    return spread64(*case64(c), c["grid"], c["order"], COULOMB)


@functools.lru_cache(maxsize=None)
def autograd_of(name):
    """(energy, dE/dpositions, dE/dcharges, dE/dbox) by autograd of spme_energy"""
    c = case(name)
    pos, q, box = (t.requires_grad_() for t in case64(c))
    e = spme_energy(pos, q, box, c["grid"], c["order"], ALPHA, COULOMB, moduli(c))
    return (e.detach(),) + torch.autograd.grad(e, (pos, q, box))


def margin_of(model):
    """the smallest distance of an atom's grid coordinate from a cell edge, in cells"""
    return float(torch.minimum(model.offset, 1 - model.offset).min())


def smallest_atom_at_a_point(c):
    """min over the atoms of |q| sqrt(coulomb) max thx max thy max thz: the least one atom missing from one grid point takes away"""
    pos, q, box = case64(c)
    _, _, th, _ = stencil(pos, box, c["grid"], c["order"])
    peak = [torch.stack(t, 1).max(1).values for t in th]
    return float((q.abs() * math.sqrt(COULOMB) * peak[0] * peak[1] * peak[2]).min())


def window_classes(K, B, order):
    """which of the window's regimes an axis of K points is in"""
    out = set()
    if K < order:
        out.add("K < order")
    if B + order - 1 >= K:
        out.add("whole axis")
    if K == B + order:
        out.add("K = B + order")
    if K == B + order + 1:
        out.add("K = B + order + 1")
    if K in (2 * B - 1, 2 * B + 1):
        out.add(f"K = 2B {'-' if K < 2 * B else '+'} 1")
    return out


ALL_WINDOW_CLASSES = {"K < order", "whole axis", "K = B + order", "K = B + order + 1", "K = 2B - 1", "K = 2B + 1"}


def rel(a, ref):
    """max|a - ref| / max|ref| of two host tensors of one dtype, complex grids included (pme_float64.rel is for real tensors)"""
    return float((a - ref).abs().max()) / float(ref.abs().max())


def rank_in_brick(model):
    order = torch.argsort(model.brick, stable=True)
    start = torch.cumsum(model.counts, 0) - model.counts
    rank = torch.empty_like(order)
    rank[order] = torch.arange(len(order)) - start[model.brick[order]]
    return rank
