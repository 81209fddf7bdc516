"""The float64 judges of the CFConv tests (no GPU code, no tests; importable anywhere), and the frames and layers they are asked about.

`Restatement` writes the continuous-filter convolution in torch float64 on float32 inputs (widened exactly): the half list {i < j}
with every displacement as d_ij = x_j - x_i + n_ij B (B: rows = box vectors), the integer minimum-image shifts n computed ONCE
from the inputs by the reference's rule (z, then y, then x, each by the diagonal entry), the Gaussian expansion, the two dense
layers, the cosine cutoff and the symmetric accumulation.  With L = <gout, CFConv(x)> it returns the output, dL/dx, and -- from
dL/dd_ij of every pair, which autograd gives -- dL/dpos (+dL/dd on j, -dL/dd on i) and the formal derivative with the shifts
held fixed, dL/dB = sum_pairs n_ij (x) dL/dd_ij, all nine entries: what nnpops_cfconv_backprop_box returns.  It is an independent
statement of the mathematics, not a wrapper of the oracle; tests/test_cfconv_box_gradient_reference_cpu.py pins it.

`SecondOrder` restates the convolution over a FIXED pair list with frozen shifts -- the pairs and n_ij B taken once from the
Restatement -- as a differentiable function of positions, input and output gradient.  Autograd with create_graph gives the backward
pass (gx, gp) and, for cotangents V of gx and Q of gp, the gradients of M = <V, gx> + <Q, gp> with respect to (g, x, positions): what
nnpops_cfconv_double_backward returns.  `closed_form` writes the same three gradients out pair by pair;
tests/test_cfconv_second_order_reference_cpu.py pins both.
"""
import functools
import math

import numpy as np
import torch

from box_gradient_judge import moved_frames
from nnpops_amd import workloads

OUT_RTOL, OUT_ATOL_FRAC = 2e-5, 2e-6       # tests/test_cfconv_gpu.py
FORCE_RTOL = 1e-4


class Restatement:
    """CFConv in torch float64; w1 is the core-level [W][G] array, w2 is [out][in] (as nnpops_cfconv_create takes them)."""

    def __init__(self, width, n_gauss, cutoff, sigma, activation, w1, b1, w2, b2):
        self.W, self.G = int(width), int(n_gauss)
        self.cutoff, self.sigma = float(np.float32(cutoff)), float(np.float32(sigma))
        self.act = {"ssp": 0, "tanh": 1, 0: 0, 1: 1}[activation]
        wide = lambda a, shape: torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64).reshape(shape))
        self.w1, self.b1 = wide(w1, (self.W, self.G)), wide(b1, (self.W,))
        self.w2, self.b2 = wide(w2, (self.W, self.W)), wide(b2, (self.W,))
        self.mu = torch.arange(self.G, dtype=torch.float64) * self.cutoff / (self.G - 1)

    def pairs(self, pos, box):
        """-> (i, j, n) of the half list {i < j, r < cutoff}: d_ij = x_j - x_i + n_ij B, the reference's single-round minimum image
        (z, then y, then x); row by row, so that a few thousand atoms need no N x N x 3 array"""
        N = len(pos)
        out_i, out_j, out_n = [], [], []
        for i in range(N - 1):
            d = pos[i + 1:] - pos[i]
            s3 = np.round(d[:, 2] / box[2, 2]); d = d - s3[:, None] * box[2]
            s2 = np.round(d[:, 1] / box[1, 1]); d = d - s2[:, None] * box[1]
            s1 = np.round(d[:, 0] / box[0, 0]); d = d - s1[:, None] * box[0]
            keep = np.nonzero(np.einsum("ij,ij->i", d, d) < self.cutoff ** 2)[0]
            out_i.append(np.full(len(keep), i)); out_j.append(keep + i + 1)
            out_n.append(-np.stack([s1[keep], s2[keep], s3[keep]], axis=1))
        return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_n).reshape(-1, 3)

    def filters(self, d):
        """-> y2 [P][W], the filter row of every pair, from its displacement [P][3]"""
        r = d.norm(dim=1)
        gamma = torch.exp(-0.5 * ((r[:, None] - self.mu[None, :]) / self.sigma) ** 2)
        s1 = gamma @ self.w1.T + self.b1
        y1 = torch.log(0.5 * torch.exp(s1) + 0.5) if self.act == 0 else torch.tanh(s1)
        fc = 0.5 * torch.cos(math.pi * r / self.cutoff) + 0.5
        return fc[:, None] * (y1 @ self.w2.T + self.b2)

    def energy(self, pos64, box64, x, gout):
        """-> (L, pairs) at float64 positions and box (the finite differences displace the box in float64)"""
        pi, pj, pn = self.pairs(pos64, box64)
        y2 = self.filters(torch.tensor(pos64[pj] - pos64[pi] + pn @ box64))
        xin, g = torch.tensor(np.asarray(x, dtype=np.float64)), torch.tensor(np.asarray(gout, dtype=np.float64))
        return float((y2 * (xin[pj] * g[pi] + xin[pi] * g[pj])).sum()), (pi, pj, pn)

    def evaluate(self, positions, box, x, gout, chunk=16384):
        """-> dict(out, L, gx = dL/dx, g = dL/dpositions, gbox = dL/dB with the shifts held fixed, and per pair: i, j, n, d, s with
        dL/dd = s d)"""
        pos = np.asarray(positions, dtype=np.float32).astype(np.float64)
        B = np.asarray(box, dtype=np.float32).astype(np.float64).reshape(3, 3)
        pi, pj, pn = self.pairs(pos, B)
        d_all = pos[pj] - pos[pi] + pn @ B
        xin = torch.tensor(np.asarray(x, dtype=np.float32).astype(np.float64), requires_grad=True)
        g = torch.tensor(np.asarray(gout, dtype=np.float32).astype(np.float64))
        out = torch.zeros_like(g)
        gx = torch.zeros_like(g)
        dLdd = np.zeros_like(d_all)
        L = 0.0
        for lo in range(0, len(pi), chunk):
            i, j = torch.tensor(pi[lo:lo + chunk]), torch.tensor(pj[lo:lo + chunk])
            d = torch.tensor(d_all[lo:lo + chunk], requires_grad=True)
            y2 = self.filters(d)
            to_i, to_j = y2 * xin[j], y2 * xin[i]
            out.index_add_(0, i, to_i.detach()); out.index_add_(0, j, to_j.detach())
            part = (to_i * g[i]).sum() + (to_j * g[j]).sum()
            dx, dd = torch.autograd.grad(part, [xin, d])
            gx += dx
            dLdd[lo:lo + chunk] = dd.numpy()
            L += float(part.detach())
        gpos = np.zeros_like(pos)
        np.add.at(gpos, pj, dLdd)
        np.add.at(gpos, pi, -dLdd)
        r2 = np.einsum("ij,ij->i", d_all, d_all)
        return dict(out=out.numpy(), L=L, gx=gx.numpy(), g=gpos, gbox=pn.T @ dLdd, i=pi, j=pj, n=pn, d=d_all,
                    s=np.einsum("ij,ij->i", dLdd, d_all) / r2)


def recovered_shifts(pos32, box32, i, j, rec32):
    """n of every pair as image_shift (box_grad.h) recovers it in float32 from the positions, the stored displacement and the box"""
    f = np.float32
    D = ((pos32[i] - pos32[j]).astype(f) + rec32).astype(f)
    nz = np.round((D[:, 2] / box32[2, 2]).astype(f))
    ny = np.round(((D[:, 1] - (nz * box32[2, 1]).astype(f)).astype(f) / box32[1, 1]).astype(f))
    nx = np.round((((D[:, 0] - (nz * box32[2, 0]).astype(f)).astype(f) - (ny * box32[1, 0]).astype(f)).astype(f) / box32[0, 0]).astype(f))
    return np.stack([nx, ny, nz], axis=1).astype(np.float64)


# ---------------------------------------------------------------------------------------------- second derivatives
def _wide(a):
    return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))


class SecondOrder:
    """The convolution over a fixed half list (i, j) with frozen shifts [P][3] (d = x_j - x_i + shift), float64, differentiable.
    `judge` is the Restatement that holds the layer."""

    def __init__(self, judge, i, j, shift):
        self.judge = judge
        self.i, self.j = torch.as_tensor(np.asarray(i), dtype=torch.int64), torch.as_tensor(np.asarray(j), dtype=torch.int64)
        self.shift = torch.as_tensor(np.asarray(shift, dtype=np.float64))

    @classmethod
    def periodic(cls, judge, pos, box):
        """pairs and shifts of a periodic frame, by the restatement's own rule"""
        p64, b64 = np.asarray(pos, np.float32).astype(np.float64), np.asarray(box, np.float32).astype(np.float64).reshape(3, 3)
        i, j, n = judge.pairs(p64, b64)
        return cls(judge, i, j, n @ b64)

    @classmethod
    def open(cls, judge, pos):
        """pairs of a non-periodic frame: every i < j below the cutoff"""
        p = np.asarray(pos, np.float32).astype(np.float64)
        r2 = ((p[None] - p[:, None]) ** 2).sum(-1)
        i, j = np.nonzero(np.triu(r2 < judge.cutoff ** 2, 1))
        return cls(judge, i, j, np.zeros((len(i), 3)))

    def margin(self, pos):
        """smallest cutoff - r over the listed pairs"""
        d = _wide(pos)[self.j] - _wide(pos)[self.i] + self.shift
        return float((self.judge.cutoff - d.norm(dim=1)).min()) if len(self.i) else float("inf")

    def forward(self, p, x):
        d = p[self.j] - p[self.i] + self.shift
        y2 = self.judge.filters(d)
        out = torch.zeros_like(x)
        return out.index_add(0, self.i, y2 * x[self.j]).index_add(0, self.j, y2 * x[self.i])

    def first(self, pos, x, g, create_graph=False):
        """-> (out, gx, gp, leaves): leaves = (p, x, g) float64 tensors that require a gradient"""
        p, xin, gin = (_wide(a).requires_grad_(True) for a in (pos, x, g))
        out = self.forward(p, xin)
        gx, gp = torch.autograd.grad((out * gin).sum(), [xin, p], create_graph=create_graph)
        return out, gx, gp, (p, xin, gin)

    def second(self, pos, x, g, V=None, Q=None):
        """-> dict(out, gx, gp, dg, dx, dp) as float64 numpy arrays; a cotangent that is None is zero"""
        out, gx, gp, (p, xin, gin) = self.first(pos, x, g, create_graph=True)
        M = 0.0
        if V is not None:
            M = M + (_wide(V) * gx).sum()
        if Q is not None:
            M = M + (_wide(Q) * gp).sum()
        dg, dx, dp = torch.autograd.grad(M, [gin, xin, p], allow_unused=True)
        z = lambda t, like: (torch.zeros_like(like) if t is None else t).numpy()
        return dict(out=out.detach().numpy(), gx=gx.detach().numpy(), gp=gp.detach().numpy(), dg=z(dg, gin), dx=z(dx, xin), dp=z(dp, p),
                    M=float(M.detach()))


def closed_form(so, pos, x, g, V, Q):
    """dM/dg, dM/dx, dM/dpos pair by pair from the written-out derivatives (no autograd)"""
    J = so.judge
    p, xin, gin, Vt, Qt = (_wide(a) for a in (pos, x, g, V, Q))
    i, j = so.i, so.j
    d = p[j] - p[i] + so.shift
    r = d.norm(dim=1)
    u = d / r[:, None]
    t = r[:, None] - J.mu[None, :]
    s2i = 1.0 / J.sigma ** 2
    gam = torch.exp(-0.5 * t * t * s2i)
    dgam = -t * s2i * gam
    ddgam = (t * t * s2i - 1.0) * s2i * gam
    s1, ds1, dds1 = gam @ J.w1.T + J.b1, dgam @ J.w1.T, ddgam @ J.w1.T
    if J.act == 0:
        sg = torch.sigmoid(s1)
        y, a1, a2 = torch.log(0.5 * torch.exp(s1) + 0.5), sg, sg * (1.0 - sg)
    else:
        th = torch.tanh(s1)
        y, a1, a2 = th, 1.0 - th * th, -2.0 * th * (1.0 - th * th)
    dy, ddy = a1 * ds1, a2 * ds1 * ds1 + a1 * dds1
    S, dS, ddS = y @ J.w2.T + J.b2, dy @ J.w2.T, ddy @ J.w2.T
    k = math.pi / J.cutoff
    fc, dfc, ddfc = 0.5 * torch.cos(k * r) + 0.5, -0.5 * k * torch.sin(k * r), -0.5 * k * k * torch.cos(k * r)
    F = fc[:, None] * S
    F1 = dfc[:, None] * S + fc[:, None] * dS
    F2 = ddfc[:, None] * S + 2.0 * dfc[:, None] * dS + fc[:, None] * ddS
    dQ = Qt[j] - Qt[i]
    a = (u * dQ).sum(1)
    A = Vt[j] * gin[i] + Vt[i] * gin[j]
    B = xin[j] * gin[i] + xin[i] * gin[j]
    F1A, F1B, F2B = (F1 * A).sum(1), (F1 * B).sum(1), (F2 * B).sum(1)
    dg = torch.zeros_like(gin).index_add(0, i, F * Vt[j] + a[:, None] * F1 * xin[j]).index_add(0, j, F * Vt[i] + a[:, None] * F1 * xin[i])
    dx = torch.zeros_like(xin).index_add(0, i, a[:, None] * F1 * gin[j]).index_add(0, j, a[:, None] * F1 * gin[i])
    T = (F1A + a * F2B - a / r * F1B)[:, None] * u + (F1B / r)[:, None] * dQ
    dp = torch.zeros_like(p).index_add(0, i, -T).index_add(0, j, T)
    terms = dict(F1A=float(F1A.abs().max()), aF2B=float((a * F2B).abs().max()))
    return dg.numpy(), dx.numpy(), dp.numpy(), terms


# ---------------------------------------------------------------------------------------------- seeded inputs
def weights(W, G, n, seed):
    """-> (w1 [W][G], b1, w2, b2, x [n][W], gout [n][W]) float32, scaled as tests/test_cfconv_gpu.py scales them"""
    rng = np.random.default_rng(seed)
    w1 = (0.3 * rng.standard_normal((W, G))).astype(np.float32)
    w2 = (0.2 * rng.standard_normal((W, W))).astype(np.float32)
    b1 = (0.3 * rng.standard_normal(W)).astype(np.float32)
    b2 = (0.3 * rng.standard_normal(W)).astype(np.float32)
    x = rng.standard_normal((n, W)).astype(np.float32)
    gout = rng.standard_normal((n, W)).astype(np.float32)
    return w1, b1, w2, b2, x, gout


def cotangents(n, W, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, W)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def frame(tag):
    """-> (pos, box or None): the frames of the tests, built once and read-only"""
    box = None
    if tag == "triclinic350":                     # all-pairs build
        pos, _, box = workloads.triclinic_box(350, seed=52)
    elif tag == "liquid1500":                     # cell-grid build, cell-ordered walk
        pos, _, box = workloads.random_box(1500, seed=31)
    elif tag == "dense1100":                      # rows longer than a wave
        pos, _, box = workloads.random_box(1100, density=0.2, seed=71)
    elif tag == "liquid600":
        pos, _, box = workloads.random_box(600, seed=81)
    elif tag == "liquid600_shifted":              # every atom 0.37 box lengths along x: a third of them outside the box
        pos, box = frame("liquid600")
        pos = moved_frames(pos, box)[0]
    elif tag == "liquid600_wrapped":              # ... and those brought back by one box vector: other shifts, another dL/dB
        pos, box = frame("liquid600")
        pos = moved_frames(pos, box)[1]
    elif tag == "triclinic80":                    # the pinning frames: L = 9.3 and 10.0, the cutoff below half the narrowest width
        pos, _, box = workloads.triclinic_box(80, seed=5)
    elif tag == "cubic100":
        pos, _, box = workloads.random_box(100, seed=6)
    elif tag == "molecule":                       # 60 bonded atoms in vacuum and one atom 100 A away from them: an empty row
        pos, _ = workloads.conformer(60, seed=4)
        far = pos.mean(axis=0) + np.array([100.0, 0.0, 0.0])
        pos = np.concatenate([pos, far[None]]).astype(np.float32)
    else:
        raise KeyError(tag)
    for a in (pos, box):
        if a is not None:
            a.setflags(write=False)
    return pos, box


def sigma_of(G):
    return 0.1 if G >= 25 else 0.4


def layer(tag, W, G):
    """-> (w1, b1, w2, b2, x, gout) of a layer on a frame: seeded by the shape (the moved frames take those of the frame they come from)"""
    return weights(W, G, len(frame(tag)[0]), 1000 * W + G)


def handles(tag, W, G, act, cutoff, periodic=None):
    """-> (CFConvNeighbors, CFConv) of layer(tag, W, G); periodic None: the frame has a box"""
    from nnpops_amd.capi import CFConv, CFConvNeighbors
    pos, box = frame(tag)
    w1, b1, w2, b2, _, _ = layer(tag, W, G)
    if periodic is None:
        periodic = box is not None
    return (CFConvNeighbors(len(pos), cutoff, periodic),
            CFConv(len(pos), W, G, cutoff, sigma_of(G), act, w1, b1, w2, b2, periodic=periodic))
