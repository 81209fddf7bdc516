"""The float64 restatement of the periodic CFConv that the box-gradient tests compare against, and what pins it (CPU only).

`Restatement` writes the continuous-filter convolution in torch float64 on float32 inputs (widened exactly): the half list {i < j}
with every displacement as d_ij = x_j - x_i + n_ij B (B: rows = box vectors), the integer minimum-image shifts n computed ONCE
from the inputs by the reference's rule (z, then y, then x, each by the diagonal entry), the Gaussian expansion, the two dense
layers, the cosine cutoff and the symmetric accumulation.  With L = <gout, CFConv(x)> it returns the output, dL/dx, and -- from
dL/dd_ij of every pair, which autograd gives -- dL/dpos (+dL/dd on j, -dL/dd on i) and the formal derivative with the shifts
held fixed, dL/dB = sum_pairs n_ij (x) dL/dd_ij, all nine entries: what nnpops_cfconv_backprop_box returns.  It is an independent
statement of the mathematics, not a wrapper of the oracle; tests/test_cfconv_box_gradient_gpu.py loads it from this file.

What pins it:
    output, dL/dx, dL/dpos   against the float32 CFConvOracle at the tolerances of tests/test_cfconv_gpu.py (the oracle is the float32
        party here: 2e-5 relative + 2e-6 of the largest entry on output and input gradient, 1e-4 of the largest force).
    dL/dB, all nine entries  against central differences of the restatement's own L in the box entry, positions held fixed and the
        shifts RECOMPUTED at every displaced box, Richardson-extrapolated from the steps h = 2^-14 and 2^-15.  The cosine cutoff
        keeps L continuous when a pair enters or leaves, but its second derivative jumps there, which a difference quotient sees
        and no extrapolation removes -- so the test asserts that the pair list and the shifts at every displaced box are those of
        the undisplaced one (the frames are chosen so; nothing about the code under test enters that choice).  What is left:
        truncation of order h^4, rounding eps |L| / h ~ 1e-16 * 1e2 / 3e-5 ~ 3e-10 absolute.  Bar: 1e-6 of the largest entry, two
        orders below the 1e-4 gate of the GPU tests.
What it also measures (printed, pytest -s): the kernel's formula on float32 records -- float64 products of the float64 pair scalars
    with float32-rounded displacements, the shifts recovered the way image_shift does (three float32 roundings per axis).  The
    recovered shifts are asserted to be the builder's exactly; the distance of that figure from the full float64 value is printed
    (2e-8 ... 3e-8 of the largest entry), and again with 1e-5 of independent relative noise on every pair scalar (8e-6 ... 3e-5):
    the 1e-4 bar of the GPU tests leaves room for the float32 filter arithmetic behind the pair scalars.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from nnpops_amd import workloads
from oracle import CFConvNeighborsOracle, CFConvOracle

OUT_RTOL, OUT_ATOL_FRAC = 2e-5, 2e-6       # tests/test_cfconv_gpu.py
FORCE_RTOL = 1e-4
FD_RTOL = 1e-6


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


def frame(tag):
    """-> (pos, box): the frames of the GPU tests"""
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
        pos = (pos + np.array([0.37 * float(box[0, 0]), 0, 0], dtype=np.float32)).astype(np.float32)
        assert 0.25 < float((pos[:, 0] > box[0, 0]).mean()) < 0.45
    elif tag == "liquid600_wrapped":              # ... and those brought back by one box vector: other shifts, another dL/dB
        pos, box = frame("liquid600_shifted")
        pos = (pos - (pos[:, :1] > box[0, 0]) * box[0]).astype(np.float32)
    elif tag == "triclinic80":                    # the pinning frames: L = 9.3 and 10.0, the cutoff below half the narrowest width
        pos, _, box = workloads.triclinic_box(80, seed=5)
    elif tag == "cubic100":
        pos, _, box = workloads.random_box(100, seed=6)
    else:
        raise KeyError(tag)
    return pos, box


# ---------------------------------------------------------------------------------------------- the pinning tests
PIN_CASES = [("triclinic80", 8, 6, 4.0, 0.5, "ssp"), ("cubic100", 12, 9, 4.5, 0.4, "tanh")]
PIN_IDS = [c[0] + "-" + c[5] for c in PIN_CASES]


@pytest.mark.parametrize("tag,W,G,cutoff,sigma,act", PIN_CASES, ids=PIN_IDS)
def test_restatement_is_the_oracle(tag, W, G, cutoff, sigma, act):
    pos, box = frame(tag)
    n = len(pos)
    w1, b1, w2, b2, x, gy = weights(W, G, n, 17)
    onb = CFConvNeighborsOracle(n, cutoff, True)
    onb.build(pos, box)
    ocf = CFConvOracle(n, W, G, cutoff, sigma, act, w1, b1, w2, b2, periodic=True)
    y_ref = ocf.forward(onb, pos, x, box)
    xg_ref, pg_ref = ocf.backward(onb, pos, x, gy, box)
    out = Restatement(W, G, cutoff, sigma, act, w1, b1, w2, b2).evaluate(pos, box, x, gy)
    start, other, _ = onb.export()
    assert np.array_equal(np.repeat(np.arange(n), np.diff(start)), out["i"]) and np.array_equal(other, out["j"])      # the same half list
    assert np.abs(out["n"]).max() == 1 and np.abs(out["gbox"]).max() > 0                                              # wrapped pairs exist
    np.testing.assert_allclose(y_ref, out["out"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(out["out"]).max())
    np.testing.assert_allclose(xg_ref, out["gx"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(out["gx"]).max())
    err = np.abs(pg_ref - out["g"]).max() / np.abs(out["g"]).max()
    print(f"\n[cfconv-box-reference] {tag} {act}: oracle position gradient {err:.2e} of max")
    assert err <= FORCE_RTOL


@pytest.mark.parametrize("tag,W,G,cutoff,sigma,act", PIN_CASES, ids=PIN_IDS)
def test_box_gradient_against_finite_differences(tag, W, G, cutoff, sigma, act):
    pos, box = frame(tag)
    w1, b1, w2, b2, x, gy = weights(W, G, len(pos), 17)
    judge = Restatement(W, G, cutoff, sigma, act, w1, b1, w2, b2)
    base = judge.evaluate(pos, box, x, gy)
    pos64, box64 = pos.astype(np.float64), box.astype(np.float64)

    def energy(b):
        L, (pi, pj, pn) = judge.energy(pos64, b, x, gy)
        assert np.array_equal(pi, base["i"]) and np.array_equal(pj, base["j"]) and np.array_equal(pn, base["n"]), \
            "a pair crosses the cutoff (or changes its image) inside the finite-difference step"
        return L

    worst, top = 0.0, np.abs(base["gbox"]).max()
    for k in range(3):
        for c in range(3):
            def central(h):
                plus, minus = box64.copy(), box64.copy()
                plus[k, c] += h; minus[k, c] -= h
                return (energy(plus) - energy(minus)) / (2 * h)
            fd = (4.0 * central(2.0 ** -15) - central(2.0 ** -14)) / 3.0
            worst = max(worst, abs(fd - base["gbox"][k, c]))
    smallest = np.abs(base["gbox"]).min()
    print(f"\n[cfconv-box-reference] {tag} {act}: box gradient vs finite differences {worst / top:.2e} of max {top:.3e} "
          f"(smallest entry {smallest / top:.1e} of max)")
    assert worst <= FD_RTOL * top, (tag, worst, top)


# ---------------------------------------------------------------------------------------------- the kernel's formula on float32 records
@pytest.mark.parametrize("tag", ["triclinic350", "liquid1500", "dense1100", "liquid600_shifted"])
def test_formula_on_float32_records(tag):
    pos, box = frame(tag)
    W, G = 16, 8
    w1, b1, w2, b2, x, gy = weights(W, G, len(pos), 23)
    out = Restatement(W, G, 5.0, 0.4, "ssp", w1, b1, w2, b2).evaluate(pos, box, x, gy)
    rec = out["d"].astype(np.float32)
    n_rec = recovered_shifts(pos, box, out["i"], out["j"], rec)
    assert np.array_equal(n_rec, out["n"]), "image_shift's three roundings do not recover the builder's shifts"
    wrapped = float((np.abs(out["n"]).sum(axis=1) > 0).mean())
    top = np.abs(out["gbox"]).max()
    gB_rec = n_rec.T @ (out["s"][:, None] * rec.astype(np.float64))
    noise = 1.0 + 1e-5 * np.random.default_rng(1).standard_normal(len(out["s"]))
    gB_noise = n_rec.T @ ((out["s"] * noise)[:, None] * rec.astype(np.float64))
    x64, B64 = pos.astype(np.float64), box.astype(np.float64)
    stress = x64.T @ out["g"] + B64.T @ out["gbox"]
    print(f"\n[cfconv-box-reference] {tag}: {len(out['i'])} pairs, {wrapped:.0%} wrapped; records-only {np.abs(gB_rec - out['gbox']).max() / top:.2e}, "
          f"with 1e-5 noise on s {np.abs(gB_noise - out['gbox']).max() / top:.2e} of max {top:.3e}; smallest entry "
          f"{np.abs(out['gbox']).min() / top:.1e} of max; antisymmetric stress {np.abs(stress - stress.T).max() / 2 / np.abs(stress).max():.1e}")
    assert wrapped > 0 and np.isfinite(out["gbox"]).all()
    assert np.abs(gB_rec - out["gbox"]).max() <= 1e-6 * top          # float32 displacements: 6e-8 relative each, far below the bar
    assert np.abs(stress - stress.T).max() / 2 <= 1e-10 * np.abs(stress).max()      # rotation invariance, float64


# ---------------------------------------------------------------------------------------------- the symbol and the op exist
def test_library_exports_backprop_box_and_reports_a_null_handle():
    from nnpops_amd import capi
    L = capi.lib()
    assert hasattr(L, "nnpops_cfconv_backprop_box")
    null = ctypes.c_void_p()
    code = L.nnpops_cfconv_backprop_box(null, null, null, null, null, null, null, null, null)
    assert code < 0 and b"NULL" in L.nnpops_last_error()


def test_operation_periodic_is_registered():
    from nnpops_amd import torch_binding
    torch_binding.load()
    assert hasattr(torch.ops.NNPOpsCFConv, "operation_periodic")
    schema = str(torch.ops.NNPOpsCFConv.operation_periodic.default._schema)
    assert schema.count("Tensor") >= 4, schema
