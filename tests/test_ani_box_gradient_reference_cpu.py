"""The float64 restatement of the AEV that the box-gradient tests compare against, pinned to oracle.AniOracle64 (CPU only).

`Restatement` writes the ANI symmetry functions in torch float64 with every displacement as d = x_j - x_i + n B (B: rows = box
vectors), the integer minimum-image shifts n computed ONCE from the inputs by the reference's rule (z, then y, then x, each by the
diagonal entry) and detached, so that autograd gives dL/dpositions and the formal derivative dL/dB = sum n (x) dL/dd that
nnpops_ani_backprop_box_strided returns.  It is an independent statement of the algorithm (pair and triple lists, index_add), not a
wrapper of the oracle; tests/test_ani_box_gradient_gpu.py loads it from this file.

What pins it (both angle modes, a ~60-atom triclinic and a ~100-atom cubic frame, cutoffs below half the box):
    values, position gradient   max |x - oracle| <= 1e-10 max |oracle|      (AniOracle64: oracle/ani_oracle.c in double precision)
    cell gradient (lower triangle)  against central finite differences of L = <w_r, radial> + <w_a, angular> evaluated with
        AniOracle64, Richardson-extrapolated from the steps h = 2^-13 and 2^-14 Angstrom.  The oracle rounds its box to float32, so
        the steps are powers of two, exactly representable next to a ~10 Angstrom entry (ulp 2^-20).  A pair that crosses a cutoff
        inside the step does so with value and slope zero (cosine cutoff) but with a jump J ~ 0.1 |w| in the SECOND derivative,
        which a difference quotient sees as an error of up to J h / 2 and no extrapolation removes: with h = 2^-8 the triclinic
        frame was 4e-6 .. 7e-6 of its largest entry off, hence the small steps (J h / 2 ~ 3e-6 absolute, 2e-7 of the largest
        entry, should a pair cross at all).  The rest is smaller: truncation of order h^4 after the extrapolation, rounding
        eps |L| / h ~ 2e-9 absolute.  Bar: 1e-6 of the largest entry, two orders below the 1e-4 gate of the GPU tests; measured
        3e-12 .. 1e-11.
"""
import math

import numpy as np
import pytest
import torch

from nnpops_amd import workloads
from oracle import AniOracle64


class Restatement:
    """ANI AEV in torch float64 on float32 inputs and parameters (widened exactly, as AniOracle64 does)."""

    def __init__(self, n_species, rcr, rca, species, radial_functions, angular_functions, torchani=True):
        self.S = int(n_species)
        self.NB = self.S * (self.S + 1) // 2
        self.rcr, self.rca = float(np.float32(rcr)), float(np.float32(rca))
        self.species = np.ascontiguousarray(species, dtype=np.int64)
        self.N = len(self.species)
        self.rf = torch.tensor(np.asarray(radial_functions, dtype=np.float32).reshape(-1, 2).astype(np.float64))
        self.af = torch.tensor(np.asarray(angular_functions, dtype=np.float32).reshape(-1, 4).astype(np.float64))
        self.nR, self.nA = self.rf.shape[0], self.af.shape[0]
        self.torchani = bool(torchani)

    # ------------------------------------------------------------------------------------------ lists (numpy, no gradient)
    def shifts(self, pos, box):
        """-> n [N, N, 3] with d_ij = x_j - x_i + n_ij B the reference's single-round minimum image"""
        d = pos[None, :, :] - pos[:, None, :]
        s3 = np.round(d[..., 2] / box[2, 2])
        d = d - s3[..., None] * box[2]
        s2 = np.round(d[..., 1] / box[1, 1])
        d = d - s2[..., None] * box[1]
        s1 = np.round(d[..., 0] / box[0, 0])
        return -np.stack([s1, s2, s3], axis=-1)

    def lists(self, pos, box):
        """-> directed radial pairs (i, j, n) and triples (centre, j, k, n_j, n_k) with j before k in the centre's list"""
        n = self.shifts(pos, box)
        d = pos[None, :, :] - pos[:, None, :] + n @ box
        r2 = np.einsum("ijk,ijk->ij", d, d)
        np.fill_diagonal(r2, np.inf)
        pi, pj = np.nonzero(r2 < self.rcr ** 2)
        ang = r2 < self.rca ** 2
        ti, tj, tk = [], [], []
        for i in range(self.N):
            nb = np.nonzero(ang[i])[0]
            if len(nb) >= 2:
                a, b = np.triu_indices(len(nb), 1)
                ti.append(np.full(len(a), i)); tj.append(nb[a]); tk.append(nb[b])
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        ti, tj, tk = cat(ti), cat(tj), cat(tk)
        return (pi, pj, n[pi, pj]), (ti, tj, tk, n[ti, tj], n[ti, tk])

    # ------------------------------------------------------------------------------------------ the functions (torch, float64)
    def _radial_terms(self, x, B, pairs):
        i, j, n = pairs
        d = x[j] - x[i] + torch.tensor(n) @ B
        r = d.norm(dim=1)
        fc = 0.5 * torch.cos(math.pi * r / self.rcr) + 0.5
        sh = r[:, None] - self.rf[None, :, 1]
        scale = 0.25 if self.torchani else 1.0
        return scale * fc[:, None] * torch.exp(-self.rf[None, :, 0] * sh * sh), torch.tensor(i * self.S + self.species[j])

    def _angular_terms(self, x, B, triples):
        i, j, k, nj, nk = triples
        u = x[j] - x[i] + torch.tensor(nj) @ B
        v = x[k] - x[i] + torch.tensor(nk) @ B
        ru, rv = u.norm(dim=1), v.norm(dim=1)
        dot = (u * v).sum(dim=1)
        if self.torchani:
            theta = torch.acos(float(np.float32(0.95)) * dot / (ru * rv))      # (the oracle's constant is the float32 0.95f)
        else:                                    # the angle itself, well conditioned next to 0 and pi (the oracle's asin branch)
            theta = torch.atan2(torch.linalg.cross(u, v).norm(dim=1), dot)
        fcfc = (0.5 * torch.cos(math.pi * ru / self.rca) + 0.5) * (0.5 * torch.cos(math.pi * rv / self.rca) + 0.5)
        eta, rs, zeta, ths = (self.af[None, :, c] for c in range(4))
        sh = 0.5 * (ru + rv)[:, None] - rs
        terms = fcfc[:, None] * (1.0 + torch.cos(theta[:, None] - ths)) ** zeta * torch.exp(-eta * sh * sh) * 2.0 ** (1.0 - zeta)
        a, b = np.minimum(self.species[j], self.species[k]), np.maximum(self.species[j], self.species[k])
        bucket = a * self.S - a * (a - 1) // 2 + (b - a)             # upper-triangular row-major
        return terms, torch.tensor(i * self.NB + bucket)

    def evaluate(self, positions, box, wr=None, wa=None, chunk=100000):
        """-> dict(r [N, S nR], a [N, NB nA]) and, with weights, L = <wr, r> + <wa, a>, g = dL/dpositions, gbox = dL/dB (all
        nine entries, shifts held fixed).  The triples go through autograd `chunk` at a time."""
        pos64 = np.asarray(positions, dtype=np.float32).astype(np.float64)
        box64 = np.asarray(box, dtype=np.float32).astype(np.float64).reshape(3, 3)
        pairs, triples = self.lists(pos64, box64)
        x = torch.tensor(pos64, requires_grad=True)
        B = torch.tensor(box64, requires_grad=True)
        want = wr is not None
        radial = torch.zeros(self.N * self.S, self.nR, dtype=torch.float64)
        angular = torch.zeros(self.N * self.NB, self.nA, dtype=torch.float64)
        gx, gB, L = torch.zeros_like(x), torch.zeros_like(B), 0.0
        if want:
            w_r = torch.tensor(np.asarray(wr, dtype=np.float64).reshape(self.N * self.S, self.nR))
            w_a = torch.tensor(np.asarray(wa, dtype=np.float64).reshape(self.N * self.NB, self.nA))

        def accumulate(terms, rows, out, weights):
            nonlocal gx, gB, L
            out.index_add_(0, rows, terms.detach())
            if want and len(rows):
                part = (terms * weights[rows]).sum()
                dx, dB = torch.autograd.grad(part, [x, B])
                gx, gB, L = gx + dx, gB + dB, L + float(part.detach())

        accumulate(*self._radial_terms(x, B, pairs), radial, w_r if want else None)
        for lo in range(0, len(triples[0]), chunk):
            accumulate(*self._angular_terms(x, B, tuple(t[lo:lo + chunk] for t in triples)), angular, w_a if want else None)
        out = dict(r=radial.reshape(self.N, -1).numpy(), a=angular.reshape(self.N, -1).numpy())
        if want:
            out.update(L=L, g=gx.numpy(), gbox=gB.numpy())
        return out


# ---------------------------------------------------------------------------------------------- the pinning tests
PIN_RTOL = 1e-10
FD_RTOL = 1e-6

_FRAMES = {}


def _frame(tag):
    """-> (n_species, rcr, rca, species, pos, box); cutoffs below half the narrowest width of the cell"""
    if tag not in _FRAMES:
        if tag == "triclinic60":                   # L = 10.6: narrowest width 10.5
            pos, species, box = workloads.triclinic_box(60, seed=5, density=0.05)
            cfg = (7, 4.2, 3.2)
        else:                                      # cubic100: L = 10.8
            pos, species, box = workloads.random_box(100, density=0.08, seed=6)
            cfg = (7, 5.1, 3.5)
        _FRAMES[tag] = cfg + (species, pos, box)
    return _FRAMES[tag]


def _weights(shape_r, shape_a, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape_r).astype(np.float32), rng.standard_normal(shape_a).astype(np.float32)


@pytest.mark.parametrize("torchani", [True, False], ids=["torchani", "paper"])
@pytest.mark.parametrize("tag", ["triclinic60", "cubic100"])
def test_restatement_is_the_oracle(tag, torchani):
    n_species, rcr, rca, species, pos, box = _frame(tag)
    rf, af = workloads.ani2x_functions()
    oracle = AniOracle64(n_species, rcr, rca, species, rf, af, periodic=True, torchani=torchani)
    r_ref, a_ref = oracle.forward(pos, box)
    wr, wa = _weights(r_ref.shape, a_ref.shape, 17)
    g_ref = oracle.backward(wr, wa)
    out = Restatement(n_species, rcr, rca, species, rf, af, torchani).evaluate(pos, box, wr, wa)
    assert np.abs(a_ref).max() > 0 and np.abs(out["gbox"]).max() > 0          # (triples and wrapped pairs exist)
    for name, x, x_ref in (("radial", out["r"], r_ref), ("angular", out["a"], a_ref), ("position gradient", out["g"], g_ref)):
        err = np.abs(x - x_ref).max() / np.abs(x_ref).max()
        print(f"\n[ani-box-reference] {tag} torchani={torchani}: {name} {err:.2e} of max")
        assert err <= PIN_RTOL, (tag, name, err)


@pytest.mark.parametrize("torchani", [True, False], ids=["torchani", "paper"])
@pytest.mark.parametrize("tag", ["triclinic60", "cubic100"])
def test_cell_gradient_against_finite_differences_of_the_oracle(tag, torchani):
    n_species, rcr, rca, species, pos, box = _frame(tag)
    rf, af = workloads.ani2x_functions()
    oracle = AniOracle64(n_species, rcr, rca, species, rf, af, periodic=True, torchani=torchani)
    r0, a0 = oracle.forward(pos, box)
    wr, wa = _weights(r0.shape, a0.shape, 17)
    w_r, w_a = wr.astype(np.float64), wa.astype(np.float64)

    def energy(b):
        assert np.array_equal(b.astype(np.float32).astype(np.float64), b)       # (the oracle's float32 box is the box meant)
        r, a = oracle.forward(pos, b)
        return float((r * w_r).sum() + (a * w_a).sum())

    out = Restatement(n_species, rcr, rca, species, rf, af, torchani).evaluate(pos, box, wr, wa)
    box64 = np.asarray(box, dtype=np.float64)
    worst, top = 0.0, np.abs(np.tril(out["gbox"])).max()
    for k in range(3):
        for c in range(k + 1):                     # the lower triangle: the entries the minimum-image rule reads
            def central(h):
                plus, minus = box64.copy(), box64.copy()
                plus[k, c] += h; minus[k, c] -= h
                return (energy(plus) - energy(minus)) / (2 * h)
            fd = (4.0 * central(2.0 ** -14) - central(2.0 ** -13)) / 3.0
            worst = max(worst, abs(fd - out["gbox"][k, c]))
    print(f"\n[ani-box-reference] {tag} torchani={torchani}: cell gradient vs finite differences {worst / top:.2e} of max {top:.3e}")
    assert worst <= FD_RTOL * top, (tag, worst, top)
