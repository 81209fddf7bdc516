"""The float64 judges of the ANI tests that are not oracle.AniOracle64 itself (no GPU code, no tests; importable anywhere), and the
frames of the family.

`Restatement` writes the ANI symmetry functions in torch float64 with every displacement as d = x_j - x_i + n B (B: rows = box
vectors), the integer minimum-image shifts n computed ONCE from the inputs by the reference's rule (z, then y, then x, each by the
diagonal entry) and detached, so that autograd gives dL/dpositions and the formal derivative dL/dB = sum n (x) dL/dd that
nnpops_ani_backprop_box_strided returns.  It is an independent statement of the algorithm (pair and triple lists, index_add), not a
wrapper of the oracle; tests/test_ani_box_gradient_reference_cpu.py pins it.

`segment_means` restates nnpops_mlp_energy_mean_segments in numpy float64: the per-atom, per-member energies lie in the species-grouped
order the networks write them in, `places[row]` is the place of a row in that order (the inverse of the frame's rows) and molecule b is
the rows offsets[b] .. offsets[b + 1] - 1.  tests/test_ani_batch_energy_cpu.py pins it.
"""
import functools
import math

import numpy as np
import torch

from box_gradient_judge import moved_frames
from nnpops_amd import workloads


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


def weights(shape_r, shape_a, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape_r).astype(np.float32), rng.standard_normal(shape_a).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the frames of the family
@functools.lru_cache(maxsize=None)
def system(tag):
    """-> (n_species, rcr, rca, species, pos, box or None), built once and read-only"""
    box = None
    cfg = (7, 5.1, 3.5)
    if tag == "liquid600":                     # 7-species periodic liquid, ~18 angular neighbours; all-pairs build
        pos, species, box = workloads.random_box(600, seed=81)
    elif tag == "liquid600_shifted":           # every atom 0.37 box lengths along x: a third of them outside the box
        _, _, _, species, pos, box = system("liquid600")
        pos = moved_frames(pos, box)[0]
    elif tag == "liquid600_wrapped":           # ... and those brought back by one box vector: other shifts, another dL/dB
        _, _, _, species, pos, box = system("liquid600")
        pos = moved_frames(pos, box)[1]
    elif tag == "conformer60":                 # a compact molecule in vacuum
        pos, species = workloads.conformer(60, seed=82)
    elif tag == "triclinic200":
        pos, species, box = workloads.triclinic_box(200)
    elif tag == "slots128":                    # records of 128 slots
        pos, species, box = workloads.random_box(400, density=0.2, seed=7, min_dist=0.8, n_species=3)
        cfg = (3, 5.2, 4.8)
    elif tag in ("slots256", "slots256_loose"):      # records of 256 slots: the same lattice gas without its box; the loose frame is 1.15 x wider
        pos, species, _ = workloads.random_box(260, density=0.5, seed=7, min_dist=0.5, n_species=2)
        if tag == "slots256_loose":
            pos = (pos * np.float32(1.15)).astype(np.float32)
        cfg = (2, 5.2, 5.0)
    elif tag == "dense900":                    # the 64-slot dense liquid of test_ani_gpu.py: two waves per atom, leg forces in the receivers' rows
        pos, species, box = workloads.random_box(900, density=0.2, seed=33)
    elif tag == "liquid2100":                  # cell-grid build; large enough for NNPOPS_ANI_STREAMS to split (2 048 atoms or more)
        pos, species, box = workloads.random_box(2100, seed=83)
    elif tag == "triclinic60":                 # the pinning frames, cutoffs below half the narrowest width of the cell.  L = 10.6: narrowest width 10.5
        pos, species, box = workloads.triclinic_box(60, seed=5, density=0.05)
        cfg = (7, 4.2, 3.2)
    elif tag == "cubic100":                    # L = 10.8
        pos, species, box = workloads.random_box(100, density=0.08, seed=6)
    else:
        raise KeyError(tag)
    for a in (species, pos, box):
        if a is not None:
            a.setflags(write=False)
    return cfg + (species, pos, box)


# ---------------------------------------------------------------------------------------------- the batched energy step
def segment_means(energies, places, offsets, scale):
    """energies [grouped atoms][members], places [rows], offsets [B + 1] -> float64 [B]: scale * sum over the molecule's atoms and members"""
    e = np.asarray(energies, dtype=np.float64)
    places, offsets = np.asarray(places, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    return np.array([scale * e[places[offsets[b]:offsets[b + 1]]].sum() for b in range(len(offsets) - 1)], dtype=np.float64)


def random_grouping(sizes, kinds, members, seed):
    """A batch of molecules of the given sizes whose atoms carry random kinds: -> (energies in grouped order [n][members] float32,
    rows [n] (grouped order -> row), places [n] (row -> grouped order), offsets [B + 1], kind of every row)"""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    kind = rng.integers(0, kinds, n)
    rows = np.argsort(kind, kind="stable").astype(np.int32)
    places = np.empty(n, dtype=np.int32)
    places[rows] = np.arange(n, dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    energies = (rng.standard_normal((n, members)) * 10.0 ** rng.uniform(-2, 1, (n, 1))).astype(np.float32)
    return energies, rows, places, offsets, kind
