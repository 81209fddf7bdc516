"""The frames and the float64 judge of the periodic-batch tests of the ANI symmetry functions (no GPU code, no tests; importable
anywhere).

A periodic batch (nnpops_ani_set_molecules on a periodic handle) is M frames behind one handle, frame m = atoms
[offsets[m], offsets[m + 1]) in the box box[m] of its own; atoms of different frames never see each other.  The judge is
ani_float64.Restatement.evaluate, run PER MOLECULE with that molecule's box and assembled to batch arrays: the AEV, dL/dpositions,
dL/dB [M, 3, 3] (shifts held fixed, all nine entries) and L of L = <w_r, radial> + <w_a, angular> with seeded float32 weights.
tests/test_ani_periodic_batch_reference_cpu.py pins it.

FRAMES: four frames of different sizes, each at least two radial cutoffs (2 x 5.1) wide and each with shifted pairs on all three
axes; as a batch their offsets are 0, 130, 330, 480, 547 -- no segment starts or ends on a multiple of 64, one is longer than three
scan batches of 64, one barely longer than one.  MODULE FRAMES: three frames of one 50-water box, jittered and scaled, for the
modules that batch conformers of their own molecule.
"""
import functools

import numpy as np

from ani_float64 import Restatement
from ani_tangent_float64 import judge as tangent_judge
from nnpops_amd import workloads

RCR, RCA, N_SPECIES = 5.1, 3.5, 7


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def frames():
    """-> tuple of (species, pos, box): the four frames of the C-ABI tests"""
    out = []
    for pos, species, box in (workloads.random_box(130, seed=91), workloads.triclinic_box(200, seed=92), workloads.water_box(50, seed=93),
                              workloads.random_box(67, density=0.05, seed=94)):
        out.append(_frozen(np.ascontiguousarray(species, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.float32),
                           np.ascontiguousarray(box, dtype=np.float32).reshape(3, 3)))
    return tuple(out)


def assemble(parts):
    """frames (species, pos, box) -> (species [N], pos [N, 3], boxes [M, 3, 3], offsets [M + 1]) of the batch, in the given order"""
    species = np.concatenate([p[0] for p in parts]).astype(np.int32)
    pos = np.concatenate([p[1] for p in parts]).astype(np.float32)
    boxes = np.stack([p[2] for p in parts]).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int32)
    return species, pos, boxes, offsets


@functools.lru_cache(maxsize=None)
def batch():
    """the four frames as one batch: offsets 0, 130, 330, 480, 547"""
    return _frozen(*assemble(frames()))


MODULE_SCALES = (0.97, 1.00, 1.04)


@functools.lru_cache(maxsize=None)
def module_frames():
    """-> (species [150], coordinates [3, 150, 3], cells [3, 3, 3]): three frames of the 50-water box, positions jittered by up to
    0.05 A and positions and box scaled by 0.97, 1.00, 1.04 (the smallest box 11.10 A wide, above 2 x 5.1)"""
    species, pos, box = frames()[2]
    rng = np.random.default_rng(95)
    coords, cells = [], []
    for s in MODULE_SCALES:
        jitter = rng.uniform(-0.05, 0.05, pos.shape)
        coords.append(((pos + jitter) * s).astype(np.float32))
        cells.append((box * np.float32(s)).astype(np.float32))
    return _frozen(species.copy(), np.stack(coords), np.stack(cells))


def weights(n_atoms, seed, n_radial=16, n_angular=32, n_species=N_SPECIES):
    """seeded float32 weights (w_r [N, S nR], w_a [N, NB nA]) of unit normal entries"""
    rng = np.random.default_rng([n_atoms, seed])
    nb = n_species * (n_species + 1) // 2
    return (rng.standard_normal((n_atoms, n_species * n_radial)).astype(np.float32),
            rng.standard_normal((n_atoms, nb * n_angular)).astype(np.float32))


def judge(species, pos, boxes, offsets, functions, torchani=True, wr=None, wa=None, n_species=N_SPECIES, rcr=RCR, rca=RCA):
    """Restatement.evaluate per molecule, each with its own box -> dict(r [N, S nR], a [N, NB nA]) and, with weights, g [N, 3],
    gbox [M, 3, 3], L (the sum over the molecules) and Lm [M]"""
    rf, af = functions
    parts = []
    for m in range(len(offsets) - 1):
        lo, hi = int(offsets[m]), int(offsets[m + 1])
        rest = Restatement(n_species, rcr, rca, species[lo:hi], rf, af, torchani)
        parts.append(rest.evaluate(pos[lo:hi], boxes[m], None if wr is None else wr[lo:hi], None if wa is None else wa[lo:hi]))
    out = dict(r=np.concatenate([p["r"] for p in parts]), a=np.concatenate([p["a"] for p in parts]))
    if wr is not None:
        out.update(g=np.concatenate([p["g"] for p in parts]), gbox=np.stack([p["gbox"] for p in parts]),
                   Lm=np.array([p["L"] for p in parts]), L=float(sum(p["L"] for p in parts)))
    return out


def tangent(species, pos, boxes, offsets, functions, v, torchani=True, n_species=N_SPECIES, rcr=RCR, rca=RCA):
    """ani_tangent_float64.judge per molecule with its own box -> (radial tangent [N, S nR], angular tangent [N, NB nA])"""
    rf, af = functions
    parts = []
    for m in range(len(offsets) - 1):
        lo, hi = int(offsets[m]), int(offsets[m + 1])
        rest = Restatement(n_species, rcr, rca, species[lo:hi], rf, af, torchani)
        parts.append(tangent_judge(rest, pos[lo:hi], boxes[m], v[lo:hi]))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def census(species, pos, box, rcr=RCR, rca=RCA):
    """-> dict(pairs, shifted, per_axis [3], triples, width [3]): directed radial pairs, how many of them carry a shift (and along
    which axis), the triples, and the widths of the box along its three diagonal entries"""
    rf, af = workloads.ani2x_functions()
    rest = Restatement(N_SPECIES, rcr, rca, species, rf, af)
    (pi, pj, n), triples = rest.lists(pos.astype(np.float64), box.astype(np.float64))
    return dict(pairs=len(pi), shifted=int((n != 0).any(axis=1).sum()), per_axis=[int((n[:, a] != 0).sum()) for a in range(3)],
                triples=len(triples[0]), width=[float(box[a, a]) for a in range(3)])


def stress_antisymmetry(pos, boxes, offsets, g, gbox):
    """per molecule: (largest entry of the antisymmetric part of W_m = x_m^T g_m + B_m^T dB_m, largest entry of W_m)"""
    out = []
    for m in range(len(offsets) - 1):
        lo, hi = int(offsets[m]), int(offsets[m + 1])
        x, B = pos[lo:hi].astype(np.float64), boxes[m].astype(np.float64)
        W = x.T @ np.asarray(g[lo:hi], dtype=np.float64) + B.T @ np.asarray(gbox[m], dtype=np.float64)
        out.append((float(np.abs(W - W.T).max()) / 2, float(np.abs(W).max())))
    return out
