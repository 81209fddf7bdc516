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
modules that batch conformers of their own molecule.  EDGE BATCHES (tests/test_ani_periodic_batch_edges_gpu.py): size_edges(),
many_molecules(), dense_pair() and slots128_pair(), described where they are built; all seeded, cached and read-only.
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


# ---------------------------------------------------------------------------------------------- the edge batches
# Tiny molecules are clusters ASTRIDE A CORNER of their box: built around the origin with an atom in the (+, +, +) octant and one in the
# (-, -, -) octant, then wrapped into the box by whole box vectors -- so the pair of those two is shifted on all three axes.
def _tiny_box(rng, triclinic):
    """a box of its own, every diagonal entry 10.5 .. 14 A (above 2 x 5.1) or, one axis in three, twice that: a shift recovered
    against ANOTHER molecule's box is then another integer.  Reduced-form triclinic on request"""
    lx, ly, lz = rng.uniform(10.5, 14.0, 3) * rng.choice([1.0, 1.0, 2.0], 3)
    if triclinic:
        return np.array([[lx, 0, 0], [0.15 * lx, ly, 0], [-0.05 * lx, -0.1 * ly, lz]], dtype=np.float32)
    return np.diag([lx, ly, lz]).astype(np.float32)


def _wrapped(points, box):
    """points around the origin -> the same points brought into the box by whole box vectors (float32)"""
    B = box.astype(np.float64)
    frac = np.asarray(points, dtype=np.float64) @ np.linalg.inv(B)
    return ((frac - np.floor(frac)) @ B).astype(np.float32)


def _corner_cluster(n, rng):
    """n points around the origin: the first in the (+, +, +) octant, the second in the (-, -, -) octant, 1.0 .. 2.4 A apart; every
    further one 0.9 .. 2.5 A from an earlier one, no two closer than 0.9 A, every coordinate inside +-2.5 A"""
    pts = [rng.uniform(0.3, 0.7, 3)]
    if n > 1:
        pts.append(-rng.uniform(0.3, 0.7, 3))
    while len(pts) < n:
        step = rng.normal(size=3)
        cand = pts[rng.integers(0, len(pts))] + step * rng.uniform(0.9, 2.5) / np.linalg.norm(step)
        if np.abs(cand).max() < 2.5 and np.min(np.linalg.norm(np.array(pts) - cand, axis=1)) >= 0.9:
            pts.append(cand)
    return np.array(pts[:n])


def _tiny_frame(n, seed, triclinic, points=None, far=0):
    """-> (species, pos, box) of a corner cluster of n atoms (or of the given points); `far` further atoms sit at the middle of the
    box, out of every other atom's reach"""
    rng = np.random.default_rng(seed)
    box = _tiny_box(rng, triclinic)
    pts = _corner_cluster(n - far, rng) if points is None else np.asarray(points, dtype=np.float64)
    if far:                                            # (in front: the molecule's last rows, the last workgroup's, keep their neighbours)
        pts = np.concatenate([np.tile(0.5 * box.astype(np.float64).sum(axis=0), (far, 1)), pts])
    species = rng.integers(0, N_SPECIES, len(pts)).astype(np.int32)
    return _frozen(species, _wrapped(pts, box), box)


def _liquid(maker, n, corner_last=False, **kwargs):
    """-> (species, pos, box) of a liquid of workloads; corner_last: the atom nearest to the origin corner of the box changes places
    with the last one, so that the molecule's last row -- the one a remainder of the walk falls on -- has shifted pairs on every axis"""
    pos, species, box = maker(n, **kwargs)
    if corner_last:
        pos, species = pos.copy(), species.copy()
        a = int(np.argmin(np.abs(pos).max(axis=1)))
        pos[[a, n - 1]], species[[a, n - 1]] = pos[[n - 1, a]], species[[n - 1, a]]
    return _frozen(np.ascontiguousarray(species, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.float32),
                   np.ascontiguousarray(box, dtype=np.float32).reshape(3, 3))


SIZE_EDGES = (257, 1, 64, 2, 300, 3, 65, 4, 256, 5)
# the 3-atom molecule, around the corner: 1 -- 0 -- 2 bent by 145 degrees at atom 0 (NOT in line: at 180 degrees the angle of the
# paper's convention has no derivative), |0 1| = 2.2, |0 2| = 2.1 and |1 2| = 4.1 A.  Atom 0 has two angular neighbours (the
# molecule's one triple); atoms 1 and 2 have ONE angular neighbour each (a lone leg, no triple of their own) and see each other
# between the angular cutoff 3.5 and the radial cutoff 5.1
THREE_ATOMS = ((0.1, -0.1, 0.1), (1.4, 1.2, 1.3), (-1.9, -0.4, -0.6))


@functools.lru_cache(maxsize=None)
def size_edge_frames():
    """-> tuple of (species, pos, box) with 257, 1, 64, 2, 300, 3, 65, 4, 256, 5 atoms: the molecule sizes at which the per-molecule
    box-gradient pass changes its walk (ani_box_molecule_blocks: 4 atoms per workgroup, at most 64 workgroups, so 256 atoms a round).
    The liquids of 64 and 65 atoms at density 0.05 (10.9 A wide), the others at 0.1; the 300- and the 65-atom frames triclinic.  The
    tiny ones are corner clusters in boxes of their own (the 3- and 5-atom boxes triclinic); the 5-atom molecule's FIRST atom stands
    at the middle of its box, alone.  The last atom of the 257- and of the 65-atom frames -- the one atom of the second round, the
    one atom of the 17th workgroup -- is the frame's nearest to a box corner."""
    return (_liquid(workloads.random_box, 257, corner_last=True, seed=101), _tiny_frame(1, 102, False),
            _liquid(workloads.random_box, 64, density=0.05, seed=103), _tiny_frame(2, 104, False),
            _liquid(workloads.triclinic_box, 300, seed=105), _tiny_frame(3, 106, True, points=THREE_ATOMS),
            _liquid(workloads.triclinic_box, 65, corner_last=True, density=0.05, seed=107), _tiny_frame(4, 108, False),
            _liquid(workloads.random_box, 256, seed=109), _tiny_frame(5, 110, True, far=1))


@functools.lru_cache(maxsize=None)
def size_edges():
    """size_edge_frames() as one batch of 957 atoms"""
    return _frozen(*assemble(size_edge_frames()))


@functools.lru_cache(maxsize=None)
def many_molecule_frames():
    """-> 70 corner clusters of 1, 2, ..., 9, 1, 2, ... atoms (343 in all), every one in a box of its own, every third box triclinic"""
    return tuple(_tiny_frame(1 + m % 9, 1000 + m, m % 3 == 1) for m in range(70))


@functools.lru_cache(maxsize=None)
def many_molecules():
    return _frozen(*assemble(many_molecule_frames()))


@functools.lru_cache(maxsize=None)
def dense_pair_frames():
    """-> two liquids of 230 and 300 atoms at density 0.2 (10.5 and 11.4 A wide): records of 64 slots and more than 200 triples per
    atom, as dense900 of ani_float64.system -- where the backward stores the leg forces in the receivers' rows"""
    return (_liquid(workloads.random_box, 230, density=0.2, seed=111), _liquid(workloads.random_box, 300, density=0.2, seed=112))


@functools.lru_cache(maxsize=None)
def dense_pair():
    return _frozen(*assemble(dense_pair_frames()))


SLOTS128 = (3, 5.2, 4.8)          # (species, radial cutoff, angular cutoff) of the 128-slot batch


@functools.lru_cache(maxsize=None)
def slots128_frames():
    """-> slots128 of ani_float64.system (400 atoms, 3 species, cutoffs 5.2 / 4.8: records of 128 slots) and a second frame of the
    same recipe, 300 atoms, another seed"""
    return (_liquid(workloads.random_box, 400, density=0.2, seed=7, min_dist=0.8, n_species=3),
            _liquid(workloads.random_box, 300, density=0.2, seed=8, min_dist=0.8, n_species=3))


@functools.lru_cache(maxsize=None)
def slots128_pair():
    return _frozen(*assemble(slots128_frames()))


def paired(boxes, offsets):
    """neighbouring molecules two by two under the box of the first of them -> (boxes [M / 2, 3, 3], offsets [M / 2 + 1])"""
    assert (len(offsets) - 1) % 2 == 0
    return np.ascontiguousarray(boxes[0::2]), np.ascontiguousarray(offsets[0::2])


def molecule_blocks(n_atoms):
    """ani_box_molecule_blocks of csrc/ani_box_grad.h restated: the workgroups (of 4 waves, an atom each) of a molecule's pass"""
    return min(max(-(-int(n_atoms) // 4), 1), 64)


def angular_counts(species, pos, box, rcr=RCR, rca=RCA):
    """-> [N] neighbours inside the angular cutoff of every atom (the restatement's lists)"""
    rf, af = workloads.ani2x_functions()
    rest = Restatement(N_SPECIES, rcr, rca, species, rf, af)
    p, b = pos.astype(np.float64), box.astype(np.float64)
    d = p[None, :, :] - p[:, None, :] + rest.shifts(p, b) @ b
    r2 = np.einsum("ijk,ijk->ij", d, d)
    np.fill_diagonal(r2, np.inf)
    return (r2 < float(np.float32(rca)) ** 2).sum(axis=1)


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
