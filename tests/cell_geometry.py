"""Geometry helpers of test_cell_geometry_gpu.py (no GPU code; importable anywhere).

* boxes and atom clouds that make the cell grid of nnpops_amd/csrc/celllist.h anisotropic, tilted, barely fitting, capped or
  flat -- as jittered lattices at about liquid density, formed in float64 and cast to float32 ONCE, so that the device and the
  reference below start from the same numbers;
* ``grid_for``: what ``decide_grid`` must answer for a box, restated on the host from the geometry (perpendicular widths as
  volume / face area of a general cell, not the lower-triangular short cut of the kernel);
* ``reference_pairs`` / ``settle``: the float64 brute force over all pairs with the reference's minimum-image rule
  (getNeighborPairsCPU.cpp:66-68: one round per axis, z then y then x, by the diagonal element), and the conditions on the
  inputs that let a pair list be compared without an "either way" escape.
"""
import math

import numpy as np
import torch

SPACING = 2.15             # lattice constant of 0.1 atoms per cubic Angstrom
MARGIN = 1e-5              # no pair within MARGIN * cutoff of a cutoff
HALF = 1e-6                # no candidate pair with a scaled displacement component this close to a half-integer


# ---------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------
def ortho(mx, my, mz, c):
    return np.diag([mx * c, my * c, mz * c]).astype(np.float64)


def tilted(lx, ly, lz):
    """Reduced-form cell near the limit of the reduction: every off-diagonal is +-0.45 of its diagonal."""
    return np.array([[lx, 0, 0], [0.45 * lx, ly, 0], [-0.45 * lx, 0.45 * ly, lz]], np.float64)


def on_binary_lattice(box, step=2.0 ** -10):
    """The box with every entry a multiple of 2^-10 A (float32, exact).  A minimum image takes whole multiples k * L of the box
    entries from a displacement: with at most 17 significant bits in L they are exact in float32 for every k the tests produce,
    so a fused multiply-add (the device) and a product followed by a difference (the float32 oracles) give the same bits, and
    atoms several boxes apart cost the comparison no rounding that only one side makes."""
    return (np.round(np.asarray(box, np.float64) / step) * step).astype(np.float32)


def perpendicular_widths(box):
    """Distance between opposite faces of the cell with rows a, b, c: (V / |b x c|, V / |c x a|, V / |a x b|)."""
    a, b, c = np.asarray(box, np.float64)
    vol = abs(np.dot(a, np.cross(b, c)))
    return np.array([vol / np.linalg.norm(np.cross(b, c)), vol / np.linalg.norm(np.cross(c, a)),
                     vol / np.linalg.norm(np.cross(a, b))])


def grid_for(widths, cutoff, max_cells, fine, periodic):
    """The grid decide_grid must build over a region of these perpendicular widths: {nx, ny, nz, ncells, m, ok, periodic}.
    Refuses to answer (asserts) when a width sits so close to a whole number of cells that float32 could count differently."""
    c = cutoff * 1.0001
    widths = np.asarray(widths, np.float64)

    def cells(width_of_cell):
        ratio = widths / width_of_cell
        assert np.all((np.abs(ratio - np.round(ratio)) > 1e-4) | (ratio < 0.5)), ratio
        return [max(1, int(math.floor(r))) for r in ratio]

    def answer(n, m, ok):
        return dict(nx=n[0], ny=n[1], nz=n[2], ncells=n[0] * n[1] * n[2], m=m, ok=ok, periodic=int(periodic))

    if fine:
        f = cells(0.5 * c)
        if f[0] * f[1] * f[2] <= max_cells and (not periodic or min(f) >= 5):
            return answer(f, 2, 1)
    nx, ny, nz = cells(c)
    ok = 0 if periodic and min(nx, ny, nz) < 3 else 1
    least = 3 if periodic else 1
    while nx * ny * nz > max_cells:                  # the cap: shave an eighth off the longest axis
        if nx >= ny and nx >= nz:
            nx = max(least, nx - (nx + 7) // 8)
        elif ny >= nz:
            ny = max(least, ny - (ny + 7) // 8)
        else:
            nz = max(least, nz - (nz + 7) // 8)
        if periodic and nx == ny == nz == 3:
            break
    if nx * ny * nz > max_cells:
        ok = 0
    return answer([nx, ny, nz], 1, ok)


def open_extent(pos32):
    """Widths of the region the non-periodic grid covers: the bounding box with a pad of 1e-3 on every side."""
    p = np.asarray(pos32, np.float64)
    return p.max(0) - p.min(0) + 2e-3


# ---------------------------------------------------------------------------------------------
# atoms
# ---------------------------------------------------------------------------------------------
def lattice_fractions(n, edges, rng, jitter=0.25):
    """n sites of a jittered lattice filling the unit cube; the number of sites along an axis follows its edge length
    (an edge of 0: one layer, every fraction exactly 0.5)."""
    edges = np.asarray(edges, np.float64)
    live = edges > 0
    scale = (n / edges[live].prod()) ** (1.0 / live.sum())
    k = np.where(live, np.maximum(1, np.ceil(edges * scale)), 1).astype(np.int64)
    assert k.prod() >= n
    idx = rng.permutation(int(k.prod()))[:n]
    ijk = np.stack(np.unravel_index(idx, tuple(k)), 1).astype(np.float64)
    frac = (ijk + 0.5 + rng.uniform(-jitter, jitter, (n, 3)) * live) / k
    return frac


def harden(frac, coarse, fine, rng, vectors=(0, 1, 2)):
    """The hard inputs: a tenth of the atoms exactly on cell faces (of the full-width and of the half-width grid, fraction 0
    included), then every atom moved by a whole combination (-3 .. 3) of the box vectors `vectors`.
    -> (fractions, snapped atoms)."""
    n = len(frac)
    frac = frac.copy()
    pick = rng.choice(n, n // 10, replace=False)
    axis = rng.integers(0, 3, len(pick))
    dims = np.where(rng.integers(0, 2, len(pick)) == 0, np.asarray(coarse)[axis], np.asarray(fine)[axis])
    face = rng.integers(0, 1 << 30, len(pick)) % dims
    face[:12] = 0                                     # a dozen on the face the periodic wrap maps to itself
    frac[pick, axis] = face / dims
    move = np.zeros((n, 3))
    move[:, list(vectors)] = rng.integers(-3, 4, (n, len(vectors)))
    return frac + move, pick


def cast_once(frac, box):
    """fractions -> float32 positions (rows of `box` are the cell vectors)."""
    return (np.asarray(frac, np.float64) @ np.asarray(box, np.float64)).astype(np.float32)


def corner_blob(n, rng):
    """A liquid-density cube of n atoms centred on the origin -- the corner of a periodic cell, so that the blob lies across all
    three seams at once (float64 positions, negative coordinates included)."""
    edge = SPACING * n ** (1.0 / 3.0)
    return (lattice_fractions(n, [edge] * 3, rng) - 0.5) * edge


def open_cloud(shape, n, rng, far=90.0):
    """Non-periodic clouds whose bounding box is no cube (float64 positions)."""
    if shape == "sheet":                                           # every z the same number
        edge = SPACING * math.sqrt(n)
        pos = lattice_fractions(n, [edge, edge, 0.0], rng) * np.array([edge, edge, 0.0])
        pos[:, 2] = 1.25
        return pos
    if shape == "rod":                                             # extents 40 : 4 : 1
        a = (n * SPACING ** 3 / 160.0) ** (1.0 / 3.0)
        edges = np.array([40 * a, 4 * a, a])
        return lattice_fractions(n, edges, rng) * edges
    if shape == "dumbbell":                                        # two blobs far apart: a bounding box of mostly empty cells
        half = n // 2
        e1, e2 = SPACING * half ** (1.0 / 3.0), SPACING * (n - half) ** (1.0 / 3.0)
        one = lattice_fractions(half, [e1] * 3, rng) * e1
        two = lattice_fractions(n - half, [e2] * 3, rng) * e2 + far * np.array([1.0, 0.8, 0.6])
        return np.concatenate([one, two])[rng.permutation(n)]
    raise ValueError(shape)


# ---------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------
def _block(pos, box, cutoffs, rows, ncols):
    """rows x columns [0, ncols) in float64 -> (row, col, delta, distance) of the pairs within cutoffs[0] * (1 + MARGIN), and
    the (row, col) that break a condition on the inputs for any of the cutoffs."""
    d = pos[rows][:, None, :] - pos[None, :ncols, :]
    near = []
    if box is not None:
        for axis in (2, 1, 0):
            s = d[..., axis] / box[axis, axis]
            near.append((axis, ((s - torch.floor(s) - 0.5).abs() < HALF).nonzero()))
            d -= torch.round(s)[..., None] * box[axis]
    dist2 = (d * d).sum(-1)
    cols = torch.arange(ncols)
    dist2[rows[:, None] == cols[None, :]] = float("inf")
    reach = max(cutoffs) * (1 + MARGIN)
    bad = []
    for axis, at in near:                      # a candidate whose image hangs on how a half-integer rounds
        if len(at):
            dd = d[at[:, 0], at[:, 1]]
            alt = torch.minimum(((dd + box[axis]) ** 2).sum(-1), ((dd - box[axis]) ** 2).sum(-1))
            hit = torch.minimum(alt, dist2[at[:, 0], at[:, 1]]) <= reach * reach
            bad.append(at[hit])
    for c in cutoffs:                          # a pair within rounding of a cutoff
        lo, hi = (c * (1 - MARGIN)) ** 2, (c * (1 + MARGIN)) ** 2
        bad.append(((dist2 > lo) & (dist2 < hi)).nonzero())
    bad = torch.cat(bad) if bad else torch.zeros((0, 2), dtype=torch.long)
    keep = (dist2 <= cutoffs[0] ** 2).nonzero()
    r, c = keep[:, 0], keep[:, 1]
    return rows[r], c, d[r, c], dist2[r, c].sqrt(), torch.stack([rows[bad[:, 0]], bad[:, 1]], 1)


def rows_against_all(pos32, box, cutoffs, rows, chunk=256):
    """Every partner (any index) of the atoms `rows`: (row, col, delta = pos[row] - pos[col] wrapped, distance, offenders)."""
    pos = torch.from_numpy(np.asarray(pos32, np.float64))
    tbox = None if box is None else torch.from_numpy(np.asarray(box, np.float64))
    rows = torch.as_tensor(np.asarray(rows), dtype=torch.long)
    out = [_block(pos, tbox, cutoffs, rows[k:k + chunk], len(pos)) for k in range(0, len(rows), chunk)]
    return [torch.cat([o[q] for o in out]).numpy() for q in range(5)]


def reference_pairs(pos32, box, cutoffs, chunk=256):
    """All pairs (row > col) within cutoffs[0], the reference's arithmetic in float64, sorted by (row, col):
    -> dict(i, j, deltas, dist, offenders [K, 2])."""
    pos = torch.from_numpy(np.asarray(pos32, np.float64))
    tbox = None if box is None else torch.from_numpy(np.asarray(box, np.float64))
    n = len(pos)
    out = []
    for k in range(0, n, chunk):
        rows = torch.arange(k, min(k + chunk, n))
        r, c, d, dist, bad = _block(pos, tbox, cutoffs, rows, int(rows[-1]) + 1)
        out.append((r, c, d, dist, bad[bad[:, 1] < bad[:, 0]]))
    r, c, d, dist, bad = [torch.cat([o[q] for o in out]).numpy() for q in range(5)]
    lower = c < r
    return dict(i=r[lower], j=c[lower], deltas=d[lower], dist=dist[lower], offenders=bad)


def settle(pos32, box, cutoffs, rng, protected=(), rows=None, axes=(0, 1, 2)):
    """Move the few atoms that break a condition on the inputs (a pair within MARGIN of a cutoff, a candidate pair at a
    half-integer of the box) by a hundredth of an Angstrom along `axes` (a sheet stays flat with axes = (0, 1)) until none
    does.  Deterministic for a given generator.
    rows = None: every pair of the system is looked at and the full reference list is returned with the positions;
    otherwise only the pairs of those rows (against all atoms), for systems too large for the full scan.
    -> (positions float32, reference dict)."""
    pos32 = np.array(pos32, np.float32)
    protected = set(int(a) for a in protected)
    n = len(pos32)
    if rows is None:
        ref = reference_pairs(pos32, box, cutoffs)
    else:
        r, c, d, dist, bad = rows_against_all(pos32, box, cutoffs, rows)
        ref = dict(i=r, j=c, deltas=d, dist=dist, offenders=bad)
    for _ in range(50):
        bad = ref["offenders"]
        if len(bad) == 0:
            return pos32, ref
        watched = set() if rows is None else set(int(a) for a in rows)
        moved = set()
        for a, b in bad:
            a, b = int(a), int(b)
            if a in moved or b in moved:
                continue
            # prefer an atom that is neither snapped onto a face nor, in the sampled mode, a watched row
            order = sorted((a, b), key=lambda t: (t in protected) + (t in watched))
            moved.add(order[0])
        moved = np.array(sorted(moved))
        nudge = np.zeros((len(moved), 3), np.float32)
        nudge[:, list(axes)] = rng.uniform(-0.02, 0.02, (len(moved), len(axes)))
        pos32[moved] += nudge
        if rows is not None:
            r, c, d, dist, bad = rows_against_all(pos32, box, cutoffs, rows)
            ref = dict(i=r, j=c, deltas=d, dist=dist, offenders=bad)
            continue
        # the pairs of the moved atoms again, against everybody; the rest of the list stands
        r, c, d, dist, bad = rows_against_all(pos32, box, cutoffs, moved)
        stay = ~(np.isin(ref["i"], moved) | np.isin(ref["j"], moved))
        flip = r < c                                  # (a pair is stored as row > col, delta = pos[row] - pos[col])
        i = np.where(flip, c, r)
        j = np.where(flip, r, c)
        d = np.where(flip[:, None], -d, d)
        _, first = np.unique(i.astype(np.int64) * n + j, return_index=True)      # both atoms moved: listed twice
        i, j, d, dist = i[first], j[first], d[first], dist[first]
        i, j = np.concatenate([ref["i"][stay], i]), np.concatenate([ref["j"][stay], j])
        d, dist = np.concatenate([ref["deltas"][stay], d]), np.concatenate([ref["dist"][stay], dist])
        order = np.lexsort((j, i))
        ref = dict(i=i[order], j=j[order], deltas=d[order], dist=dist[order], offenders=bad)
    raise AssertionError("the inputs did not settle")


# ---------------------------------------------------------------------------------------------
# handles that say which grid they built
# ---------------------------------------------------------------------------------------------
def recording_ani(capi, seen):
    """A subclass of capi.AniSymmetryFunctions for helpers that make their own handle (test_ani_gpu.py::_run_case): the first
    compute() runs once more in front, unchecked, and keeps what that build left -- the overflow word before any check() has
    consumed it, the grid, and whether the cells were used -- in ``.first``; the instance is appended to `seen`."""
    class Recording(capi.AniSymmetryFunctions):
        def compute(self, positions, box=None, radial=None, angular=None, check=True):
            if not seen:
                seen.append(self)
                super().compute(positions, box, check=False)
                self.first = dict(word=self.overflow_word(), grid=self.read_grid(), cells=self.describe()["cells"])
            return super().compute(positions, box, radial, angular, check)

    return Recording


def recording_cfconv_neighbors(capi, seen):
    """The same for capi.CFConvNeighbors (test_cfconv_gpu.py::_case): ``.first`` is the grid of the first, unchecked build."""
    class Recording(capi.CFConvNeighbors):
        def build(self, positions, box=None, check=True):
            if not seen:
                seen.append(self)
                super().build(positions, box, check=False)
                self.first = self.read_grid()
            return super().build(positions, box, check)

    return Recording
