"""The cell grid (nnpops_amd/csrc/celllist.h) in boxes that are anisotropic, tilted, barely wide enough, capped or flat.

Every other GPU test that walks a grid does so in a cube or in one mildly tilted cell with equal diagonals, where an exchange
of nx / ny / nz, a width taken from the box diagonal, or an off-by-one in a stencil that covers an axis exactly once would go
unseen.  Here each of the three consumers -- the ANI neighbour rows, the CFConv half list, getNeighborPairs -- walks

    ortho345    diag(3.2, 4.3, 5.4) c          three different cell counts per axis
    fine5       diag(2.6, 4.3, 5.4) c          exactly 5 half-width cells along x, where full-width cells would be 2 (refused)
    tilt        off-diagonals +-0.45           perpendicular widths well below the diagonals: fewer cells than the diagonals say
    edge3+-     x width 3.001 c / 2.999 c      exactly 3 full-width cells / refused, falls back to the all-pairs search
    edge5+-     x width 2.51 c / 2.49 c        exactly 5 half-width cells / refused
    seam_blob   a cube of (L/c)^3 > the cap    coarsened, unequal dims; all atoms in a blob on the box corner, across all three seams
    sheet, rod, dumbbell (no box)              nz = 1; a 40:4:1 bounding box; two far blobs: empty cells and the cap

(c: the consumer's grid cutoff; getNeighborPairs stretches y and z so that its 8 200 atoms stay near liquid density) and says
through the read_grid accessors which grid it walked: a case whose grid is not the one it claims FAILS.  ortho345 and tilt run a
second time with a tenth of the atoms exactly on cell faces and every atom moved by whole box vectors.  References: the oracles
of test_ani_gpu.py / test_cfconv_gpu.py with their assertions and bars, and for getNeighborPairs a float64 brute force over all
pairs (cell_geometry.py); each walked ANI / getNeighborPairs case is also compared with the same handle / op on its all-pairs path.
The inputs are made so that, in float64, no pair is within 1e-5 cutoff of a cutoff and no candidate pair hangs on how a
half-integer rounds (asserted before anything is launched): the lists are compared exactly.  Seeds are the CRC-32 of the case name.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import cell_geometry as cg
from nnpops_amd import workloads
from oracle import neighbor_pairs_backward_oracle
from test_ani_gpu import AEV_ATOL, AEV_RTOL, _run_case as ani_run_case
from test_cfconv_gpu import _case as cfconv_run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

RCR, RCA = 5.1, 3.5                       # ANI-2x: the grid is built for the radial cutoff
ATOMS = {"ani": 600, "cfconv": 1100, "pairs": 8200}
PAIRS_CUTOFF = 5.0
BLOB_CELLS = {"ani": 18.5, "cfconv": 18.5, "pairs": 22.5}          # seam_blob: box edge in cutoffs, (edge / c)^3 above the cap
X_WIDTH = {"ortho345": 3.2, "fine5": 2.6, "edge3+": 3.001, "edge3-": 2.999, "edge5+": 2.51, "edge5-": 2.49}
OPEN = ("sheet", "rod", "dumbbell")


def _seed(*name):
    return zlib.crc32("/".join(str(x) for x in name).encode())


def _box_in_cutoffs(consumer, tag):
    """The periodic cell of a case in units of the consumer's cutoff (float64 rows)."""
    base = tag.replace("_hardx", "").replace("_hard", "")
    if base == "seam_blob":
        return cg.ortho(*[BLOB_CELLS[consumer]] * 3, 1.0)
    if base == "tilt":
        return cg.tilted(4.05, 10.1, 19.9) if consumer == "pairs" else cg.tilted(4.05, 4.05, 4.05)
    if base == "ortho16k":                                   # getNeighborPairs above 16 384 atoms
        return cg.ortho(3.2, 14.3, 28.9, 1.0)
    x = X_WIDTH[base]
    if consumer == "pairs":                                  # x as tabled, y and z stretched: 8 200 atoms near 0.1 per cubic Angstrom
        return cg.ortho(x, 10.3, int(656.0 / (x * 10.3)) + 0.3, 1.0)
    return cg.ortho(x, 4.3, 5.4, 1.0)


def _max_cells(consumer, n, periodic, fine):
    """The cap decide_grid is given: N + 4096, and 8 192 where the two-launch (binned) build holds the grid."""
    binned = periodic and (n <= 65536 if consumer != "pairs" else n <= (16384 if fine else 200000))
    return min(n + 4096, 8192) if binned else n + 4096


@functools.lru_cache(maxsize=None)
def _frame(consumer, tag):
    """-> dict(pos float32 [N, 3], box float32 [3, 3] or None, cutoff, widths, ref): made once per case and shared, never changed.
    ref: the float64 pair list of cell_geometry.reference_pairs (for getNeighborPairs above 16 384 atoms: of 500 sampled rows)."""
    rng = np.random.default_rng(_seed(consumer, tag))
    n = 16500 if tag == "ortho16k" else ATOMS[consumer]
    base = tag.replace("_hardx", "").replace("_hard", "")
    snapped = ()
    if base in OPEN:
        cutoff = {"ani": RCR, "cfconv": 5.0, "pairs": PAIRS_CUTOFF}[consumer]
        pos = cg.open_cloud(base, n, rng, far=150.0 if consumer == "pairs" else 110.0).astype(np.float32)
        box = None
        widths = cg.open_extent(pos)
    else:
        unit = _box_in_cutoffs(consumer, tag)
        if consumer == "cfconv":                             # the cutoff is free: liquid density in the tabled cell
            cutoff = 5.0 if base == "seam_blob" else float(np.float32((n / (0.1 * abs(np.linalg.det(unit)))) ** (1.0 / 3.0)))
        else:
            cutoff = RCR if consumer == "ani" else PAIRS_CUTOFF
        box = cg.on_binary_lattice(unit * cutoff)            # what the device is given; everything below starts from these numbers
        box64 = box.astype(np.float64)
        widths = cg.perpendicular_widths(box64)
        if base == "seam_blob":
            pos = cg.corner_blob(n, rng).astype(np.float32)
        else:
            frac = cg.lattice_fractions(n, np.linalg.norm(box64, axis=1), rng)
            if "_hard" in tag:                                # (_hardx: whole multiples of the short x vector only)
                coarse = [max(1, int(w / (1.0001 * cutoff))) for w in widths]
                fine = [max(1, int(w / (0.50005 * cutoff))) for w in widths]
                frac, snapped = cg.harden(frac, coarse, fine, rng, vectors=(0,) if tag.endswith("_hardx") else (0, 1, 2))
            pos = cg.cast_once(frac, box64)
    cutoffs = [RCR, RCA] if consumer == "ani" else [cutoff]
    rows = rng.choice(n, 500, replace=False) if tag == "ortho16k" else None
    pos, ref = cg.settle(pos, box, cutoffs, rng, protected=snapped, rows=rows, axes=(0, 1) if base == "sheet" else (0, 1, 2))
    pos.setflags(write=False)
    return dict(pos=pos, box=box, cutoff=cutoff, widths=widths, ref=ref, rows=rows, n=n)


def _check_inputs(frame):
    """The conditions on the inputs, on the CPU, before anything is launched."""
    assert len(frame["ref"]["offenders"]) == 0                       # no pair at a cutoff, no candidate at a half-integer (float64)
    if frame["box"] is not None:
        assert np.all(frame["widths"] >= 2 * frame["cutoff"])         # the reference's contract


def _expected(consumer, frame, fine):
    periodic = frame["box"] is not None
    return cg.grid_for(frame["widths"], frame["cutoff"], _max_cells(consumer, frame["n"], periodic, fine), fine, periodic)


def _same_grid(got, want):
    assert {k: got[k] for k in want} == want, (got, want)
    assert got["bin_overflow"] == 0


def _claim(want, dims, m, ok):
    """The grid the case is about, spelled out: the host restatement must agree before the device is asked."""
    assert (want["nx"], want["ny"], want["nz"], want["m"], want["ok"]) == (*dims, m, ok), want


def _open_dims(consumer, frame, want, tag):
    """Open clouds: the dims follow the bounding box of the atoms; what makes each shape the case it is, is asserted here."""
    dims = (want["nx"], want["ny"], want["nz"])
    pos = frame["pos"]
    if tag == "sheet":                                           # flat: every z the same number, one layer of cells from the pad alone
        assert np.all(pos[:, 2] == pos[0, 2]) and want["nz"] == 1
    if tag == "rod":
        assert want["nx"] >= 8 * want["ny"]
    if tag == "dumbbell":                                        # the bounding-box grid is past the cap, at either cell width
        full = np.floor(frame["widths"] / (1.0001 * frame["cutoff"]))
        assert full.prod() > _max_cells(consumer, frame["n"], False, 0) and want["m"] == 1
        assert want["ncells"] < full.prod() and len(set(dims)) > 1      # coarsened, and to unequal dims
    return dims


# ---------------------------------------------------------------------------------------------
# ANI neighbour rows
# ---------------------------------------------------------------------------------------------
# (tag, fine, fused, claimed dims, m, ok)
ANI_CASES = [
    ("ortho345", 0, 0, (3, 4, 5), 1, 1), ("ortho345", 0, 1, (3, 4, 5), 1, 1),
    ("ortho345", 1, 0, (6, 8, 10), 2, 1), ("ortho345", 1, 1, (6, 8, 10), 2, 1),
    ("ortho345_hard", 0, 1, (3, 4, 5), 1, 1), ("ortho345_hard", 1, 0, (6, 8, 10), 2, 1),
    ("fine5", 1, 0, (5, 8, 10), 2, 1), ("fine5", 1, 1, (5, 8, 10), 2, 1), ("fine5", 0, 1, (2, 4, 5), 1, 0),
    ("tilt", 0, 0, (3, 3, 4), 1, 1), ("tilt", 0, 1, (3, 3, 4), 1, 1), ("tilt", 1, 0, (6, 7, 8), 2, 1), ("tilt", 1, 1, (6, 7, 8), 2, 1),
    ("tilt_hard", 0, 0, (3, 3, 4), 1, 1), ("tilt_hard", 1, 1, (6, 7, 8), 2, 1),
    ("edge3+", 0, 0, (3, 4, 5), 1, 1), ("edge3+", 0, 1, (3, 4, 5), 1, 1), ("edge3-", 0, 0, (2, 4, 5), 1, 0),
    ("edge5+", 1, 0, (5, 8, 10), 2, 1), ("edge5+", 1, 1, (5, 8, 10), 2, 1), ("edge5-", 1, 1, (2, 4, 5), 1, 0),
    ("seam_blob", 1, 0, (15, 15, 18), 1, 1), ("seam_blob", 0, 1, (15, 15, 18), 1, 1),
    ("sheet", 0, 0, None, 1, 1), ("sheet", 1, 1, None, 2, 1), ("rod", 0, 1, None, 1, 1), ("rod", 1, 0, None, 2, 1),
    ("dumbbell", 1, 0, None, 1, 1), ("dumbbell", 0, 1, None, 1, 1),
]


@pytest.mark.parametrize("tag,fine,fused,dims,m,ok", ANI_CASES, ids=[f"{c[0]}-fine{c[1]}-fuse{c[2]}" for c in ANI_CASES])
def test_ani_rows(monkeypatch, tag, fine, fused, dims, m, ok):
    """The assertions and bars of test_ani_gpu.py (AEV 2e-5 / 2e-6, energy 1e-5, forces 1e-4 of the largest component against
    oracle.AniOracle) on a handle that proves which grid it walked.  NNPOPS_ANI_FINE_GRID picks the 3x3x3 or the 5x5x5 stencil,
    NNPOPS_ANI_FUSE the fused build+forward or the two-launch build (both read at handle creation).  Walked cases force the grid
    (algorithm 2) and show bit 1 of the overflow word clear; refused ones (ok = 0) lower the automatic threshold to their size,
    show the bit before check() consumes it, and end on the all-pairs search."""
    from nnpops_amd import capi
    frame = _frame("ani", tag)
    _check_inputs(frame)
    want = _expected("ani", frame, fine)
    if dims is None:
        dims = _open_dims("ani", frame, want, tag)
    _claim(want, dims, m, ok)
    monkeypatch.setenv("NNPOPS_ANI_FINE_GRID", str(fine))
    monkeypatch.setenv("NNPOPS_ANI_FUSE", str(fused))
    if not ok:
        monkeypatch.setenv("NNPOPS_ANI_CELL_ATOMS", "256")
    seen = []
    monkeypatch.setattr(capi, "AniSymmetryFunctions", cg.recording_ani(capi, seen))      # (the first build, before any check())
    rng = np.random.default_rng(_seed("species", tag))
    species = rng.integers(0, 7, frame["n"]).astype(np.int32)
    rf, af = workloads.ani2x_functions()
    pos, box = np.array(frame["pos"]), frame["box"]
    r, a, _ = ani_run_case(7, RCR, RCA, species, rf, af, pos, box, algorithm=2 if ok else 0)
    sym, = seen
    assert sym.first["cells"] == "1"
    _same_grid(sym.first["grid"], want)
    assert sym.describe()["fused_build"] == str(fused)
    if not ok:
        assert sym.first["word"] & 2 and sym.describe()["cells"] == "0"
        return
    assert not sym.first["word"] & 2 and sym.describe()["cells"] == "1"
    _same_grid(sym.read_grid(), want)
    # second witness: the same handle on the all-pairs search, same frame
    stats = sym.neighbor_stats()
    sym.set_neighbor_algorithm(1)
    tpos = torch.tensor(pos, device=DEV)
    r1, a1 = sym.compute(tpos, None if box is None else torch.tensor(box, device=DEV))
    assert sym.describe()["cells"] == "0" and sym.neighbor_stats() == stats
    np.testing.assert_allclose(r, r1.cpu().numpy(), rtol=AEV_RTOL, atol=AEV_ATOL)
    np.testing.assert_allclose(a, a1.cpu().numpy(), rtol=AEV_RTOL, atol=AEV_ATOL)


# ---------------------------------------------------------------------------------------------
# CFConv half list (no half-width grid: fine5 is a refusal here)
# ---------------------------------------------------------------------------------------------
# (tag, width, gaussians, claimed dims, ok)
CFCONV_CASES = [
    ("ortho345", 16, 7, (3, 4, 5), 1), ("ortho345", 64, 25, (3, 4, 5), 1), ("ortho345_hard", 16, 7, (3, 4, 5), 1),
    ("fine5", 16, 7, (2, 4, 5), 0), ("tilt", 16, 7, (3, 3, 4), 1), ("tilt_hard", 16, 7, (3, 3, 4), 1),
    ("edge3+", 16, 7, (3, 4, 5), 1), ("edge3-", 16, 7, (2, 4, 5), 0), ("seam_blob", 16, 7, (15, 18, 18), 1),
    ("sheet", 16, 7, None, 1), ("rod", 16, 7, None, 1), ("dumbbell", 16, 7, None, 1),
]


@pytest.mark.parametrize("tag,W,G,dims,ok", CFCONV_CASES, ids=[f"{c[0]}-W{c[1]}" for c in CFCONV_CASES])
def test_cfconv_list(monkeypatch, tag, W, G, dims, ok):
    """The assertions and bars of test_cfconv_gpu.py -- the exact pair list and distances of CFConvNeighborsOracle, outputs and
    gradients of CFConvOracle -- at 1 100 atoms (the grid is taken from 1 024 on; there is no switch).  Refused boxes (ok = 0) go
    through check(): cells disabled, rebuilt with the all-pairs rows."""
    from nnpops_amd import capi
    frame = _frame("cfconv", tag)
    _check_inputs(frame)
    want = _expected("cfconv", frame, 0)
    if dims is None:
        dims = _open_dims("cfconv", frame, want, tag)
    _claim(want, dims, 1, ok)
    seen = []
    monkeypatch.setattr(capi, "CFConvNeighbors", cg.recording_cfconv_neighbors(capi, seen))
    cfconv_run_case(np.array(frame["pos"]), frame["box"], W, G, frame["cutoff"], 0.4, "ssp", seed=_seed("weights", tag) % 1000)
    nb, = seen
    _same_grid(nb.first, want)
    _same_grid(nb.read_grid(), want)             # (a refused grid stays as the refused build left it: the all-pairs rows build none)


# ---------------------------------------------------------------------------------------------
# getNeighborPairs
# ---------------------------------------------------------------------------------------------
def _pairs(frame, dtype, max_num_pairs, return_grid=True):
    from nnpops_amd.capi import neighbor_pairs_forward
    tp = torch.tensor(np.array(frame["pos"]), dtype=dtype, device=DEV)
    tb = None if frame["box"] is None else torch.tensor(frame["box"], dtype=dtype, device=DEV)
    out = neighbor_pairs_forward(tp, frame["cutoff"], max_num_pairs, tb, return_grid=return_grid)
    torch.cuda.synchronize()
    return out


def _listed(nb, dl, ds):
    """The used slots of a list on the host, sorted by (row, col)."""
    used = nb[0] >= 0
    nb, dl, ds = nb[:, used].cpu().numpy(), dl[used].cpu().numpy(), ds[used].cpu().numpy()
    order = np.lexsort((nb[1], nb[0]))
    return nb[:, order], dl[order], ds[order]


def _compare_with_reference(got, ref, dtype):
    nb, dl, ds = got
    assert np.array_equal(nb[0], ref["i"]) and np.array_equal(nb[1], ref["j"])          # the same set of (i, j)
    f32 = dtype == torch.float32
    print("max |distance error| / distance", float(np.max(np.abs(ds - ref["dist"]) / ref["dist"])),
          "max |delta error|", float(np.max(np.abs(dl - ref["deltas"]))))
    np.testing.assert_allclose(ds, ref["dist"], rtol=2e-5 if f32 else 1e-12)
    np.testing.assert_allclose(dl, ref["deltas"], rtol=2e-5 if f32 else 1e-12, atol=1e-5 if f32 else 1e-12)


# (tag, dtype, fine, claimed dims, m, ok)
F32, F64 = torch.float32, torch.float64
PAIRS_CASES = [
    ("ortho345", F32, 1, (6, 20, 38), 2, 1), ("ortho345", F64, 1, (6, 20, 38), 2, 1),
    ("ortho345", F32, 0, (3, 10, 19), 1, 1), ("ortho345", F64, 0, (3, 10, 19), 1, 1),
    ("ortho345_hard", F64, 1, (6, 20, 38), 2, 1), ("ortho345_hard", F64, 0, (3, 10, 19), 1, 1),
    ("ortho345_hardx", F32, 1, (6, 20, 38), 2, 1), ("ortho345_hardx", F32, 0, (3, 10, 19), 1, 1),
    ("fine5", F32, 1, (5, 20, 48), 2, 1), ("fine5", F64, 1, (5, 20, 48), 2, 1), ("fine5", F32, 0, (2, 10, 24), 1, 0),
    ("tilt", F32, 1, (7, 19, 39), 2, 1), ("tilt", F64, 1, (7, 19, 39), 2, 1), ("tilt", F32, 0, (3, 9, 19), 1, 1), ("tilt", F64, 0, (3, 9, 19), 1, 1),
    ("tilt_hard", F64, 1, (7, 19, 39), 2, 1), ("tilt_hard", F64, 0, (3, 9, 19), 1, 1),
    ("edge3+", F32, 0, (3, 10, 21), 1, 1), ("edge3-", F32, 0, (2, 10, 21), 1, 0), ("edge3-", F64, 0, (2, 10, 21), 1, 0),
    ("edge5+", F32, 1, (5, 20, 50), 2, 1), ("edge5+", F64, 1, (5, 20, 50), 2, 1), ("edge5-", F32, 1, (2, 10, 25), 1, 0),
    ("seam_blob", F32, 1, (19, 19, 22), 1, 1), ("seam_blob", F64, 0, (19, 19, 22), 1, 1),
    ("sheet", F32, 1, None, 2, 1), ("sheet", F64, 0, None, 1, 1), ("rod", F32, 0, None, 1, 1), ("rod", F64, 1, None, 2, 1),
    ("dumbbell", F32, 1, None, 1, 1), ("dumbbell", F64, 0, None, 1, 1),
]


@pytest.mark.parametrize("tag,dtype,fine,dims,m,ok", PAIRS_CASES,
                         ids=[f"{c[0]}-{'f32' if c[1] == F32 else 'f64'}-fine{c[2]}" for c in PAIRS_CASES])
def test_pairs_list(monkeypatch, tag, dtype, fine, dims, m, ok):
    """8 200 atoms, a compacted list: the set of (i, j) and num_pairs equal to the float64 brute force over ALL pairs, deltas and
    distances inside the bars of test_neighbor_pairs_gpu.py::test_periodic (2e-5 / 1e-5 absolute in float32, 1e-12 in float64;
    the float64 run is given the same float32-representable numbers).  The default half-width grid and NNPOPS_PAIRS_FINE_GRID=0.
    The hard frames run in float64 (where the grid is still built from the float32 copy of the positions): atoms up to six
    boxes apart differ by up to 600 A, and one float32 rounding of such a difference (ulp 6e-5 A) is past the 1e-5 A bar.
    In float32 the hard inputs are ortho345_hardx: the same snapped atoms, moved by whole multiples of the 16 A x vector only
    (differences below 128 A: half an ulp is 3.8e-6 A).
    Refused grids (ok = 0) must scan every column of every row and still be right.  Every walked case is also compared with the
    op's own all-pairs kernel (max_num_pairs = -1) on the same frame."""
    frame = _frame("pairs", tag)
    _check_inputs(frame)
    want = _expected("pairs", frame, fine)
    if dims is None:
        dims = _open_dims("pairs", frame, want, tag)
    _claim(want, dims, m, ok)
    if not fine:
        monkeypatch.setenv("NNPOPS_PAIRS_FINE_GRID", "0")
    ref = frame["ref"]
    found = len(ref["i"])
    nb, dl, ds, count, grid = _pairs(frame, dtype, found + 1000)
    _same_grid(grid, want)
    assert int(count) == found
    assert bool((nb[:, found:] == -1).all()) and bool(torch.isnan(ds[found:]).all())
    rows = nb[0, :found].cpu().numpy()
    assert np.all(np.diff(rows) >= 0)                                    # grouped by row, ascending
    got = _listed(nb, dl, ds)
    _compare_with_reference(got, ref, dtype)
    if ok:                                                               # second witness: the all-pairs kernel, every slot
        nb1, dl1, ds1, count1 = _pairs(frame, dtype, -1, return_grid=False)[:4]
        one = _listed(nb1, dl1, ds1)
        assert int(count1) == found and np.array_equal(one[0], got[0])


def test_pairs_list_above_the_binned_build(monkeypatch):
    """16 500 atoms in diag(3.2, 14.3, 28.9) c: past the two-launch build, so grid_setup .. order_cells with the tiled scan
    (9 576 half-width cells: more than one tile of 8 192).  The full scan is too large for a test: 500 sampled rows against all
    atoms in float64, and the identities of test_large_system_cell_grid on the whole list."""
    frame = _frame("pairs", "ortho16k")
    _check_inputs(frame)
    want = _expected("pairs", frame, 1)
    _claim(want, (6, 28, 57), 2, 1)
    assert want["ncells"] > 8192
    max_pairs = 30 * frame["n"]
    nb, dl, ds, count, grid = _pairs(frame, F32, max_pairs)
    _same_grid(grid, want)
    found = int(count)
    assert 0 < found < max_pairs
    nb, dl, ds = nb.cpu().numpy(), dl.cpu().numpy(), ds.cpu().numpy()
    valid = nb[0] >= 0
    assert int(valid.sum()) == found and np.all(valid[:found]) and np.all(nb[0][valid] > nb[1][valid])
    assert np.all(np.diff(nb[0][:found]) >= 0)
    np.testing.assert_allclose(np.sqrt((dl[valid].astype(np.float64) ** 2).sum(1)), ds[valid], rtol=1e-6)
    # the sampled rows: every partner with a smaller index must be listed under the row, every one with a larger index under
    # the partner -- the same (i, j) as the float64 scan, no more and no fewer
    ref = frame["ref"]
    sample = np.isin(nb[0][:found], frame["rows"]) | np.isin(nb[1][:found], frame["rows"])
    got = set(zip(nb[0][:found][sample].tolist(), nb[1][:found][sample].tolist()))
    expect = set((max(i, j), min(i, j)) for i, j in zip(ref["i"].tolist(), ref["j"].tolist()))
    assert got == expect
    lower = ref["i"] > ref["j"]
    watched = set(frame["rows"].tolist())
    key = {(i, j): k for k, (i, j) in enumerate(zip(nb[0][:found].tolist(), nb[1][:found].tolist())) if i in watched}
    at = np.array([key[(int(i), int(j))] for i, j in zip(ref["i"][lower], ref["j"][lower])])
    np.testing.assert_allclose(ds[at], ref["dist"][lower], rtol=2e-5)
    np.testing.assert_allclose(dl[at], ref["deltas"][lower], rtol=2e-5, atol=1e-5)


@pytest.mark.parametrize("tag,dtype", [("ortho345", F32), ("tilt", F64)])
def test_pairs_torch_op_backward(tag, dtype):
    """The same frames through torch.ops' getNeighborPairs with positions that require a gradient: the list is the reference's,
    and the backward -- the owner-computes gather over the list's transposed index -- is neighbor_pairs_backward_oracle's on that
    list (bars of test_neighbor_pairs_gpu.py::test_backward_indexed)."""
    from NNPOps.neighbors import getNeighborPairs
    frame = _frame("pairs", tag)
    _check_inputs(frame)
    ref = frame["ref"]
    found = len(ref["i"])
    p = torch.tensor(np.array(frame["pos"]), dtype=dtype, device=DEV, requires_grad=True)
    box = torch.tensor(frame["box"], dtype=dtype, device=DEV)
    nb, deltas, dist, count = getNeighborPairs(p, cutoff=frame["cutoff"], max_num_pairs=found + 1000, box_vectors=box)
    assert int(count) == found
    _compare_with_reference(_listed(nb.detach(), deltas.detach(), dist.detach()), ref, dtype)
    npdt = np.float32 if dtype == F32 else np.float64
    rng = np.random.default_rng(_seed("grad", tag))
    gd = rng.standard_normal(tuple(deltas.shape)).astype(npdt)
    gs = rng.standard_normal(tuple(dist.shape)).astype(npdt)
    used = nb[0] >= 0
    ((deltas[used] * torch.tensor(gd, device=DEV)[used]).sum() + (dist[used] * torch.tensor(gs, device=DEV)[used]).sum()).backward()
    want = neighbor_pairs_backward_oracle(frame["n"], nb.cpu().numpy(), deltas.detach().cpu().numpy(), dist.detach().cpu().numpy(), gd, gs)
    tol = 1e-5 if dtype == F32 else 1e-12
    np.testing.assert_allclose(p.grad.cpu().numpy(), want, rtol=tol, atol=tol * np.abs(want).max())
