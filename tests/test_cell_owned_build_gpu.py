"""The one-launch build of the periodic cell grid (nnpops_amd/csrc/celllist.h: bin_atoms_owned -- every block orders the cells it
owns) against the two-launch build (bin_atoms + order_binned) of the same library.

Both must leave the SAME sorted arrays, so everything downstream is compared bit for bit: radial AEV, angular AEV, the position
gradient of a fixed random weighting, and the grid words.  There is no tolerance anywhere in this file.  The yardstick is a
handle created with NNPOPS_ANI_GRID_OWNED=0 (read once, at create); systems below the all-pairs size are forced onto the cell
search with set_neighbor_algorithm(2).  The shapes are the smallest at which the new kernel can go wrong: N no multiple of the
block, fewer cells than blocks, a ragged last block, anisotropic / tilted / barely fitting boxes, atoms on cell and box faces,
an overflowing cell range, the size threshold, graph replay, and a handle that changes build from call to call.
"""
import os
import re

import numpy as np
import pytest
import torch

import cell_geometry as cg
from nnpops_amd import workloads
from test_cell_geometry_gpu import RCA, RCR, _expected, _frame, _same_grid, _seed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nnpops_amd", "csrc", "celllist.h")


def _constant(name):
    return int(re.search(rf"constexpr int {name} = (\d+);", open(_HEADER).read()).group(1))


K_OWNED_ATOMS = _constant("kOwnedAtoms")


def _blocks(n):
    """celllist.h: owned_blocks."""
    return min(128, max(32, -(-n // 128)))


def _handle(monkeypatch, species, owned, fine=1):
    from nnpops_amd import capi
    monkeypatch.setenv("NNPOPS_ANI_GRID_OWNED", "1" if owned else "0")
    monkeypatch.setenv("NNPOPS_ANI_FINE_GRID", str(fine))
    rf, af = workloads.ani2x_functions()
    sym = capi.AniSymmetryFunctions(7, RCR, RCA, species, rf, af, periodic=True)
    sym.set_neighbor_algorithm(2)
    return sym


def _weights(sym, seed=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn((sym.num_atoms, sym.radial_width), device=DEV, generator=gen),
            torch.randn((sym.num_atoms, sym.angular_width), device=DEV, generator=gen))


def _step(sym, tpos, tbox, weights, check=True):
    radial, angular = sym.compute(tpos, tbox, check=check)
    grad = sym.backprop(*weights)
    torch.cuda.synchronize()
    return radial, angular, grad


def _equal(got, want):
    for g, w, name in zip(got, want, ("radial", "angular", "gradient")):
        assert torch.equal(g, w), name
    assert bool(torch.isfinite(want[2]).all()) and float(want[0].abs().max()) > 0


def _both(monkeypatch, pos, box, species, fine=1, build="owned"):
    """One frame through a handle of each build -> (results, grid of the handle under test); asserts equality, bit for bit."""
    tpos, tbox = torch.tensor(np.array(pos), device=DEV), torch.tensor(np.array(box), device=DEV)
    two = _handle(monkeypatch, species, owned=False, fine=fine)
    one = _handle(monkeypatch, species, owned=True, fine=fine)
    assert two.describe()["grid_build"] == "binned" and one.describe()["grid_build"] == build
    w = _weights(two)
    want = _step(two, tpos, tbox, w)
    got = _step(one, tpos, tbox, w)
    assert one.describe()["cells"] == "1" and two.describe()["cells"] == "1"
    assert one.describe()["grid_build"] == build                 # (no overflow turned it away)
    _equal(got, want)
    grid, grid_two = one.read_grid(), two.read_grid()
    assert grid == grid_two and grid["ok"] == 1 and grid["bin_overflow"] == 0, (grid, grid_two)
    return got, grid


def _species(n, *name):
    return np.random.default_rng(_seed("species", *name)).integers(0, 7, n).astype(np.int32)


def _liquid(n, seed):
    pos, species, box = workloads.random_box(n, density=0.1, seed=seed, n_species=7)
    return pos, species, box


def test_liquid_not_a_multiple_of_the_block(monkeypatch):
    """2 003 atoms, cubic, 0.1 per cubic Angstrom: the last 1 024 threads' worth of atoms is ragged; 32 blocks."""
    pos, species, box = _liquid(2003, 41)
    _, grid = _both(monkeypatch, pos, box, species)
    assert grid["m"] == 2 and grid["ncells"] > 32


def test_fewer_cells_than_blocks(monkeypatch):
    """27 full-width cells under 32 blocks: one cell each, five blocks own nothing; block 26 writes cell_start[ncells]."""
    n = 450
    rng = np.random.default_rng(_seed("owned", "cube27"))
    box = cg.on_binary_lattice(cg.ortho(3.2, 3.2, 3.2, RCR))
    pos = cg.cast_once(cg.lattice_fractions(n, np.diag(box.astype(np.float64)), rng), box.astype(np.float64))
    _, grid = _both(monkeypatch, pos, box, _species(n, "cube27"), fine=0)
    assert (grid["nx"], grid["ny"], grid["nz"], grid["m"]) == (3, 3, 3, 1) and grid["ncells"] < _blocks(n)


@pytest.mark.parametrize("tag,fine", [("tilt", 1), ("fine5", 1)])
def test_ragged_last_block(monkeypatch, tag, fine):
    """per = ceil(ncells / blocks) does not divide ncells: the last owner has a short range and still writes cell_start[ncells];
    the blocks behind it own nothing (tilt: 336 cells, 11 per block, block 30 owns 6; fine5: 400 cells, 13 per block, block 30 owns 10)."""
    frame = _frame("ani", tag)
    _, grid = _both(monkeypatch, frame["pos"], frame["box"], _species(frame["n"], tag), fine=fine)
    _same_grid(grid, _expected("ani", frame, fine))
    blocks = _blocks(frame["n"])
    per = -(-grid["ncells"] // blocks)
    assert grid["ncells"] % per != 0 and per * (blocks - 1) > grid["ncells"]


GEOMETRIES = [("ortho345", 0), ("ortho345", 1), ("ortho345_hard", 0), ("ortho345_hard", 1), ("tilt", 0), ("tilt_hard", 0),
              ("tilt_hard", 1), ("edge3+", 0), ("edge5+", 1), ("seam_blob", 0), ("seam_blob", 1)]


@pytest.mark.parametrize("tag,fine", GEOMETRIES, ids=[f"{t}-fine{f}" for t, f in GEOMETRIES])
def test_geometries(monkeypatch, tag, fine):
    """The anisotropic, tilted, barely fitting and capped boxes of cell_geometry.py / test_cell_geometry_gpu.py; the _hard frames have
    a tenth of their atoms exactly on cell faces (fraction 0 included) and every atom moved by whole box vectors (-3 .. 3)."""
    frame = _frame("ani", tag)
    _, grid = _both(monkeypatch, frame["pos"], frame["box"], _species(frame["n"], tag), fine=fine)
    _same_grid(grid, _expected("ani", frame, fine))


@pytest.mark.parametrize("fine", [0, 1])
def test_atoms_on_faces(monkeypatch, fine):
    """Coordinates exactly 0, exactly L, a hair below 0 (wraps to the last cell), a hair below L, and a hundred atoms exactly on
    faces of the cells, on every axis: each must land in the same cell in both builds."""
    pos, species, box = _liquid(2003, 43)
    pos = np.array(pos)
    L = float(box[0, 0])
    cells = int(np.floor(L / ((0.5 if fine else 1.0) * 1.0001 * RCR)))
    k = 0
    for axis in range(3):
        for value in (0.0, L, -1e-7, np.nextafter(np.float32(L), np.float32(0)), -L, 2 * L):
            pos[k, axis] = value
            k += 1
    rng = np.random.default_rng(_seed("owned", "faces", fine))
    for i in range(k, k + 100):
        axis = int(rng.integers(0, 3))
        pos[i, axis] = np.float32(round(float(pos[i, axis]) / L * cells) * L / cells)
    _, grid = _both(monkeypatch, pos, box, species, fine=fine)
    assert grid["nx"] == cells and grid["m"] == 1 + fine


def _crowded(n_blob=4600, n_gas=1800):
    """A 400 A box (capped grid: ~20 A cells) with a liquid slab of 72 x 72 x 8 A inside it: 4 x 4 cells of one layer, a span
    of under 80 consecutive cell indices (less than one block's range) holding more than twice kOwnedCap atoms -- the list of one
    of the at most two blocks that share them must overflow."""
    rng = np.random.default_rng(_seed("owned", "crowded"))
    L = 400.0
    edges = np.array([72.0, 72.0, 8.0])
    blob = cg.lattice_fractions(n_blob, edges, rng) * edges + np.array([101.0, 101.0, 103.0])
    gas = cg.lattice_fractions(n_gas, [L] * 3, rng) * L
    gas = gas[~np.all((gas > 95.0) & (gas < 180.0), axis=1)]
    pos = np.concatenate([blob, gas]).astype(np.float32)
    pos = pos[rng.permutation(len(pos))]
    return pos, np.diag([L, L, L]).astype(np.float32)


def test_overflowing_range_falls_back(monkeypatch):
    pos, box = _crowded()
    monkeypatch.setenv("NNPOPS_CELL_BIN_CAP", "512")                 # (the bins of the two-launch build: room for a 20 A cell of liquid, no growth steps)
    n = len(pos)
    species = _species(n, "crowded")
    tpos, tbox = torch.tensor(pos, device=DEV), torch.tensor(box, device=DEV)
    one = _handle(monkeypatch, species, owned=True)
    assert one.describe()["grid_build"] == "owned"
    one.compute(tpos, tbox, check=False)
    assert one.overflow_word() & 4                                   # the first, unchecked evaluation says so ...
    grid = one.read_grid()
    assert grid["bin_overflow"] == 1 and grid["ok"] == 0
    assert one.describe()["grid_build"] == "owned"
    w = _weights(one)
    got = _step(one, tpos, tbox, w)                                  # ... check() turns the handle to the two-launch build ...
    assert one.describe()["grid_build"] == "binned" and one.describe()["cells"] == "1"
    two = _handle(monkeypatch, species, owned=False)                 # ... and the results are those of a handle that never used the new one
    want = _step(two, tpos, tbox, w)
    _equal(got, want)
    assert one.read_grid() == two.read_grid() and one.read_grid()["ok"] == 1
    _equal(_step(one, tpos, tbox, w, check=False), want)             # (for good)
    assert one.describe()["grid_build"] == "binned"


@pytest.mark.parametrize("extra,build", [(0, "owned"), (1, "binned")])
def test_size_threshold(monkeypatch, extra, build):
    """N = kOwnedAtoms takes the new build, N = kOwnedAtoms + 1 the old one (low density: the grid is capped at 8 192 cells)."""
    n = K_OWNED_ATOMS + extra
    pos, species, box = workloads.random_box(n, density=0.02, seed=47 + extra, n_species=7)
    _, grid = _both(monkeypatch, pos, box, species, build=build)
    assert grid["ncells"] <= 8192


def test_graph_replay(monkeypatch):
    """compute + backprop captured once, replayed on two other frames: each replay equals the eager result of the two-launch build."""
    pos, species, box = _liquid(2003, 41)
    tbox = torch.tensor(box, device=DEV)
    one = _handle(monkeypatch, species, owned=True)
    two = _handle(monkeypatch, species, owned=False)
    w = _weights(one)
    static = torch.tensor(pos, device=DEV)
    radial = torch.empty((one.num_atoms, one.radial_width), device=DEV)
    angular = torch.empty((one.num_atoms, one.angular_width), device=DEV)
    grad = torch.empty((one.num_atoms, 3), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                           # fits the capacities
            one.compute(static, tbox, radial, angular, check=True)
            one.backprop(*w, grad)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one.compute(static, tbox, radial, angular, check=False)
        one.backprop(*w, grad)
    rng = np.random.default_rng(5)
    for _ in range(2):
        new = (pos + rng.normal(0, 0.1, pos.shape)).astype(np.float32)
        static.copy_(torch.tensor(new, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert one.overflow_word() == 0
        _equal((radial, angular, grad), _step(two, static, tbox, w))
    assert one.describe()["grid_build"] == "owned"


def test_alternating_builds(monkeypatch):
    """One handle, the build changed before every call: the histogram the two-launch build counts in must be as clean after an owned
    build as after one of its own (the consumers clear it either way)."""
    pos, species, box = _liquid(2003, 41)
    tbox = torch.tensor(box, device=DEV)
    one = _handle(monkeypatch, species, owned=True)
    two = _handle(monkeypatch, species, owned=False)
    w = _weights(one)
    rng = np.random.default_rng(7)
    for k, owned in enumerate([True, False, False, True, False, True, True, False]):
        frame = torch.tensor((pos + rng.normal(0, 0.1, pos.shape)).astype(np.float32), device=DEV)
        one.set_grid_build(owned)
        assert one.describe()["grid_build"] == ("owned" if owned else "binned")
        _equal(_step(one, frame, tbox, w, check=k == 0), _step(two, frame, tbox, w))
        assert one.overflow_word() == 0 and one.read_grid() == two.read_grid()
