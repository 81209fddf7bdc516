"""The per-atom ANI kernels take their launch shape as arguments (no blockDim / gridDim), walk the XCD-contiguous order through a
closed form, and clear the cell histogram only behind a two-launch grid build (nnpops_amd/csrc/device_common.h, celllist.h).

None of that changes a kernel's arithmetic, so what can go wrong is index arithmetic -- a wave id that is no longer a bijection
skips an atom or takes one twice -- and the invariant "the histogram is zero between evaluations".  The shapes are the smallest
at which those show:

    1  every atom exactly once: periodic 7-species boxes of 1 801, 1 803, 2 003 and 2 050 atoms at 0.1 per cubic Angstrom (the
       cell path starts at 1 800; workgroup counts that are no multiple of 8, atom counts that are no multiple of the waves per
       workgroup) and molecules of 50 and 115 atoms (all pairs), outputs filled with NaN before the call
    2  paths that must agree on the 2 003-atom box: the two grid builds bit for bit, cell search against all pairs, call against call
    3  the histogram: a handle that changes build from call to call, an owned build driven into overflow, graphs replayed behind an
       eager call of the other build, the fused build + forward kernel
    4  the other instantiations whose index arithmetic changed, each on its smallest reachable shape

The float64 judge is ani_float64.Restatement (the box and molecule frames of this file, one evaluation each, kept for the module)
and, for the frames test_ani_dispatch_gpu.py already judges, that module's AniOracle64 references; the bars are that module's
(_judge: AEV 2e-5 relative + 2e-6 of the largest element, energies 1e-5, forces 1e-4 of the largest component).  Everything else is
compared bit for bit.  No accessor exposes the histogram words themselves: a histogram left dirty shows as a bin overflow or other
sorted arrays in the next two-launch build, which is what the bit comparisons of section 3 look at, together with read_grid().
"""
import functools

import numpy as np
import pytest
import torch

from ani_float64 import Restatement, weights
from nnpops_amd import workloads
from test_ani_dispatch_gpu import AEV_ATOL, AEV_RTOL, FORCE_RTOL, _evaluate, _judge, _reference
from test_ani_dispatch_gpu import _system as _dispatch_system
from test_cell_owned_build_gpu import _crowded, _equal, _species, _step, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RCR, RCA = 5.1, 3.5


@functools.lru_cache(maxsize=None)
def _frame(tag):
    """-> (species, pos, box or None), read-only"""
    kind, n = tag.split("-")
    n = int(n)
    if kind == "box":
        pos, species, box = workloads.random_box(n, density=0.1, seed=900 + n % 97, n_species=7)
    else:
        pos, species = workloads.conformer(n, seed=900 + n)
        box = None
    for a in (species, pos, box):
        if a is not None:
            a.setflags(write=False)
    return species, pos, box


@functools.lru_cache(maxsize=None)
def _float64(tag):
    """The restatement's AEV and forces of a frame under seeded weights, once per module: dict(r, a, g, wr, wa) as _judge reads it."""
    species, pos, box = _frame(tag)
    rf, af = workloads.ani2x_functions()
    judge = Restatement(7, RCR, RCA, species, rf, af, torchani=True)
    n = len(species)
    wr, wa = weights((n, 7 * judge.nR), (n, judge.NB * judge.nA), seed=n)
    if n > 4000:      # (the restatement holds [N, N, 3] arrays: the larger frame goes to the C restatement in double, which agrees with it to 1e-14)
        from oracle import AniOracle64
        oracle = AniOracle64(7, RCR, RCA, species, rf, af, periodic=True, torchani=True)
        r, a = oracle.forward(pos, box)
        return dict(r=r, a=a, g=oracle.backward(wr, wa), wr=wr, wa=wa)
    # (a molecule: a box far wider than the molecule and both cutoffs gives the restatement zero shifts everywhere)
    box64 = box if box is not None else np.diag([1e4, 1e4, 1e4]).astype(np.float32)
    out = judge.evaluate(pos, box64, wr, wa)
    return dict(r=out["r"], a=out["a"], g=out["g"], wr=wr, wa=wa)


def _make(monkeypatch, species, periodic, env=None):
    from nnpops_amd import capi
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    rf, af = workloads.ani2x_functions()
    sym = capi.AniSymmetryFunctions(7, RCR, RCA, species, rf, af, periodic=periodic)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return sym


def _nan_step(sym, pos, box, ref):
    """compute + backprop into NaN-filled arrays -> (radial, angular, gradient) as numpy; a second backprop must give the same bits"""
    n = len(pos)
    tpos = torch.tensor(np.array(pos), device=DEV)
    tbox = torch.tensor(np.array(box), device=DEV) if box is not None else None
    nan = float("nan")
    radial = torch.full((n, sym.radial_width), nan, device=DEV)
    angular = torch.full((n, sym.angular_width), nan, device=DEV)
    sym.compute(tpos, tbox, radial, angular, check=True)
    radial.fill_(nan); angular.fill_(nan)
    sym.compute(tpos, tbox, radial, angular, check=False)          # (capacities fitted: this evaluation writes every row by itself)
    t_wr, t_wa = torch.tensor(ref["wr"], device=DEV), torch.tensor(ref["wa"], device=DEV)
    grad = torch.full((n, 3), nan, device=DEV)
    sym.backprop(t_wr, t_wa, grad)
    again = torch.full((n, 3), nan, device=DEV)
    sym.backprop(t_wr, t_wa, again)
    torch.cuda.synchronize()
    for name, x in (("radial", radial), ("angular", angular), ("gradient", grad)):
        assert not bool(torch.isnan(x).any()), f"{name}: {int(torch.isnan(x).any(dim=1).sum())} rows were not written"
    assert torch.equal(grad, again)
    return radial.cpu().numpy(), angular.cpu().numpy(), grad.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. every atom exactly once
# (box-8203: above 8 192 atoms the radial backward runs its occupancy variant, the one of the 10 000-atom headline; 2 051 workgroups)
@pytest.mark.parametrize("tag", ["box-1801", "box-1803", "box-2003", "box-2050", "box-8203", "mol-50", "mol-115"])
def test_every_atom_exactly_once(monkeypatch, tag):
    species, pos, box = _frame(tag)
    sym = _make(monkeypatch, species, box is not None)
    ref = _float64(tag)
    r, a, g = _nan_step(sym, pos, box, ref)
    what = sym.describe()
    assert what["cells"] == ("1" if box is not None else "0"), what
    if box is not None:      # (the compact molecules have 64 and 128 record slots: two waves per atom, and the row kernel as radial backward at 128)
        assert what["grid_build"] == "owned" and what["radial_bwd"] == "lanes" and what["cap_angular"] == "32", what
        n = len(species)
        assert n % 4 != 0 or (n // 4) % 8 != 0                   # (radial backward: four waves per workgroup, ceil(n / 4) workgroups)
    _judge(f"prologue 1 {tag}", ref, r, a, g)


# ---------------------------------------------------------------------------------------------- 2. paths that must agree
def test_paths_that_must_agree(monkeypatch):
    tag = "box-2003"
    species, pos, box = _frame(tag)
    ref = _float64(tag)
    tpos, tbox = torch.tensor(np.array(pos), device=DEV), torch.tensor(np.array(box), device=DEV)
    owned = _make(monkeypatch, species, True, {"NNPOPS_ANI_GRID_OWNED": "1"})
    binned = _make(monkeypatch, species, True, {"NNPOPS_ANI_GRID_OWNED": "0"})
    pairs = _make(monkeypatch, species, True)
    pairs.set_neighbor_algorithm(1)
    w = (torch.tensor(ref["wr"], device=DEV), torch.tensor(ref["wa"], device=DEV))
    got = _step(owned, tpos, tbox, w)
    assert owned.describe()["grid_build"] == "owned" and owned.describe()["cells"] == "1"
    want = _step(binned, tpos, tbox, w)
    assert binned.describe()["grid_build"] == "binned" and binned.describe()["cells"] == "1"
    _equal(got, want)                                             # the two builds, bit for bit
    assert owned.read_grid() == binned.read_grid()
    _equal(_step(owned, tpos, tbox, w, check=False), got)         # call against call, one handle
    _equal(_step(binned, tpos, tbox, w, check=False), want)
    other = _step(pairs, tpos, tbox, w)                           # another row order, another summation order: the family's bars
    assert pairs.describe()["cells"] == "0"
    for x, y in zip(got[:2], other[:2]):
        x, y = x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)
        assert bool((np.abs(x - y) <= AEV_RTOL * np.abs(y) + AEV_ATOL * max(1.0, float(np.abs(y).max()))).all())
    gx, gy = got[2].cpu().numpy().astype(np.float64), other[2].cpu().numpy().astype(np.float64)
    assert float(np.abs(gx - gy).max()) <= FORCE_RTOL * float(np.abs(gy).max())
    _judge("prologue 2 all pairs", ref, *(t.cpu().numpy() for t in other))


# ---------------------------------------------------------------------------------------------- 3. the histogram invariant
def _moved(pos, rng):
    return torch.tensor((np.array(pos) + rng.normal(0, 0.1, np.shape(pos))).astype(np.float32), device=DEV)


@pytest.mark.parametrize("fused", ["0", "1"], ids=["two_kernels", "fused_build_forward"])
def test_builds_alternate_on_one_handle(monkeypatch, fused):
    """owned, binned, owned, owned, binned, binned, owned with fresh positions: every call equals, bit for bit, a handle that only ever
    ran that call's build.  (A histogram the owned build's consumer had left dirty -- or one a binned build's consumer had NOT
    cleared -- gives the next binned build other counts: a bin overflow, or other sorted arrays.)"""
    species, pos, box = _frame("box-2003")
    tbox = torch.tensor(np.array(box), device=DEV)
    env = {"NNPOPS_ANI_FUSE": fused}
    one = _make(monkeypatch, species, True, dict(env, NNPOPS_ANI_GRID_OWNED="1"))
    only = {True: _make(monkeypatch, species, True, dict(env, NNPOPS_ANI_GRID_OWNED="1")),
            False: _make(monkeypatch, species, True, dict(env, NNPOPS_ANI_GRID_OWNED="0"))}
    w = _weights(one)
    rng = np.random.default_rng(11)
    for k, owned in enumerate([True, False, True, True, False, False, True]):
        frame = _moved(pos, rng)
        one.set_grid_build(owned)
        assert one.describe()["grid_build"] == ("owned" if owned else "binned")
        got = _step(one, frame, tbox, w, check=k == 0)
        assert one.describe()["fused_build"] == fused and one.describe()["cells"] == "1", one.describe()
        _equal(got, _step(only[owned], frame, tbox, w))
        grid = one.read_grid()
        assert one.overflow_word() == 0 and grid == only[owned].read_grid() and grid["ok"] == 1 and grid["bin_overflow"] == 0, grid


def test_owned_build_driven_into_overflow(monkeypatch):
    """4 600 atoms in 4 x 5 cells of a capped grid: the owned build overflows, check() turns the handle to the two-launch build, and
    that and three more evaluations equal a handle that never ran anything else."""
    pos, box = _crowded()
    monkeypatch.setenv("NNPOPS_CELL_BIN_CAP", "512")
    species = _species(len(pos), "crowded")
    tbox = torch.tensor(box, device=DEV)
    one = _make(monkeypatch, species, True, {"NNPOPS_ANI_GRID_OWNED": "1"})
    two = _make(monkeypatch, species, True, {"NNPOPS_ANI_GRID_OWNED": "0"})
    one.set_neighbor_algorithm(2); two.set_neighbor_algorithm(2)
    tpos = torch.tensor(pos, device=DEV)
    one.compute(tpos, tbox, check=False)
    assert one.overflow_word() & 4 and one.read_grid()["bin_overflow"] == 1
    w = _weights(one)
    got = _step(one, tpos, tbox, w)                               # check() inside: binned from here on
    assert one.describe()["grid_build"] == "binned"
    _equal(got, _step(two, tpos, tbox, w))
    rng = np.random.default_rng(13)
    for _ in range(3):
        frame = _moved(pos, rng)
        _equal(_step(one, frame, tbox, w), _step(two, frame, tbox, w))
        assert one.read_grid() == two.read_grid() and one.read_grid()["ok"] == 1 and one.describe()["grid_build"] == "binned"


@pytest.mark.parametrize("captured", [True, False], ids=["graph_owned_eager_binned", "graph_binned_eager_owned"])
def test_graph_replayed_behind_the_other_build(monkeypatch, captured):
    """A step captured under one build, then an eager call of the other build, then the graph twice on two frames."""
    species, pos, box = _frame("box-2003")
    tbox = torch.tensor(np.array(box), device=DEV)
    one = _make(monkeypatch, species, True, {"NNPOPS_ANI_GRID_OWNED": "1"})
    only = {True: _make(monkeypatch, species, True, {"NNPOPS_ANI_GRID_OWNED": "1"}),
            False: _make(monkeypatch, species, True, {"NNPOPS_ANI_GRID_OWNED": "0"})}
    w = _weights(one)
    static = torch.tensor(np.array(pos), device=DEV)
    radial = torch.empty((one.num_atoms, one.radial_width), device=DEV)
    angular = torch.empty((one.num_atoms, one.angular_width), device=DEV)
    grad = torch.empty((one.num_atoms, 3), device=DEV)
    one.set_grid_build(captured)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                        # fits the capacities
            one.compute(static, tbox, radial, angular, check=True)
            one.backprop(*w, grad)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one.compute(static, tbox, radial, angular, check=False)
        one.backprop(*w, grad)
    rng = np.random.default_rng(17)
    one.set_grid_build(not captured)                              # the eager call of the other build
    frame = _moved(pos, rng)
    _equal(_step(one, frame, tbox, w, check=False), _step(only[not captured], frame, tbox, w))
    assert one.describe()["grid_build"] == ("binned" if captured else "owned")
    for _ in range(2):
        static.copy_(_moved(pos, rng))
        graph.replay()
        torch.cuda.synchronize()
        assert one.overflow_word() == 0
        _equal((radial, angular, grad), _step(only[captured], static, tbox, w))
    frame = _moved(pos, rng)                                      # ... and eagerly again behind the replays
    _equal(_step(one, frame, tbox, w, check=False), _step(only[not captured], frame, tbox, w))
    assert one.read_grid()["ok"] == 1 and one.read_grid()["bin_overflow"] == 0


# ---------------------------------------------------------------------------------------------- 4. the other instantiations
# (frames and AniOracle64 references of test_ani_dispatch_gpu.py: liquid2100 -- 32 record slots, cell grid -- and dense900 -- 64
#  slots, all pairs, two waves per atom, leg forces in the receivers' rows)
INSTANTIATIONS = [
    ("liquid2100", {"NNPOPS_ANI_FWD_WPA": "1", "NNPOPS_ANI_FUSE": "0"}, dict(bwd_mode="1", radial_bwd="lanes", cap_angular="32")),      # forward, one wave per atom
    ("liquid2100", {"NNPOPS_ANI_FUSE": "0"}, dict(bwd_mode="1", radial_bwd="lanes", fused_build="0")),                                 # forward, two waves; LAT, 32-wide id rows
    ("liquid2100", {"NNPOPS_ANI_BACKWARD": "3"}, dict(bwd_mode="3", radial_bwd="lanes")),                                             # backward, two waves per atom
    ("liquid2100", {"NNPOPS_ANI_STREAMS": "2", "NNPOPS_ANI_FUSE": "0"}, dict(bwd_mode="1", radial_bwd="lanes")),                       # span launches, w0 > 0
    ("liquid2100", {"NNPOPS_ANI_STREAMS": "4", "NNPOPS_ANI_FUSE": "0"}, dict(bwd_mode="1", radial_bwd="lanes")),
    ("liquid2100", {"NNPOPS_ANI_BWD_APG": "4", "NNPOPS_ANI_FWD_APG": "2"}, dict(bwd_mode="1")),                                       # several atoms per workgroup, strided loop
    ("dense900", {}, dict(bwd_mode="3", scatter="1", cap_angular="64", radial_bwd="lanes")),                                         # RECV, 64-wide rows
    ("dense900", {"NNPOPS_ANI_SCATTER": "0"}, dict(bwd_mode="3", scatter="0", cap_angular="64", radial_bwd="lanes")),                 # LAT gather, 64-wide id rows
    ("dense900", {"NNPOPS_ANI_BACKWARD": "1", "NNPOPS_ANI_BWD_CLASSES": "0"}, dict(bwd_mode="1", cap_angular="64")),                  # one wave per atom at 64 slots
]


@pytest.mark.parametrize("system,env,expect", INSTANTIATIONS, ids=[f"{s}-{'-'.join(f'{k[11:]}={v}' for k, v in e.items()) or 'default'}" for s, e, _ in INSTANTIATIONS])
def test_instantiations(monkeypatch, system, env, expect):
    import os
    for k in [k for k in os.environ if k.startswith("NNPOPS_ANI_")]:
        monkeypatch.delenv(k)
    n_species, rcr, rca, species, pos, box = _dispatch_system(system)
    rf, af = workloads.ani2x_functions()
    ref = _reference((system, "ani2x"), n_species, rcr, rca, species, rf, af, pos, box, True)
    from nnpops_amd.capi import AniSymmetryFunctions
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sym = AniSymmetryFunctions(n_species, rcr, rca, species, rf, af, periodic=True, torchani=True)
    r, a, g = _evaluate(sym, pos, box, ref)
    what = sym.describe()
    for k, v in expect.items():
        assert what[k] == v, (k, what)
    _judge(f"prologue 4 {system} {env}", ref, r, a, g)


def test_class_launches_and_their_clean_up(monkeypatch):
    """The dense liquid launched by class (three class launches and the clean-up launch behind them), then a second frame WITHOUT a
    check in between: atoms that outgrew their class are the clean-up launch's, whose 256 workgroups stride over all atoms."""
    system = "dense900"
    n_species, rcr, rca, species, pos, box = _dispatch_system(system)
    rf, af = workloads.ani2x_functions()
    from nnpops_amd.capi import AniSymmetryFunctions
    from oracle import AniOracle64
    for k, v in {"NNPOPS_ANI_BWD_CLASSES": "1", "NNPOPS_ANI_BWD_CLASS_MIN": "0", "NNPOPS_ANI_BWD_CLASS_ATOMS": "0"}.items():
        monkeypatch.setenv(k, v)
    sym = AniSymmetryFunctions(n_species, rcr, rca, species, rf, af, periodic=True, torchani=True)
    ref = _reference((system, "ani2x"), n_species, rcr, rca, species, rf, af, pos, box, True)
    r, a, g = _evaluate(sym, pos, box, ref)
    assert int(sym.describe()["classes"]) >= 2, sym.describe()
    _judge("prologue 4 classes", ref, r, a, g)
    moved = (np.array(pos) + np.random.default_rng(19).normal(0, 0.25, pos.shape)).astype(np.float32)
    oracle = AniOracle64(n_species, rcr, rca, species, rf, af, periodic=True, torchani=True)
    r2, a2 = oracle.forward(moved, box)
    ref2 = dict(r=r2, a=a2, g=oracle.backward(ref["wr"], ref["wa"]), wr=ref["wr"], wa=ref["wa"])
    r, a, g = _evaluate(sym, moved, box, ref2, check=False)
    assert sym.overflow_word() == 8, sym.overflow_word()          # an atom outgrew its class and nothing else overflowed
    _judge("prologue 4 clean-up", ref2, r, a, g)
