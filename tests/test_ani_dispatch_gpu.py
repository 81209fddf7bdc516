"""Every angular and radial kernel the ANI handle's dispatcher can reach, against the algorithm in float64.

nnpops_ani picks its kernels from the function list (uniform or per-factor eta / zeta, padded factor shapes), the record
capacity (32 / 64 / 128 / 256 slots), the alignment of the caller's arrays and the NNPOPS_ANI_* switches.  test_ani_gpu.py
follows the ANI-2x default path closely; this file walks the rest of the matrix:

    a  factor grids with several eta and several zeta (the per-factor forward and backward instantiations), every padded shape
    b  128 record slots: the pair matrix beyond 64 KB of LDS, the row kernel as the radial backward
    c  256 record slots: the first-generation angular backward as the production fall-back, atoms below and above its tile
    d  mode 4: two waves per atom with the gradient row in LDS (a dense system whose rows are not 16-byte aligned)
    e  the documented A/B switches, each against float64, the schedule-only ones bit for bit against the default run

The judge is oracle.AniOracle64 (oracle/ani_oracle.c in double precision on the same float32 inputs): on the dense systems of
b and c the float32 oracle's own forces sit 2e-5 .. 5e-5 of the largest component away from it, half of the 1e-4 gate.  Every
reference is evaluated once per (system, function set, torchani) and kept for the module; the weights of the energy
functional E = <w, aev> are seeded.  Bars (BASELINE.json north_star, the fuzz file's form for the AEV):

    AEV      |a - ref| <= 2e-5 |ref| + 2e-6 max(1, max|ref|)   element-wise, radial and angular part each
    energy   E = <w, aev> to 1e-5 of sum |w aev|;  E = sum aev to 1e-5 relative
    forces   max |g - g_ref| <= 1e-4 max |g_ref|
    all outputs finite; two consecutive backprop() calls bit-identical (no path here has atomics)

Every test asserts through nnpops_ani_describe that the path it names is the one that ran (bwd_mode, radial_bwd, cap_angular,
uniform, literal, generic, forward, fused_build, scatter, classes), in addition to the numbers.  Each judged evaluation prints
one line with its measured errors (pytest -s shows them).
"""
import zlib

import numpy as np
import pytest
import torch

from ani_float64 import system as _system      # (tests here take a parameter named system)
from nnpops_amd import workloads
from oracle import AniOracle64

pytestmark = pytest.mark.gpu

ENERGY_RTOL = 1e-5
FORCE_RTOL = 1e-4      # of the largest force component of the system
AEV_ATOL, AEV_RTOL = 2e-6, 2e-5

_REFERENCES = {}       # key -> dict(r, a, g, wr, wa): one float64 evaluation per (system, function set, torchani)
_DEFAULT_RUNS = {}     # section e: system tag -> (r, a, g) of the handle without any switch


# ---------------------------------------------------------------------------------------------- inputs
# The frames are ani_float64.system's: liquid600 and conformer60 (section a), slots128 (b), slots256 and slots256_loose (c), dense900
# (d, e) and liquid2100 (e).
def _neighbour_counts(pos, box, cutoff):
    """Neighbours of every atom inside `cutoff` (float64, minimum image in a cubic box)."""
    d = pos.astype(np.float64)[:, None, :] - pos.astype(np.float64)[None, :, :]
    if box is not None:
        L = float(box[0, 0])
        d -= L * np.round(d / L)
    return (np.einsum("ijk,ijk->ij", d, d) < float(np.float32(cutoff)) ** 2).sum(axis=1) - 1


def _grid_functions(n_eta, n_shf, n_zeta, n_ths, rca, eta=(12.5, 6.0, 9.0), zeta=(14.1, 4.0, 8.0)):
    """-> (radial factors [(eta, Rs)], angular factors [(zeta, theta_s)]) of a full grid with n_eta distinct eta and n_zeta
    distinct zeta, in the order the torch binding's loops meet them (for eta: for Rs / for zeta: for theta_s)."""
    shf_a = np.linspace(0.8, rca - 0.5, n_shf) if n_shf > 1 else np.array([1.5])
    shf_z = (np.arange(n_ths) + 0.5) * np.pi / n_ths
    fr = [(e, float(rs)) for e in eta[:n_eta] for rs in shf_a]
    fz = [(z, float(t)) for z in zeta[:n_zeta] for t in shf_z]
    return fr, fz


# (nFR, nFZ) -> (number of eta, shifts per eta, number of zeta, angles per zeta): at least two distinct eta and two distinct zeta
NONUNIFORM_SHAPES = {
    (4, 4): (2, 2, 2, 2),
    (3, 3): (3, 1, 3, 1),          # padded to 4 x 4: two slots stay empty on each side
    (4, 6): (2, 2, 2, 3),          # 4 x 8
    (8, 4): (2, 4, 2, 2),          # ANI-2x's shape, not its values
    (6, 8): (2, 3, 2, 4),          # 8 x 8
    (12, 4): (2, 6, 2, 2),         # 16 x 4
    (16, 8): (2, 8, 2, 4),         # 16 x 8, 128 functions
}


def _angular_list(fr, fz, order):
    """The function list [nA, 4] = {(eta, Rs)} x {(zeta, theta_s)} and, for every row, its column in the factor-major list
    (the layout the references are kept in).
        factor_major  for (eta, Rs): for (zeta, theta_s) -- function m sits at canonical slot m when no factor slot is padded
        binding       the torch binding's loop nest: for eta: for zeta: for Rs: for theta_s
        shuffled      a seeded permutation"""
    nz = len(fz)
    idx = [(a, z) for a in range(len(fr)) for z in range(nz)]
    if order == "binding":
        etas, zetas = list(dict.fromkeys(e for e, _ in fr)), list(dict.fromkeys(z for z, _ in fz))
        idx = [(a, z) for e in etas for zt in zetas for a in range(len(fr)) if fr[a][0] == e for z in range(nz) if fz[z][0] == zt]
    elif order == "shuffled":
        perm = np.random.default_rng(1234 + 100 * len(fr) + nz).permutation(len(idx))
        idx = [idx[k] for k in perm]
    else:
        assert order == "factor_major"
    af = np.array([[fr[a][0], fr[a][1], fz[z][0], fz[z][1]] for a, z in idx], dtype=np.float32)
    return af, np.array([a * nz + z for a, z in idx])


def _function_set(name, rca):
    """-> (radial functions, angular functions) of a named set of sections b and c, in factor-major order."""
    rf, af = workloads.ani2x_functions()
    if name == "ani2x":
        return rf, af
    if name == "uniform8x4":                   # one eta, one zeta, eight equally spaced shifts: not the published constants
        fr, fz = _grid_functions(1, 8, 1, 4, rca, eta=(9.5,), zeta=(8.0,))
    elif name == "nonuniform8x4":
        fr, fz = _grid_functions(*NONUNIFORM_SHAPES[(8, 4)], rca)
    elif name == "nonuniform4x4":
        fr, fz = _grid_functions(*NONUNIFORM_SHAPES[(4, 4)], rca)
    else:
        raise KeyError(name)
    return rf, _angular_list(fr, fz, "factor_major")[0]


# ---------------------------------------------------------------------------------------------- reference and judge
def _reference(key, n_species, rcr, rca, species, rf, af, pos, box, torchani):
    """The float64 evaluation of `key`, once per module, with seeded weights."""
    if key not in _REFERENCES:
        oracle = AniOracle64(n_species, rcr, rca, species, rf, af, periodic=box is not None, torchani=torchani)
        r, a = oracle.forward(pos, box)
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        wr = rng.standard_normal(r.shape).astype(np.float32)
        wa = rng.standard_normal(a.shape).astype(np.float32)
        _REFERENCES[key] = dict(r=r, a=a, g=oracle.backward(wr, wa), wr=wr, wa=wa)
    return _REFERENCES[key]


def _permuted(ref, n_species, column_of_row):
    """The same reference for a function list whose row m is the factor-major list's row column_of_row[m]."""
    nb = n_species * (n_species + 1) // 2
    n = ref["a"].shape[0]
    take = lambda x: np.ascontiguousarray(x.reshape(n, nb, -1)[:, :, column_of_row].reshape(n, -1))
    return dict(r=ref["r"], wr=ref["wr"], g=ref["g"], a=take(ref["a"]), wa=take(ref["wa"]))


def _evaluate(sym, pos, box, ref, check=True, pad=None):
    """compute() + two backprop() calls with the reference's weights -> radial, angular, forces (numpy).  pad: through
    nnpops_ani_compute_strided / _backprop_strided on ONE [N, W_r + W_a + pad] array."""
    from nnpops_amd.capi import lib, _ptr, _check
    dev = torch.device("cuda:0")
    tpos = torch.tensor(pos, device=dev)
    tbox = torch.tensor(box, device=dev) if box is not None else None
    t_wr, t_wa = torch.tensor(ref["wr"], device=dev), torch.tensor(ref["wa"], device=dev)
    if pad is None:
        radial, angular = sym.compute(tpos, tbox, check=check)
        g1 = sym.backprop(t_wr, t_wa).clone()
        g2 = sym.backprop(t_wr, t_wa)
    else:
        radial, angular = sym.compute(tpos, tbox, check=check)        # (dense call first: capacities are grown and fitted by its checks)
        wr, wa = radial.shape[1], angular.shape[1]
        ld = wr + wa + pad
        aev = torch.full((len(pos), ld), float("nan"), device=dev)
        L = lib()
        _check(L.nnpops_ani_compute_strided(sym._h, _ptr(tpos), _ptr(tbox), aev.data_ptr(), ld, aev.data_ptr() + 4 * wr, ld))
        torch.cuda.synchronize()
        assert bool(torch.isnan(aev[:, wr + wa:]).all())                # nothing written behind the rows
        radial, angular = aev[:, :wr], aev[:, wr:wr + wa]
        grads = torch.zeros((len(pos), ld), device=dev)
        grads[:, :wr], grads[:, wr:wr + wa] = t_wr, t_wa
        out = []
        for _ in range(2):
            g = torch.empty((len(pos), 3), device=dev)
            _check(L.nnpops_ani_backprop_strided(sym._h, grads.data_ptr(), ld, grads.data_ptr() + 4 * wr, ld, _ptr(g)))
            out.append(g)
        g1, g2 = out
    torch.cuda.synchronize()
    assert torch.equal(g1, g2), "two consecutive backprop() calls differ"
    return radial.cpu().numpy().copy(), angular.cpu().numpy().copy(), g1.cpu().numpy().copy()


def _judge(tag, ref, r, a, g):
    """The bars of the module docstring; prints the measured figures first."""
    r64, a64, g64 = r.astype(np.float64), a.astype(np.float64), g.astype(np.float64)
    finite = bool(np.isfinite(r).all() and np.isfinite(a).all() and np.isfinite(g).all())
    aev_excess = 0.0                 # largest |error| / allowance over both parts (<= 1 passes)
    aev_err = 0.0                    # largest |error| / largest element of its part
    for x, x_ref in ((r64, ref["r"]), (a64, ref["a"])):
        top = float(np.abs(x_ref).max()) if x_ref.size else 0.0
        allow = AEV_RTOL * np.abs(x_ref) + AEV_ATOL * max(1.0, top)
        aev_excess = max(aev_excess, float((np.abs(x - x_ref) / allow).max()))
        aev_err = max(aev_err, float(np.abs(x - x_ref).max()) / max(top, 1e-300))
    e_ref = float((ref["r"] * ref["wr"]).sum() + (ref["a"] * ref["wa"]).sum())
    e = float((r64 * ref["wr"]).sum() + (a64 * ref["wa"]).sum())
    scale = float(np.abs(ref["r"] * ref["wr"]).sum() + np.abs(ref["a"] * ref["wa"]).sum())
    s_ref, s = float(ref["r"].sum() + ref["a"].sum()), float(r64.sum() + a64.sum())
    fmax = float(np.abs(ref["g"]).max())
    f_err = float(np.abs(g64 - ref["g"]).max())
    print(f"\n[ani-dispatch] {tag}: aev {aev_err:.2e} of max (x{aev_excess:.2f} of the bar)  E_w {abs(e - e_ref) / max(scale, 1e-300):.2e}  "
          f"E_sum {abs(s - s_ref) / max(abs(s_ref), 1e-300):.2e}  force {f_err / max(fmax, 1e-300):.2e}  finite {finite}")
    assert finite, tag
    assert aev_excess <= 1.0, (tag, aev_excess, aev_err)
    assert abs(e - e_ref) <= ENERGY_RTOL * scale, (tag, e, e_ref, scale)
    assert abs(s - s_ref) <= ENERGY_RTOL * abs(s_ref), (tag, s, s_ref)
    assert f_err <= FORCE_RTOL * fmax, (tag, f_err, fmax)


def _handle(tag, rf, af, torchani):
    from nnpops_amd.capi import AniSymmetryFunctions
    n_species, rcr, rca, species, pos, box = _system(tag)
    return AniSymmetryFunctions(n_species, rcr, rca, species, rf, af, periodic=box is not None, torchani=torchani)


def test_describe_before_and_after_backprop():
    """The launch records of nnpops_ani_describe: nothing launched yet reads -1 / none, also after a compute(); after a backprop()
    the pair kernels report their mode and no tile; the existing keys are all there and the line fits the 512 bytes capi reads."""
    n_species, rcr, rca, species, pos, box = _system("liquid600")
    rf, af = workloads.ani2x_functions()
    sym = _handle("liquid600", rf, af, True)
    dev = torch.device("cuda:0")
    for step in range(2):
        what = sym.describe()
        assert (what["bwd_mode"], what["radial_bwd"], what["tile"], what["compact"]) == ("-1", "none", "-1", "-1"), what
        radial, angular = sym.compute(torch.tensor(pos, device=dev), torch.tensor(box, device=dev))
    sym.backprop(torch.ones_like(radial), torch.ones_like(angular))
    what = sym.describe()
    assert (what["bwd_mode"], what["radial_bwd"], what["tile"], what["compact"]) == ("1", "lanes", "-1", "-1"), what
    assert list(what) == ["forward", "backward", "generic", "uniform", "grid", "literal", "dynamic_quads", "fused_build", "cap", "cap_angular",
                          "chunk", "classes", "cells", "scatter", "row_major_walk", "bwd_mode", "radial_bwd", "tile", "compact"], what
    assert len(" ".join(f"{k}={v}" for k, v in what.items())) < 400


# ---------------------------------------------------------------------------------------------- a. non-uniform factor grids
def _nonuniform_case(system, shape, order, torchani):
    """-> handle, reference (in the list's order), positions, box"""
    n_species, rcr, rca, species, pos, box = _system(system)
    rf, _ = workloads.ani2x_functions()
    fr, fz = _grid_functions(*NONUNIFORM_SHAPES[shape], rca)
    assert len(fr) == shape[0] and len(fz) == shape[1]
    assert len({e for e, _ in fr}) >= 2 and len({z for z, _ in fz}) >= 2
    af_major, _ = _angular_list(fr, fz, "factor_major")
    ref = _reference(("a", system, shape, torchani), n_species, rcr, rca, species, rf, af_major, pos, box, torchani)
    af, column = _angular_list(fr, fz, order)
    return _handle(system, rf, af, torchani), _permuted(ref, n_species, column), pos, box


def _pad(n):
    p = 4
    while p < n:
        p *= 2
    return p


@pytest.mark.parametrize("torchani", [True, False])
@pytest.mark.parametrize("system", ["liquid600", "conformer60"])
@pytest.mark.parametrize("order", ["factor_major", "binding", "shuffled"])
@pytest.mark.parametrize("shape", list(NONUNIFORM_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_nonuniform_factor_grids(shape, order, system, torchani):
    """Function sets with several eta and several zeta take the per-factor instantiations (ani_angular_forward_mfma<..., 7>,
    ani_angular_backward_pair<..., {1, 2}, false> and their LDS-row variants): every padded shape, in the order that puts
    function m at canonical slot m (16-byte loads of the gradient blocks: mode 1 or 3), in the torch binding's loop order and
    shuffled (c_of_m is not the identity: gradient row staged in LDS, mode 2 or 4).  A kernel that read factor 0's eta or
    zeta for every factor fails here."""
    sym, ref, pos, box = _nonuniform_case(system, shape, order, torchani)
    r, a, g = _evaluate(sym, pos, box, ref)
    what = sym.describe()
    assert what["uniform"] == "0" and what["generic"] == "0" and what["literal"] == "0", what
    busiest = int(_neighbour_counts(pos, box, 3.5).max())                  # (24 in the liquid, 44 in the molecule: records of 32 and 64 slots)
    assert what["forward"] == "mfma" and what["radial_bwd"] == "lanes" and what["cap_angular"] == ("32" if busiest <= 32 else "64"), what
    identity = order == "factor_major" and shape == (_pad(shape[0]), _pad(shape[1]))
    assert what["bwd_mode"] in (("1", "3") if identity else ("2", "4")), (identity, what)
    assert what["fused_build"] == ("1" if identity and shape == (8, 4) else "0"), what
    _judge(f"a {shape} {order} {system} torchani={torchani} mode={what['bwd_mode']}", ref, r, a, g)


@pytest.mark.parametrize("torchani", [True, False])
@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("forward", ["0", "1", "2"])
@pytest.mark.parametrize("shape", [(8, 4), (4, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nonuniform_grids_on_every_forward_kernel(monkeypatch, shape, forward, fuse, torchani):
    """The same sets through the run-merging (0) and chunked (1) forward kernels with per-factor constants and through the
    matrix-core one (2), stand-alone and -- the 8 x 4 shape, which alone has a fused kernel -- fused with the neighbour build
    (ani_build_forward<TA, 8, 4, 7>)."""
    monkeypatch.setenv("NNPOPS_ANI_FORWARD", forward)
    monkeypatch.setenv("NNPOPS_ANI_FUSE", fuse)
    sym, ref, pos, box = _nonuniform_case("liquid600", shape, "factor_major", torchani)
    r, a, g = _evaluate(sym, pos, box, ref)
    what = sym.describe()
    assert what["forward"] == {"0": "merge", "1": "chunked", "2": "mfma"}[forward], what
    assert what["fused_build"] == ("1" if (fuse, forward, shape) == ("1", "2", (8, 4)) else "0"), what
    assert what["uniform"] == "0" and what["generic"] == "0", what
    assert what["bwd_mode"] in (("1", "3") if shape == (8, 4) else ("2", "4")) and what["radial_bwd"] == "lanes", what
    _judge(f"a-forward {shape} FORWARD={forward} FUSE={fuse} torchani={torchani}", ref, r, a, g)


# ---------------------------------------------------------------------------------------------- b. 128 record slots
@pytest.mark.parametrize("classes", [False, True], ids=["one_launch", "by_class"])
@pytest.mark.parametrize("fset", ["uniform8x4", "nonuniform8x4", "ani2x"])
def test_128_record_slots(monkeypatch, fset, classes):
    """76-105 angular neighbours per atom (Rca 4.8 on a liquid of density 0.2): records of 128 slots.  The pair matrix is
    ~100 KB of LDS (hipFuncSetAttribute, one workgroup per CU), the lane-per-neighbour radial backward is off and the
    first-generation row kernel produces the radial forces.  With the classes on, the forces must equal the one-launch
    ones bit for bit (the same per-atom arithmetic, whatever launch it ran in)."""
    n_species, rcr, rca, species, pos, box = _system("slots128")
    counts = _neighbour_counts(pos, box, rca)
    assert 64 < counts.max() <= 256 and box[0, 0] >= 2.05 * rcr, (counts.min(), counts.max(), box[0, 0])       # the scenario
    rf, af = _function_set(fset, rca)
    ref = _reference(("b", fset), n_species, rcr, rca, species, rf, af, pos, box, True)
    if classes:
        monkeypatch.setenv("NNPOPS_ANI_BWD_CLASSES", "1")
        monkeypatch.setenv("NNPOPS_ANI_BWD_CLASS_MIN", "0")
        monkeypatch.setenv("NNPOPS_ANI_BWD_CLASS_ATOMS", "0")           # (by default only systems of 16 384+ atoms launch by class)
    sym = _handle("slots128", rf, af, True)
    r, a, g = _evaluate(sym, pos, box, ref)
    what = sym.describe()
    assert what["cap_angular"] == "128" and what["radial_bwd"] == "rows" and what["bwd_mode"] in ("1", "3"), what
    assert what["generic"] == "0" and what["forward"] == "mfma" and what["scatter"] == "0", what
    assert what["uniform"] == ("0" if fset == "nonuniform8x4" else "1"), what
    # the ANI-2x list with another cutoff: every derived constant still equals the compiled-in one, so the literal kernels run
    assert what["literal"] == ("1" if fset == "ani2x" else "0"), what
    assert (int(what["classes"]) >= 1) == classes, what
    _judge(f"b {fset} classes={classes} mode={what['bwd_mode']}", ref, r, a, g)
    if not classes:
        _DEFAULT_RUNS[("b", fset)] = (r, a, g)
    else:
        if ("b", fset) not in _DEFAULT_RUNS:
            _DEFAULT_RUNS[("b", fset)] = _evaluate(_with_env(monkeypatch, {"NNPOPS_ANI_BWD_CLASSES": None, "NNPOPS_ANI_BWD_CLASS_MIN": None,
                                                                           "NNPOPS_ANI_BWD_CLASS_ATOMS": None},
                                                             lambda: _handle("slots128", rf, af, True)), pos, box, ref)
        r0, a0, g0 = _DEFAULT_RUNS[("b", fset)]
        assert np.array_equal(r, r0) and np.array_equal(a, a0) and np.array_equal(g, g0)


def _with_env(monkeypatch, env, make):
    """make() under the given switches (None: unset) -- the handle reads them in nnpops_ani_create -- then the caller's again."""
    import os
    before = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
    try:
        return make()
    finally:
        for k, v in before.items():
            monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------- c. 256 record slots
@pytest.mark.parametrize("torchani", [True, False])
@pytest.mark.parametrize("fset", ["uniform8x4", "nonuniform4x4"])
def test_256_record_slots_take_the_first_generation_backward(fset, torchani):
    """36-223 angular neighbours in one frame (a dense cluster in vacuum, Rca 5.0): records of 256 slots, the pair kernels'
    matrix no longer fits 160 KiB of LDS and the first-generation ani_angular_backward runs WITHOUT any switch, atoms below
    and above its tile side by side (one tile from the builder's list / tile pairs); the 8-bit p and q fields of the triple
    words run to their limit in the forward.  Then a looser frame and the dense one again, unchecked: capacities do not shrink
    and the results stay the float64 ones."""
    n_species, rcr, rca, species, pos, box = _system("slots256")
    assert box is None
    counts = _neighbour_counts(pos, None, rca)
    assert 163 < counts.max() <= 256 and counts.min() < 64, (counts.min(), counts.max())                        # the scenario
    rf, af = _function_set(fset, rca)
    ref = _reference(("c", fset, torchani), n_species, rcr, rca, species, rf, af, pos, None, torchani)
    sym = _handle("slots256", rf, af, torchani)
    r, a, g = _evaluate(sym, pos, None, ref)
    what = sym.describe()
    assert what["cap_angular"] == "256" and what["bwd_mode"] == "0" and what["backward"] == "1", what          # (configured 1, launched 0)
    assert what["radial_bwd"] == "rows" and what["generic"] == "0" and what["forward"] == "mfma", what
    assert what["uniform"] == ("1" if fset == "uniform8x4" else "0") and what["scatter"] == "0", what
    assert 8 <= int(what["tile"]) <= 32 and what["compact"] == "0", what        # busier atoms than the tile: never the compact layout
    assert int(what["tile"]) < counts.max()
    _judge(f"c {fset} torchani={torchani} tile={what['tile']} compact={what['compact']}", ref, r, a, g)
    if torchani:
        _, _, _, _, loose, _ = _system("slots256_loose")
        ref_loose = _reference(("c-loose", fset, torchani), n_species, rcr, rca, species, rf, af, loose, None, torchani)
        r2, a2, g2 = _evaluate(sym, loose, None, ref_loose, check=False)
        assert sym.describe()["cap_angular"] == "256" and sym.describe()["bwd_mode"] == "0", sym.describe()
        _judge(f"c {fset} torchani={torchani} loose frame, unchecked", ref_loose, r2, a2, g2)
        r3, a3, g3 = _evaluate(sym, pos, None, ref, check=False)
        assert sym.describe()["cap_angular"] == "256" and sym.describe()["bwd_mode"] == "0", sym.describe()
        _judge(f"c {fset} torchani={torchani} dense frame again, unchecked", ref, r3, a3, g3)


# ---------------------------------------------------------------------------------------------- d. mode 4
def test_mode_4_on_a_dense_system_with_unaligned_rows():
    """A dense system (64 record slots: 27 KB of pair matrix, two waves per atom) whose gradient rows are not 16-byte aligned
    (one [N, W_r + W_a + 5] array through the strided entry points): mode 3 + 1 = 4, two waves per atom with the gradient row
    staged in LDS; the radial rows are unaligned too, so the row kernel is the radial backward.  Judged against float64, not
    against the dense call."""
    n_species, rcr, rca, species, pos, box = _system("dense900")
    rf, af = workloads.ani2x_functions()
    ref = _reference(("dense900", "ani2x"), n_species, rcr, rca, species, rf, af, pos, box, True)
    sym = _handle("dense900", rf, af, True)
    r, a, g = _evaluate(sym, pos, box, ref, pad=5)
    what = sym.describe()
    assert what["bwd_mode"] == "4" and what["radial_bwd"] == "rows" and what["cap_angular"] == "64", what
    assert what["forward"] == "mfma" and what["fused_build"] == "0" and what["scatter"] == "0" and what["generic"] == "0", what
    assert what["uniform"] == "1" and what["literal"] == "1", what
    _judge("d dense900 pad=5 mode=4", ref, r, a, g)


# ---------------------------------------------------------------------------------------------- e. the forced variants
SWITCHES = [("BACKWARD", v) for v in "0234"] + [("RBWD", "0"), ("BWD_LITERAL", "0"), ("OCC", "6"), ("LPT", "0"), ("LPT", "1"),
            ("STREAMS", "2"), ("STREAMS", "4"), ("STORE", "0"), ("STORE", "1"), ("STORE", "2"), ("FWD_WPA", "1"), ("FWD_ROWLDS", "0"),
            ("FWD_OCC", "6"), ("FWD_OCC", "8"), ("FWD_CHUNK", "64"), ("FWD_CHUNK", "512"), ("FWD_APG", "2"), ("FWD_APG", "4"),
            ("BWD_APG", "2"), ("BWD_APG", "4")]
SCHEDULE_ONLY = ("LPT", "STREAMS", "FWD_APG", "BWD_APG", "STORE")      # same arithmetic per atom: the default run's bits
BACKWARD_ONLY = ("BACKWARD", "RBWD", "BWD_LITERAL", "OCC", "BWD_APG")  # the forward is the default run's: its AEV bit for bit


def _default_run(system, ref):
    """AEV and forces of the handle without any switch, once per system; -> (r, a, g), describe()"""
    if system not in _DEFAULT_RUNS:
        n_species, rcr, rca, species, pos, box = _system(system)
        sym = _handle(system, *workloads.ani2x_functions(), True)
        out = _evaluate(sym, pos, box, ref)
        _DEFAULT_RUNS[system] = (out, sym.describe())
        _judge(f"e {system} default", ref, *out)
    return _DEFAULT_RUNS[system]


@pytest.mark.parametrize("switch,value", SWITCHES, ids=[f"{s}={v}" for s, v in SWITCHES])
@pytest.mark.parametrize("system", ["liquid2100", "dense900"])
def test_forced_variants(monkeypatch, system, switch, value):
    """The documented A/B switches (README: environment switches), on a 2 100-atom liquid (32 record slots, cell grid, large
    enough for NNPOPS_ANI_STREAMS to split) and on the 64-slot dense liquid (two waves per atom, leg forces scattered): each
    variant against float64; what describe() can tell is asserted to be in effect; the switches that only change the schedule
    must reproduce the default run's AEV and forces bit for bit."""
    import os
    for k in [k for k in os.environ if k.startswith("NNPOPS_ANI_")]:
        monkeypatch.delenv(k)
    n_species, rcr, rca, species, pos, box = _system(system)
    rf, af = workloads.ani2x_functions()
    ref = _reference((system, "ani2x"), n_species, rcr, rca, species, rf, af, pos, box, True)
    (r0, a0, g0), base = _default_run(system, ref)
    dense = system == "dense900"
    assert base["cap_angular"] == ("64" if dense else "32") and base["radial_bwd"] == "lanes" and base["literal"] == "1", base
    assert base["bwd_mode"] == ("3" if dense else "1") and base["scatter"] == ("1" if dense else "0"), base
    assert base["fused_build"] == "1" and base["cells"] == ("0" if dense else "1"), base
    if switch == "STREAMS" and dense:
        # Not schedule-only here: leg forces are scattered only by handles configured for ONE stream (a condition of
        # nnpops_ani_backprop_strided), also where the system is too small to be split, so this switch turns the scattering off.
        # Like with like: the default handle with the gathering backward ($NNPOPS_ANI_SCATTER=0), bit for bit.
        if (system, "gather") not in _DEFAULT_RUNS:
            gather = _with_env(monkeypatch, {"NNPOPS_ANI_SCATTER": "0"}, lambda: _handle(system, rf, af, True))
            _DEFAULT_RUNS[(system, "gather")] = _evaluate(gather, pos, box, ref)
            assert gather.describe()["scatter"] == "0" and gather.describe()["bwd_mode"] == "3", gather.describe()
        r0, a0, g0 = _DEFAULT_RUNS[(system, "gather")]
    monkeypatch.setenv("NNPOPS_ANI_" + switch, value)
    sym = _handle(system, rf, af, True)
    r, a, g = _evaluate(sym, pos, box, ref)
    what = sym.describe()
    assert what["scatter"] == ("1" if dense and switch not in ("STREAMS", "BACKWARD", "RBWD", "BWD_LITERAL", "OCC") else "0"), what
    assert what["generic"] == "0" and what["forward"] == "mfma" and what["cap_angular"] == base["cap_angular"], what
    if switch == "BACKWARD":
        assert what["backward"] == value and what["bwd_mode"] == value, what         # forced: the mode asked for, no automatic 1 -> 3
    else:
        assert what["backward"] == "1", what
    assert what["radial_bwd"] == ("rows" if switch == "RBWD" else "lanes"), what
    # (BWD_LITERAL: leg forces are scattered by the literal kernels only -- scatter=0 above is what describe() shows of this switch)
    if switch == "FWD_CHUNK":
        assert what["chunk"] == value, what
    assert what["literal"] == "1", what          # (the forward's literals are NNPOPS_ANI_FWD_LITERAL's, not this list's)
    _judge(f"e {system} {switch}={value} mode={what['bwd_mode']} radial={what['radial_bwd']} scatter={what['scatter']} "
           f"fused={what['fused_build']} chunk={what['chunk']}", ref, r, a, g)
    same_aev = bool(np.array_equal(r, r0) and np.array_equal(a, a0))
    same_forces = bool(np.array_equal(g, g0))
    print(f"[ani-dispatch] e {system} {switch}={value}: AEV bits equal default {same_aev}, force bits equal default {same_forces}")
    if switch in SCHEDULE_ONLY:
        assert same_aev and same_forces, (switch, value, what, base)
    elif switch in BACKWARD_ONLY:
        assert same_aev, (switch, value, what, base)
