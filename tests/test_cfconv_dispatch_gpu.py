"""Every kernel the CFConv dispatcher can reach, forward and backward, against float64 at the edges of the dispatch.

nnpops_cfconv_create picks one of four kernel families -- about twenty template instantiations -- from the width, the number of Gaussians,
the weights and three LDS-fit formulas.  test_cfconv_gpu.py and the fuzz file follow the common shapes against the float32 oracle; this
file stands on the edges: the K steps of the register-fed kernels' first layer (G = 31, 32, 63, 2), the last shape of the register path
(G = 63 at W = 32, 64, 96; G = 55 at W = 128), the plane kernel thinning out to one wave, the one shape (W 128, G 172) that reaches the
fp32 matrix kernel with a single wave, odd numbers of column blocks, the vector kernel with one to eight channels per lane and with its
weights in LDS in one direction and streamed in the other, the forced paths, pair counts around the filters kernels' tiles, rows around the
vector kernel's tile and around the row capacities, and more pairs than one sweep of the grid.  The table, the frames and the expected
plan of every row are in tests/cfconv_dispatch_float64.py; tests/test_cfconv_dispatch_reference_cpu.py proves, before anything runs
here, that no launch of the table asks for more LDS than there is, and that the float32 oracle sits inside half of every bar below.

Every (row, activation) goes through one helper.  It asserts that describe() -- what the handle's launches use -- is the table's row and is
nnpops_cfconv_plan of the same arguments; on the small frames that export() is the judge's half list with distances to rtol 1e-6; that the
first check() reports the row overflow where the frame's rows outgrow 64 entries, and only there.  Then, in this order: backprop() on the
fresh handle (the backward kernel stores its own filter rows), compute(), backprop() again (it reads the forward call's rows back),
compute() again.  Each of the first three results is judged against cfconv_float64.Restatement (one float64 evaluation per frame, shape
and activation, kept for the module):

    output, input gradient   |a - ref| <= 2e-5 |ref| + 2e-6 max|ref|   element-wise
    position gradient        max |g - g_ref| <= 1e-4 max |g_ref|
    energy                   L = <gout, out> within 1e-5 of sum |gout out|
    all outputs finite; the two backprop() results within the same bars of each other; the two compute() results equal bit for bit;
    without any pair (chain:0, one atom) output, input gradient and position gradient exactly zero

(cfconv_float64's OUT_RTOL, OUT_ATOL_FRAC, FORCE_RTOL; no bar is widened for any row.)  box1000c10 gets no list assertion: with 63 000
pairs per angstrom at its cutoff some pair lies within float32 rounding of it, and the builder and the judge may disagree about that
pair -- which carries fc ~ delta^2 ~ 1e-13 of a filter row, far under any bar.

Each judged evaluation prints one line with its figures as fractions of the bars (pytest -s).  Measured on an MI355X, worst over the
table per path (docs/LAB_NOTEBOOK_cfconv_dispatch.md has them next to the float32 oracle's on the same case):

    path (worst case)                              output   input gradient   force     float32 oracle on the same case
    split registers (sweep_w128_g50 ssp)           0.494    0.541            5.30e-6   0.462 / 0.642 / 9.56e-6
    split planes (sweep_w128_g56 ssp)              0.614    0.569            4.39e-6   0.546 / 0.587 / 7.12e-6
    split planes (chain33_w32_g70 tanh)            0.141    0.577            2.40e-6   0.103 / 0.142 / 9.95e-7
    fp32 matrix (w80_g256 ssp)                     0.301    0.263            1.81e-6   0.299 / 0.198 / 2.27e-6
    fp32 matrix (w112_g236_last_matrix ssp)        0.200    0.334            1.21e-6   0.179 / 0.253 / 2.23e-6
    vector (w512_g256_maxima ssp)                  0.356    0.325            1.72e-6   0.281 / 0.284 / 4.15e-6

(output and input gradient as fractions of their bar, forces as a fraction of the largest component against the bar of 1e-4; the
energy never above 0.017 of its bar).  All 184 cases pass in 4 s.
"""
import numpy as np
import pytest
import torch

import cfconv_dispatch_float64 as dispatch
from box_gradient_judge import clean_env
from cfconv_float64 import FORCE_RTOL, OUT_ATOL_FRAC, OUT_RTOL, Restatement, sigma_of
from nnpops_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_REFERENCES = {}       # (frame, W, G, act) -> Restatement.evaluate: one float64 evaluation per module


def _reference(row, act):
    key = (row.frame, row.W, row.G, act)
    if key not in _REFERENCES:
        pos, box, cutoff = dispatch.frame(row.frame)
        w1, b1, w2, b2, x, gout = dispatch.layer(row.frame, row.W, row.G)
        if len(pos) == 1:                                   # one atom: nothing to evaluate
            zero = np.zeros((1, row.W))
            ref = dict(out=zero, gx=zero, g=np.zeros((1, 3)), L=0.0, i=np.zeros(0, int), j=np.zeros(0, int), d=np.zeros((0, 3)))
        else:
            ref = Restatement(row.W, row.G, cutoff, sigma_of(row.G), act, w1, b1, w2, b2).evaluate(
                pos, dispatch.FAR_BOX if box is None else box, x, gout)
        _REFERENCES[key] = ref
    return _REFERENCES[key]


def _close(a, b, what):
    """a within the bars of b (two results of the same handle)"""
    if what == "gp":
        return float(np.abs(a - b).max()) <= FORCE_RTOL * float(np.abs(b).max())
    return bool(np.all(np.abs(a - b) <= OUT_RTOL * np.abs(b) + OUT_ATOL_FRAC * np.abs(b).max()))


def _run(monkeypatch, row, act):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)
    pos, box, cutoff = dispatch.frame(row.frame)
    n, periodic = len(pos), box is not None
    w1, b1, w2, b2, x, gout = dispatch.layer(row.frame, row.W, row.G)
    ref = _reference(row, act)

    # ---- the path: the handle's launches are the table's row and the plan of the same arguments ----
    plan = dispatch.plan_of(row, act)
    nb = capi.CFConvNeighbors(n, cutoff, periodic)
    cf = capi.CFConv(n, row.W, row.G, cutoff, sigma_of(row.G), act, w1, b1, w2, b2, periodic=periodic)
    described = cf.describe()
    assert described == plan
    assert {k: described[k] for k in dispatch.expected_plan(row)} == dispatch.expected_plan(row), described

    # ---- the list: capacity growth reported by the first check() where the rows outgrow 64 entries, then the judge's pairs ----
    tpos = torch.tensor(pos, device=DEV)
    tbox = torch.tensor(box, device=DEV) if periodic else None
    tx, tg = torch.tensor(x, device=DEV), torch.tensor(gout, device=DEV)
    nb.build(tpos, tbox, check=False)
    if row.grows:
        with pytest.raises(capi.NNPOpsHipError) as overflow:
            nb.num_pairs()
        assert overflow.value.code == capi.ERR_CAPACITY
        nb.build(tpos, tbox)
    assert nb.num_pairs() == len(ref["i"]) or row.frame == "box1000c10"
    if row.frame != "box1000c10":
        atoms, dist = nb.export()
        assert np.array_equal(atoms[0], ref["i"]) and np.array_equal(atoms[1], ref["j"])
        np.testing.assert_allclose(dist, np.sqrt(np.einsum("ij,ij->i", ref["d"], ref["d"])), rtol=1e-6)

    # ---- backward on the fresh handle, forward, backward on the forward call's rows, forward again ----
    gx0, gp0 = cf.backprop(nb, tpos, tx, tg, tbox)
    out = cf.compute(nb, tpos, tx, tbox)
    gx1, gp1 = cf.backprop(nb, tpos, tx, tg, tbox)
    again = cf.compute(nb, tpos, tx, tbox)
    torch.cuda.synchronize()
    gx0, gp0, out, gx1, gp1, again = (t.cpu().numpy() for t in (gx0, gp0, out, gx1, gp1, again))

    figs = [dispatch.measure(ref, gout, gx=gx0, gp=gp0), dispatch.measure(ref, gout, out=out), dispatch.measure(ref, gout, gx=gx1, gp=gp1)]
    print(f"\n[cfconv-dispatch] {row.name} {act} {described['path']} waves {described['waves_fwd']}/{described['waves_bwd']} "
          f"pairs {len(ref['i'])}: fresh backward {dispatch.figures(figs[0])} | forward {dispatch.figures(figs[1])} | "
          f"backward {dispatch.figures(figs[2])}")
    for a in (gx0, gp0, out, gx1, gp1):
        assert np.isfinite(a).all()
    assert np.array_equal(out.view(np.int32), again.view(np.int32))
    if len(ref["i"]) == 0:
        for a in (gx0, gp0, out, gx1, gp1):
            assert not a.any()
        return
    for fig in figs:
        assert dispatch.within(fig), (row.name, act, fig)
    assert _close(gx0, gx1, "gx") and _close(gp0, gp1, "gp")


@pytest.mark.parametrize("case", dispatch.CASES, ids=dispatch.case_id)
def test_dispatch_edge(monkeypatch, case):
    _run(monkeypatch, *case)
