"""The plan of every row of the CFConv dispatch table, the frames the GPU tests run on and the room the bars leave (CPU only).

tests/cfconv_dispatch_float64.py holds the table and the frames; tests/test_cfconv_dispatch_gpu.py runs them.  Here, without a GPU:
    * nnpops_cfconv_plan (host arithmetic) gives every row the path, the waves per workgroup and -- on the vector path -- the channels
      per lane and the places of the weights that the table states; no launch asks for less than one wave or for more dynamic LDS than
      a workgroup can have (163 840 bytes; the vector kernel budgets 156 KiB); two calls agree;
    * a scan over G = 2 .. 256 at the widths 32, 64, 96, 128 finds the path switches exactly where the table has its rows, so the table
      cannot drift from the selection rule unnoticed; the same for the first G at width 112 whose matrix-core weights no longer fit;
    * the frames are what their names say, in float64: chain:P has exactly P pairs, every row of blob:n has n - 1 entries, every
      listed pair of a small frame keeps cutoff - r >= 1e-3 and r >= 0.7, and box1000c10 has more than 65 536 pairs (one sweep of the
      forward register kernel's grid).  No unlisted pair of a small frame lies closer than 1e-4 beyond the cutoff either -- 300 times
      the float32 rounding of a distance of 5 -- so the float32 builder cannot list another set of pairs than the judge;
    * the float32 oracle (oracle.CFConvOracle: plain float32 arithmetic, pair by pair) on a sample of the rows sits inside HALF of
      every bar against the judge.  The frames and bars therefore leave float32 arithmetic room, and a kernel that misses a bar on the
      GPU has itself to blame.  Measured here (fractions of the bar: output / input gradient; forces as a fraction of the largest
      component): between 0.02 and 0.34 on output and input gradient, forces at most 4.6e-6 against the bar of 1e-4; on box1000c10
      (not asserted here: 22 s of oracle time a case) 0.46 to 0.64 and 9.6e-6.
"""
import numpy as np
import pytest

import cfconv_dispatch_float64 as dispatch
from box_gradient_judge import clean_env
from cfconv_float64 import Restatement, sigma_of
from nnpops_amd import capi
from oracle import CFConvNeighborsOracle, CFConvOracle


def _set_env(monkeypatch, row):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    for k, v in row.env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", dispatch.CASES, ids=dispatch.case_id)
def test_plan_of_every_row(monkeypatch, case):
    row, act = case
    _set_env(monkeypatch, row)
    plan = dispatch.plan_of(row, act)
    assert {k: plan[k] for k in dispatch.expected_plan(row)} == dispatch.expected_plan(row), plan
    limit = dispatch.VECTOR_LDS_LIMIT if plan["path"] == "vector" else dispatch.LDS_LIMIT
    for d in ("fwd", "bwd"):
        assert plan["waves_" + d] >= 1 and 0 < plan["lds_" + d] <= limit, plan
    assert 0 <= plan["dy_scale_log2"] <= 12
    assert dispatch.plan_of(row, act) == plan


@pytest.mark.parametrize("W", [32, 64, 96, 128])
def test_scan_over_gaussians_finds_the_switches_of_the_table(monkeypatch, W):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    w1, b1, w2, _, _, _ = dispatch.weights(W, 256, 1, 7)
    found, last = {}, None
    for G in range(2, 257):
        plan = capi.cfconv_plan(W, G, sigma_of(G), "ssp", w1[:, :G], b1, w2)
        limit = dispatch.VECTOR_LDS_LIMIT if plan["path"] == "vector" else dispatch.LDS_LIMIT
        assert min(plan["waves_fwd"], plan["waves_bwd"]) >= 1 and max(plan["lds_fwd"], plan["lds_bwd"]) <= limit, (G, plan)
        if last is not None and plan["path"] != last:
            found[G] = plan["path"]
        last = plan["path"]
    assert found == dispatch.path_switches(W)
    assert found == ({64: "split_planes"} if W < 128 else {56: "split_planes", 172: "matrix", 173: "vector"})


def test_width_112_leaves_the_matrix_cores_where_the_table_says(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    w1, b1, w2, _, _, _ = dispatch.weights(112, 256, 1, 7)
    paths = [capi.cfconv_plan(112, G, sigma_of(G), "tanh", w1[:, :G], b1, w2)["path"] for G in range(2, 257)]
    first_vector = 2 + paths.index("vector")
    assert set(paths[:first_vector - 2]) == {"matrix"} and set(paths[first_vector - 2:]) == {"vector"}
    assert first_vector == 237
    assert {r.G: r.path for r in dispatch.TABLE if r.W == 112} == {236: "matrix", 237: "vector"}


def test_plan_refuses_what_create_refuses():
    w1, b1, w2, _, _, _ = dispatch.weights(8, 4, 1, 7)
    for W, G, sigma, code in [(0, 4, 0.4, -1), (513, 4, 0.4, -1), (8, 257, 0.4, -1), (8, 1, 0.4, 0), (8, 4, 0.0, 0)]:
        with pytest.raises(capi.NNPOpsHipError) as err:
            capi.cfconv_plan(W, G, sigma, "ssp", w1, b1, w2)
        assert err.value.code < 0
    with pytest.raises(ValueError):
        capi.cfconv_plan(8, 4, 0.4, "relu", w1, b1, w2)


# ---------------------------------------------------------------------------------------------- frames
def _pairs64(tag):
    pos, box, cutoff = dispatch.frame(tag)
    p = pos.astype(np.float64)
    d = p[None, :, :] - p[:, None, :]
    if box is not None:
        L = float(box[0, 0])
        d -= L * np.round(d / L)
    r = np.sqrt(np.einsum("ijk,ijk->ij", d, d))
    i, j = np.triu_indices(len(p), 1)
    return r[i, j], cutoff, len(p), r


@pytest.mark.parametrize("tag", dispatch.SMALL_FRAMES)
def test_small_frames_are_what_their_names_say(tag):
    r, cutoff, n, full = _pairs64(tag)
    listed = r[r < cutoff]
    if len(listed):
        assert (cutoff - listed).min() >= 1e-3 and listed.min() >= 0.7
    assert not len(r) or (r[r >= cutoff] - cutoff).min(initial=1.0) >= 1e-4
    rows = (full < cutoff).sum(axis=1) - 1
    if tag.startswith("chain:"):
        assert len(listed) == int(tag[6:]) and n == max(int(tag[6:]), 1) + 1      # (P = 0: two atoms out of each other's reach)
    elif tag.startswith("blob:"):
        assert n == int(tag[5:]) and np.all(rows == n - 1)
    elif tag == "atom1":
        assert n == 1 and len(r) == 0
    else:
        assert tag == "conformer90" and len(listed) == 2493 and rows.min() == 15 and rows.max() == 80
    grows = {row.grows for row in dispatch.TABLE if row.frame == tag}
    assert grows == {bool(rows.max() > 64)}                  # the rows the table expects to outgrow the first capacity do


def test_periodic_frame_outgrows_one_sweep():
    r, cutoff, n, full = _pairs64("box1000c10")
    assert cutoff == 10.0 and (r < cutoff).sum() > 65536
    assert float(dispatch.frame("box1000c10")[1][0, 0]) >= 2 * cutoff      # one image per pair: the judge's single-round minimum image holds


# ---------------------------------------------------------------------------------------------- room under the bars
ORACLE_SAMPLE = [("conformer90", 512, 256, "ssp"), ("conformer90", 128, 172, "tanh"), ("conformer90", 128, 63, "ssp"),
                 ("conformer90", 257, 10, "tanh"), ("conformer90", 100, 256, "ssp"), ("conformer90", 32, 31, "tanh"),
                 ("chain:1", 32, 16, "ssp"), ("chain:33", 32, 16, "tanh"), ("blob:66", 128, 50, "ssp"), ("blob:130", 128, 50, "tanh")]


def oracle_figures(tag, W, G, act):
    """the float32 oracle against the judge on one case -> cfconv_dispatch_float64.measure's figures"""
    pos, box, cutoff = dispatch.frame(tag)
    n = len(pos)
    w1, b1, w2, b2, x, gout = dispatch.layer(tag, W, G)
    ref = Restatement(W, G, cutoff, sigma_of(G), act, w1, b1, w2, b2).evaluate(pos, dispatch.FAR_BOX if box is None else box, x, gout)
    onb = CFConvNeighborsOracle(n, cutoff, box is not None)
    onb.build(pos, box)
    ocf = CFConvOracle(n, W, G, cutoff, sigma_of(G), act, w1, b1, w2, b2, periodic=box is not None)
    out = ocf.forward(onb, pos, x, box)
    gx, gp = ocf.backward(onb, pos, x, gout, box)
    start, other, _ = onb.export()
    assert np.array_equal(np.repeat(np.arange(n), np.diff(start)), ref["i"]) and np.array_equal(other, ref["j"])
    return dispatch.measure(ref, gout, out=out, gx=gx, gp=gp)


@pytest.mark.parametrize("tag,W,G,act", ORACLE_SAMPLE, ids=[f"{c[0]}-w{c[1]}-g{c[2]}-{c[3]}" for c in ORACLE_SAMPLE])
def test_float32_oracle_sits_inside_half_of_every_bar(tag, W, G, act):
    fig = oracle_figures(tag, W, G, act)
    print(f"\n[cfconv-dispatch-reference] {tag} W {W} G {G} {act}: float32 oracle, fractions of the bars: {dispatch.figures(fig)}")
    assert dispatch.within(fig, 0.5), fig
