"""PME over a batch of frames on the GPU (pme_frames.hip) against the per-frame float64 judge (tests/pme_frames_float64.py) at the
project's end-to-end bars, the exact properties by bits, and the public surface.

Bars (test_pme_gpu.py, test_pme_reciprocal_passes_gpu.py): a frame's direct energy within 1e-5 of the frame's sum of |terms|, its
reciprocal energy within 1e-5 relative, dE/dx and dE/dq within 1e-4 of the frame's largest component."""
import functools
import math
import os
import sys

import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
from NNPOps.pme import PME
from nnpops_amd.pme.pme import bspline_moduli

sys.path.insert(0, os.path.dirname(__file__))
import pme_float64 as f64  # noqa: E402
import pme_frames_float64 as judge  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA, COULOMB, CUTOFF = judge.ALPHA, judge.COULOMB, judge.CUTOFF


def direct_op(case, weights=None):
    """torch.ops.pme.pme_direct_frames on a batch -> energies, d(sum w E)/dx, d(sum w E)/dq on the host"""
    pos, q, boxes, offsets, excl = case
    x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV, requires_grad=True)
    table = torch.ops.pme.pmeFramesTable(torch.tensor(offsets), torch.device(DEV))
    ex = torch.tensor(f64.sorted_excl(excl), dtype=torch.int32, device=DEV)
    e = torch.ops.pme.pme_direct_frames(x, c, ex, torch.tensor(boxes, device=DEV), table, CUTOFF, ALPHA, COULOMB)
    w = torch.ones_like(e) if weights is None else torch.tensor(weights, dtype=e.dtype, device=DEV)
    e.backward(w)
    return e.detach().cpu(), x.grad.cpu(), c.grad.cpu()


def recip_op(case, grid, order, weights=None):
    pos, q, boxes, offsets, _ = case
    x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV, requires_grad=True)
    table = torch.ops.pme.pmeFramesTable(torch.tensor(offsets), torch.device(DEV))
    e = torch.ops.pme.pme_reciprocal_frames(x, c, torch.tensor(boxes, device=DEV), table, *grid, order, ALPHA, COULOMB,
                                            *[bspline_moduli(k, order).to(DEV) for k in grid])
    w = torch.ones_like(e) if weights is None else torch.tensor(weights, dtype=e.dtype, device=DEV)
    e.backward(w)
    return e.detach().cpu(), x.grad.cpu(), c.grad.cpu()


def worst_rows(got, ref, offsets):
    """per frame max|got - ref| / max|ref| over the frame's rows (0 / 0 counts as 0: exact zeros expected where the judge has zeros)"""
    worst = 0.0
    for a, b in zip(offsets, offsets[1:]):
        if b > a:
            err, scale = float((got[a:b].double() - ref[a:b]).abs().max()), float(ref[a:b].abs().max())
            worst = max(worst, err / scale if scale > 0 else (0.0 if err == 0 else math.inf))
    return worst


@functools.lru_cache(maxsize=None)
def direct_case(name):
    case = judge.batch(**judge.DIRECT_CASES[name])
    return case, judge.direct_judge(*case[:4], f64.sorted_excl(case[4]))


@pytest.mark.parametrize("name", list(judge.DIRECT_CASES))
def test_direct_against_float64(name):
    case, (e_ref, terms, gx_ref, gq_ref) = direct_case(name)
    e, gx, gq = direct_op(case)
    e_err = [abs(float(a) - float(b)) / float(t) if t > 0 else (0.0 if float(a) == float(b) else math.inf) for a, b, t in zip(e, e_ref, terms)]
    figures = max(e_err), worst_rows(gx, gx_ref, case[3]), worst_rows(gq, gq_ref, case[3])
    print(f"direct {name}: energy {figures[0]:.2e} of sum|terms|  dE/dx {figures[1]:.2e}  dE/dq {figures[2]:.2e}")
    assert figures[0] <= 1e-5 and figures[1] <= 1e-4 and figures[2] <= 1e-4, figures


@pytest.mark.parametrize("name", list(judge.RECIP_CASES))
def test_reciprocal_against_float64(name):
    grid, order, sizes, seed, scales = judge.RECIP_CASES[name]
    case = judge.batch(sizes, seed, scales, excl="none")
    e_ref, gx_ref, gq_ref = judge.recip_judge(*case[:4], grid, order, [bspline_moduli(k, order) for k in grid])
    e, gx, gq = recip_op(case, grid, order)
    e_err = [abs(float(a) - float(b)) / abs(float(b)) if b != 0 else (0.0 if float(a) == 0 else math.inf) for a, b in zip(e, e_ref)]
    figures = max(e_err), worst_rows(gx, gx_ref, case[3]), worst_rows(gq, gq_ref, case[3])
    print(f"reciprocal {name}: energy {figures[0]:.2e}  dE/dx {figures[1]:.2e}  dE/dq {figures[2]:.2e}")
    assert figures[0] <= 1e-5 and figures[1] <= 1e-4 and figures[2] <= 1e-4, figures


@pytest.mark.parametrize("term", ["direct", "reciprocal"])
def test_a_frame_has_the_same_bits_alone_in_company_and_reversed(term):
    case = judge.batch((17, 0, 5, 33, 300), seed=81, scales=(1.0, 2.0))
    op = direct_op if term == "direct" else functools.partial(recip_op, grid=(8, 8, 16), order=5)
    e, gx, gq = op(case)
    again = op(case)
    assert all(torch.equal(a, b) for a, b in zip((e, gx, gq), again))
    offsets, B = case[3], len(case[3]) - 1
    er, gxr, gqr = op(judge.reorder(case, range(B - 1, -1, -1)))
    at = 0
    for m in range(B - 1, -1, -1):
        a, b = offsets[m], offsets[m + 1]
        alone = op(judge.reorder(case, [m]))
        for got in ((er[B - 1 - m : B - m], gxr[at : at + b - a], gqr[at : at + b - a]), alone):
            assert torch.equal(got[0], e[m : m + 1]) and torch.equal(got[1], gx[a:b]) and torch.equal(got[2], gq[a:b]), (term, m)
        at += b - a


def test_newtons_third_law_by_bits():
    case = judge.batch((2, 40, 17), seed=91, scales=(1.0, 1.0, 2.0), excl="none")
    pos, q, boxes, offsets, excl = case
    _, gx, _ = direct_op(case)
    assert torch.equal(gx[0], -gx[1]) and float(gx[0].abs().max()) > 0          # the two-atom frame: exact negatives
    # Both owners of a pair add the same float terms with opposite signs, so a frame's rows sum to the roundings of their float32
    # accumulations alone: each of a row's at most n additions errs by at most 2^-24 of the row's sum of |terms|, and over the frame
    # those sums are twice the pairs' |f| = |dE/dr|, formed here in float64 from the judge's pair set.
    for m, (a, b) in enumerate(zip(offsets, offsets[1:])):
        x, c = torch.tensor(pos[a:b], dtype=torch.float64), torch.tensor(q[a:b], dtype=torch.float64)
        i, j, shift, _, _ = judge.frame_pairs(x, torch.tensor(boxes[m], dtype=torch.float64), excl[a:b], a, CUTOFF)
        r = torch.linalg.norm(x[i] - x[j] - shift, dim=1)
        f = COULOMB * (c[i] * c[j]).abs() * (torch.erfc(ALPHA * r) + 2 * ALPHA * r * torch.exp(-(ALPHA * r) ** 2) / math.sqrt(math.pi)) / r ** 2
        residual = float(gx[a:b].double().sum(0).abs().max())
        assert residual <= (b - a) * 2.0 ** -24 * 2 * float(f.sum()), (m, residual)


def test_a_zero_upstream_gradient_gives_exact_zeros():
    case = judge.batch((17, 9, 33), seed=95)
    a, b = case[3][1], case[3][2]
    for op in (direct_op, functools.partial(recip_op, grid=(5, 7, 18), order=4)):
        _, gx, gq = op(case, weights=[1.0, 0.0, 2.5])
        _, hx, hq = op(case, weights=[1.0, 1.0, 2.5])
        assert not gx[a:b].any() and not gq[a:b].any() and hx[a:b].any()
        for rows in (slice(0, a), slice(b, None)):
            assert torch.equal(gx[rows], hx[rows]) and torch.equal(gq[rows], hq[rows])


def test_public_surface_against_the_ewald_sum_and_weighted_backward():
    case = judge.batch((24, 9, 30), seed=101, scales=(1.0, 2.0, 1.0))
    pos, q, boxes, offsets, excl = case
    alpha, grid, order = 4.0, (64, 64, 64), 5                               # (test_pme_reciprocal_gpu.py: erfc(alpha cutoff) ~ 1e-8)
    pme = PME(*grid, order, alpha, COULOMB, torch.tensor(excl), reciprocal=True)
    x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV, requires_grad=True)
    tb = torch.tensor(boxes, device=DEV)
    total = pme.compute_direct_frames(x, c, CUTOFF, tb, offsets) + pme.compute_reciprocal_frames(x, c, tb, offsets)
    assert total.shape == (3,)
    weights = [0.5, -2.0, 1.25]
    total.backward(torch.tensor(weights, device=DEV))
    # the full Ewald sum knows no exclusions: compare a table-free object's energies with it, the excluded one with the judge below
    free = PME(*grid, order, alpha, COULOMB, torch.zeros(len(q), 0, dtype=torch.int32), reciprocal=True)
    with torch.no_grad():
        e_free = (free.compute_direct_frames(x, c, CUTOFF, tb, offsets) + free.compute_reciprocal_frames(x, c, tb, offsets)).cpu()
    for m, (a, b) in enumerate(zip(offsets, offsets[1:])):
        full = float(f64.ewald_energy(torch.tensor(pos[a:b], dtype=torch.float64), torch.tensor(q[a:b], dtype=torch.float64),
                                      torch.tensor(boxes[m], dtype=torch.float64), alpha, COULOMB))
        assert abs(float(e_free[m]) - full) <= 2e-4 * max(abs(full), 1.0), (m, float(e_free[m]), full)
    moduli = [bspline_moduli(k, order) for k in grid]
    ed, _, dx, dq = judge.direct_judge(pos, q, boxes, offsets, f64.sorted_excl(excl), alpha=alpha, weights=weights)
    er, rx, rq = judge.recip_judge(pos, q, boxes, offsets, grid, order, moduli, alpha=alpha, weights=weights)
    self_q = torch.cat([torch.full((b - a,), w) for w, a, b in zip(weights, offsets, offsets[1:])]).double() * \
        (-2 * COULOMB * alpha / math.sqrt(math.pi)) * torch.tensor(q, dtype=torch.float64)
    assert worst_rows(x.grad.cpu(), dx + rx, offsets) <= 1e-4 and worst_rows(c.grad.cpu(), dq + rq + self_q, offsets) <= 1e-4


def test_graph_capture_follows_positions_and_boxes_written_in_place():
    first, second = judge.batch((17, 0, 33), seed=111), judge.batch((17, 0, 33), seed=112, scales=(2.0, 1.0))
    pme = PME(8, 8, 16, 5, ALPHA, COULOMB, torch.tensor(first[4]), reciprocal=True)
    x, c, tb = (torch.tensor(t, device=DEV) for t in first[:3])
    x.requires_grad_()
    offsets = first[3]

    def step():
        e = pme.compute_direct_frames(x, c, CUTOFF, tb, offsets) + pme.compute_reciprocal_frames(x, c, tb, offsets)
        (g,) = torch.autograd.grad(e.sum(), x)
        return e, g
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                               # warm-up: tables, moduli, FFT plans
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e_graph, g_graph = step()
    with torch.no_grad():
        x.copy_(torch.tensor(second[0], device=DEV)); tb.copy_(torch.tensor(second[2], device=DEV))
    e_eager, g_eager = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(e_graph, e_eager) and torch.equal(g_graph, g_eager)


def test_device_refusals():
    pos, q, boxes, offsets, excl = judge.batch((9, 12), seed=121)
    x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV)
    pme = PME(8, 8, 8, 5, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True)
    with pytest.raises(RuntimeError, match="box gradients"):
        pme.compute_direct_frames(x, c, CUTOFF, torch.tensor(boxes, device=DEV, requires_grad=True), offsets)
    with pytest.raises(RuntimeError, match="box gradients"):
        pme.compute_reciprocal_frames(x, c, torch.tensor(boxes, device=DEV, requires_grad=True), offsets)
    tb = torch.tensor(boxes, device=DEV)
    for e in (pme.compute_direct_frames(x, c, CUTOFF, tb, offsets), pme.compute_reciprocal_frames(x, c, tb, offsets)):
        with pytest.raises(RuntimeError, match="second derivatives"):
            torch.autograd.grad(e.sum(), x, create_graph=True)
    table = torch.ops.pme.pmeFramesTable(torch.tensor(offsets), torch.device(DEV))
    with pytest.raises(RuntimeError, match="pmeOrder 4 or 5"):
        torch.ops.pme.pme_reciprocal_frames(x, c, tb, table, 8, 8, 8, 6, ALPHA, COULOMB, *[bspline_moduli(8, 6).to(DEV)] * 3)
