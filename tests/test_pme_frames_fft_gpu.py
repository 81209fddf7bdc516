"""The LDS-resident transform of PME over frames (pme_frames_fft.hip) on the GPU: the one-launch rfftn -> convolution ->
irfftn against numpy in float64, transform="lds" end to end against the float64 judges of the frames ops, bits, and refusals.
Bars.  The transform: 4 x the largest error the library route (two-step torch transforms around nnpops_pme_reciprocal_frames_convolve)
shows against the same judge on the same inputs, relative to each array's largest entry (two float32 operation orders of the same
sums).  End to end: those of test_pme_frames_gpu.py and test_pme_frames_box_gpu.py (energy 1e-5, gradients 1e-4 of the frame's largest)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
from NNPOps.pme import PME
from nnpops_amd import capi
from nnpops_amd.pme.pme import bspline_moduli

sys.path.insert(0, os.path.dirname(__file__))
import pme_float64 as f64  # noqa: E402
import pme_frames_float64 as judge  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA, COULOMB = judge.ALPHA, judge.COULOMB
# Measured on an MI355X against the float64 judge below on these inputs (docs/LAB_NOTEBOOK_pme_frames_fft.md has every grid), largest over
# the grids: the library route 5.2e-7 (potential), 7.0e-7 (scaled spectrum), 2.4e-7 (energies); this kernel 4.7e-7, 6.0e-7, 2.4e-7.
# The bar is 4 x the library route's largest, 4 x 7.0e-7, far below the cap of 1e-4 of the largest entry.
BAR_TRANSFORM = 2.8e-6
# (32, 32, 36): 156 920 bytes with its tables, the largest grid of this shape that fits the 163 840 bytes of LDS -- served, not refused
GRIDS = [(8, 8, 16), (6, 10, 12), (5, 7, 18), (16, 16, 16), (24, 24, 24), (32, 32, 32), (32, 32, 36)]


def transform_float64(real, boxes, grid, moduli, alpha):
    """numpy float64: rfftn -> the convolution's expressions -> irfftn without a factor -> potential, scaled spectrum, energies"""
    pot, scaled, energies = [], [], []
    k = [np.arange(n) for n in grid]
    mx, my, mz = np.meshgrid(*[np.where(i < (n + 1) // 2, i, i - n) for i, n in zip(k, grid)], indexing="ij")
    xm, ym, zm = np.meshgrid(*[np.asarray(m, np.float64) for m in moduli], indexing="ij")
    half = slice(0, grid[2] // 2 + 1)
    for r, b in zip(real.astype(np.float64), boxes.astype(np.float64)):
        inv = np.linalg.inv(b)                                      # m_hat = inv(B) m, lower triangular
        mh = [inv[a, 0] * mx + inv[a, 1] * my + inv[a, 2] * mz for a in range(3)]
        m2 = (mh[0] ** 2 + mh[1] ** 2 + mh[2] ** 2)[..., half]
        m2[0, 0, 0] = 1.0
        eterm = np.exp(-(math.pi / alpha) ** 2 * m2) / (m2 * math.pi * np.linalg.det(b) * (xm * ym * zm)[..., half])
        eterm[0, 0, 0] = 0.0
        g = np.fft.rfftn(r)
        kz = k[2][half]
        w = np.where((kz > 0) & (kz <= (grid[2] - 1) // 2), 2.0, 1.0)
        energies.append(0.5 * float((w * eterm * np.abs(g) ** 2).sum()))
        scaled.append(g * eterm)
        pot.append(np.fft.irfftn(scaled[-1], s=grid, axes=(0, 1, 2)) * np.prod(grid))
    return np.stack(pot), np.stack(scaled), np.array(energies)


def worst(got, ref):
    return float(np.abs(np.asarray(got, ref.dtype) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_transform_against_float64(grid):
    frames = 2 if grid[0] >= 24 else 3
    boxes = judge.batch((1,) * frames, seed=301, scales=(1.0, 2.0))[2]
    real = np.random.default_rng(sum(grid)).normal(size=(frames, *grid)).astype(np.float32)
    moduli = [bspline_moduli(n, 5) for n in grid]
    pot, scaled, energies = capi.pme_reciprocal_frames_transform(torch.tensor(real, device=DEV), torch.tensor(boxes, device=DEV), 5, ALPHA,
                                                                 *[m.to(DEV) for m in moduli], scaled=True)
    ref = transform_float64(real, boxes, grid, [m.numpy() for m in moduli], ALPHA)
    figures = worst(pot.cpu().numpy(), ref[0]), worst(scaled.cpu().numpy(), ref[1]), worst(energies.cpu().numpy(), ref[2])
    print(f"transform {grid}: potential {figures[0]:.2e}  scaled spectrum {figures[1]:.2e}  energies {figures[2]:.2e}")
    assert max(figures) <= BAR_TRANSFORM, figures


CASES = {name: judge.RECIP_CASES[name] for name in ("ragged_grid_5", "cube_16", "second_round_4")}
CASES["workload_24"] = ((24, 24, 24), 5, (60, 33, 100), 311, (1.0, 2.0))


def run(case, grid, order, box=False, weights=None):
    """compute_reciprocal_frames(transform="lds") -> energies, d(sum w E)/dx, /dq and, with `box`, /dB on the host"""
    pos, q, boxes, offsets, excl = case
    x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV, requires_grad=True)
    tb = torch.tensor(boxes, device=DEV, requires_grad=box)
    e = PME(*grid, order, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True).compute_reciprocal_frames(
        x, c, tb, offsets, box_gradient=box, transform="lds")
    e.backward(torch.ones_like(e) if weights is None else torch.tensor(weights, dtype=e.dtype, device=DEV))
    return e.detach().cpu(), x.grad.cpu(), c.grad.cpu(), tb.grad.cpu() if box else None


def rows(got, ref, offsets):
    """per frame max|got - ref| / max|ref| over the frame's rows (0 / 0 counts as 0: exact zeros expected where the judge has zeros)"""
    worst_of = 0.0
    for a, b in ((a, b) for a, b in zip(offsets, offsets[1:]) if b > a):
        err, scale = float((got[a:b].double() - ref[a:b]).abs().max()), float(ref[a:b].abs().max())
        worst_of = max(worst_of, err / scale if scale > 0 else (0.0 if err == 0 else math.inf))
    return worst_of


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end_against_float64(name):
    grid, order, sizes, seed, scales = CASES[name]
    case = judge.batch(sizes, seed, scales, excl="none")
    pos, q, boxes, offsets, _ = case
    moduli = [bspline_moduli(k, order) for k in grid]
    e_ref, gx_ref, gq_ref = judge.recip_judge(pos, q, boxes, offsets, grid, order, moduli)
    self_scale = -COULOMB * ALPHA / math.sqrt(math.pi)                   # the self energy the public method adds
    q64 = torch.tensor(q, dtype=torch.float64)
    e_ref = e_ref + self_scale * torch.stack([(q64[a:b] ** 2).sum() for a, b in zip(offsets, offsets[1:])])
    gq_ref = gq_ref + 2 * self_scale * q64
    e, gx, gq, gb = run(case, grid, order, box=True)
    gb_ref = torch.zeros(len(boxes), 3, 3, dtype=torch.float64)
    for m, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b > a:
            box = torch.tensor(boxes[m], dtype=torch.float64, requires_grad=True)
            gb_ref[m] = torch.autograd.grad(f64.spme_energy(torch.tensor(pos[a:b], dtype=torch.float64), q64[a:b], box, grid, order, ALPHA,
                                                            COULOMB, moduli), box)[0]
    e_err = max(abs(float(a) - float(b)) / abs(float(b)) if b != 0 else abs(float(a)) for a, b in zip(e, e_ref))
    figures = e_err, rows(gx, gx_ref, offsets), rows(gq, gq_ref, offsets), rows(gb.reshape(-1, 3), gb_ref.reshape(-1, 3), range(0, 3 * len(boxes) + 1, 3))
    print(f"lds {name}: energy {figures[0]:.2e}  dE/dx {figures[1]:.2e}  dE/dq {figures[2]:.2e}  dE/dB {figures[3]:.2e}")
    assert figures[0] <= 1e-5 and max(figures[1:]) <= 1e-4, figures
    plain = run(case, grid, order)                                        # without the box gradient: the same bits
    assert all(torch.equal(a, b) for a, b in zip((e, gx, gq), plain[:3]))


def test_a_frame_has_the_same_bits_alone_in_company_reversed_and_again():
    case, grid, order, B = judge.batch((17, 0, 5, 33, 300), seed=81, scales=(1.0, 2.0), excl="none"), (8, 8, 16), 5, 5
    first = run(case, grid, order, box=True)
    assert all(torch.equal(a, b) for a, b in zip(run(case, grid, order, box=True), first)) and bool(first[3][0].any())
    reverse = run(judge.reorder(case, range(B - 1, -1, -1)), grid, order, box=True)
    for m in range(B):
        alone = run(judge.reorder(case, [m]), grid, order, box=True)
        a, b = case[3][m], case[3][m + 1]
        ra = reverse[1].shape[0] - b
        for k, sl, rsl in ((0, slice(m, m + 1), slice(B - 1 - m, B - m)), (1, slice(a, b), slice(ra, ra + b - a)),
                           (2, slice(a, b), slice(ra, ra + b - a)), (3, slice(m, m + 1), slice(B - 1 - m, B - m))):
            assert torch.equal(alone[k], first[k][sl]) and torch.equal(reverse[k][rsl], first[k][sl]), (m, k)


def test_a_captured_graph_replays_to_the_eager_bits():
    pos, q, boxes, offsets, excl = judge.batch((17, 0, 33), seed=111, excl="none")
    pme = PME(24, 24, 24, 5, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True)
    x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV, requires_grad=True)
    tb = torch.tensor(boxes, device=DEV, requires_grad=True)

    def step():
        e = pme.compute_reciprocal_frames(x, c, tb, offsets, box_gradient=True, transform="lds")
        return (e,) + torch.autograd.grad(e.sum(), (x, c, tb))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                           # warm-up: tables, moduli, the kernel's LDS grant
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    eager = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager)) and bool(eager[3].any())


@pytest.mark.parametrize("grid, options, error, rule", [
    ((32, 32, 40), {}, ValueError, "LDS"), ((11, 8, 8), {}, ValueError, "prime factors"), ((8, 8, 9), {}, ValueError, "even"),
    ((8, 8, 16), {"twice_differentiable": True}, RuntimeError, "twice_differentiable"), ((8, 8, 16), {"transform": "fast"}, ValueError, '"torch" or "lds"')])
def test_what_is_not_served_is_refused_before_a_launch(grid, options, error, rule):
    pos, q, boxes, offsets, excl = judge.batch((5, 3), seed=121, excl="none")
    args = [torch.tensor(t, device=DEV) for t in (pos, q, boxes)]
    with pytest.raises(error, match=rule):
        PME(*grid, 4, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True).compute_reciprocal_frames(*args, offsets, **{"transform": "lds", **options})
    if not options:                                                      # the C ABI refuses the grid as well and touches nothing
        energies = torch.full((2,), 7.0, device=DEV)
        with pytest.raises(capi.NNPOpsHipError, match=rule):
            capi.pme_reciprocal_frames_transform(torch.zeros((2, *grid), device=DEV), args[2], 4, ALPHA,
                                                 *[bspline_moduli(k, 4).to(DEV) for k in grid], energies=energies)
        torch.cuda.synchronize()
        assert bool((energies == 7.0).all())
