"""Second derivatives of PME over frames on the GPU (pme_frames_second_order.hip) against float64, frame by frame:
pme_float64.second_order over the direct sum of the frame's own pairs with frozen shifts (direct_energy_frozen on
pme_frames_float64.frame_pairs) or over smooth PME with the frame's box (spme_energy), with cotangents v, w and distinct upstream
gradients g_m (frame 1 of a batch of three or more frames has g = 0).

Energies and first gradients: the bits of the default ops.  dL/dx, dL/dq, dL/dg: per frame, max error over the frame's largest reference
entry; a frame whose largest entry is below 1e-6 of the batch's is measured against the batch's.  BARS are ten times the worst figure
measured on an MI355X, one digit (DESIGN.md s8f holds the figures), none looser than the project's 1e-4."""
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
# dL/dx, dL/dq, dL/dg.  Measured worst: direct 1.4e-5 (seventy_small), 6.7e-6, 1.2e-5 (tile_edges); reciprocal 2.9e-6, 1.5e-6, 5.0e-6
BARS = {"direct": (1e-4, 7e-5, 1e-4), "reciprocal": (3e-5, 1e-5, 5e-5)}
# d loss/dx, d loss/dq of the losses through the class.  Measured worst: direct 1.0e-5, 9.5e-6; reciprocal 1.5e-6, 1.1e-6
CLASS_BARS = {"direct": (1e-4, 1e-4), "reciprocal": (2e-5, 1e-5)}


def upstream(case):
    B = len(case[2])
    return [0.0 if (m == 1 and B > 2) else 0.5 + 0.125 * m for m in range(B)]


def energies(term, case, x, c, grid, order, twice):
    pos, q, boxes, offsets, excl = case
    tb = torch.tensor(boxes, device=DEV)
    table = torch.ops.pme.pmeFramesTable(torch.tensor(offsets), torch.device(DEV))
    if term == "direct":
        op = torch.ops.pme.pme_direct_frames_twice if twice else torch.ops.pme.pme_direct_frames
        return op(x, c, torch.tensor(f64.sorted_excl(excl), dtype=torch.int32, device=DEV), tb, table, CUTOFF, ALPHA, COULOMB)
    op = torch.ops.pme.pme_reciprocal_frames_twice if twice else torch.ops.pme.pme_reciprocal_frames
    return op(x, c, tb, table, *grid, order, ALPHA, COULOMB, *[bspline_moduli(k, order).to(DEV) for k in grid])


def run(term, case, g, v, w, grid=None, order=None):
    """the _twice op of `term` on a batch -> energies, g P, g C, dL/dx, dL/dq, dL/dg on the host"""
    x, c = torch.tensor(case[0], device=DEV, requires_grad=True), torch.tensor(case[1], device=DEV, requires_grad=True)
    gt = torch.tensor(g, dtype=torch.float32, device=DEV, requires_grad=True)
    e = energies(term, case, x, c, grid, order, True)
    P, C = torch.autograd.grad((gt * e).sum(), (x, c), create_graph=True)
    assert P.requires_grad and C.requires_grad
    out = torch.autograd.grad((v.to(DEV) * P).sum() + (w.to(DEV) * C).sum(), (x, c, gt))
    return tuple(t.detach().cpu() for t in (e, P, C) + out)


def default_bits(term, case, g, grid=None, order=None):
    x, c = torch.tensor(case[0], device=DEV, requires_grad=True), torch.tensor(case[1], device=DEV, requires_grad=True)
    e = energies(term, case, x, c, grid, order, False)
    e.backward(torch.tensor(g, dtype=torch.float32, device=DEV))
    return e.detach().cpu(), x.grad.cpu(), c.grad.cpu()


def reference(energy_of_frame, case, g, v, w):
    """dL/dx [N, 3], dL/dq [N], dL/dg [B] in float64, frame by frame"""
    pos, q, _, offsets = case[:4]
    gx, gq, gg = torch.zeros(len(q), 3, dtype=torch.float64), torch.zeros(len(q), dtype=torch.float64), torch.zeros(len(g), dtype=torch.float64)
    for m, (a, b) in enumerate(zip(offsets, offsets[1:])):
        if b > a:
            x, c, _ = f64.leaves(pos[a:b], q[a:b], torch.float64)
            gm = torch.tensor(g[m], dtype=torch.float64, requires_grad=True)
            gx[a:b], gq[a:b], gg[m] = f64.second_order(lambda xx, cc: energy_of_frame(m, xx, cc), x, c, gm, v[a:b].double(), w[a:b].double())[3:]
    return gx, gq, gg


def direct_energy(case):
    pos, _, boxes, offsets, excl = case
    p64, b64, ex = torch.tensor(pos, dtype=torch.float64), torch.tensor(boxes, dtype=torch.float64), f64.sorted_excl(excl)
    pairs = [judge.frame_pairs(p64[a:b], b64[m], ex[a:b], a, CUTOFF) for m, (a, b) in enumerate(zip(offsets, offsets[1:]))]
    return lambda m, x, c: f64.direct_energy_frozen(x, c, pairs[m], ALPHA, COULOMB)


def recip_energy(case, grid, order):
    b64, moduli = torch.tensor(case[2], dtype=torch.float64), [bspline_moduli(k, order) for k in grid]
    return lambda m, x, c: f64.spme_energy(x, c, b64[m], grid, order, ALPHA, COULOMB, moduli)


def check(label, term, case, got, ref, plain):
    assert all(torch.equal(a, b) for a, b in zip(got[:3], plain)), label    # energies, g P, g C: the default op's bits
    offsets, figures = case[3], []
    for k, (out, want) in enumerate(zip(got[3:], ref)):
        rows = [(out[a:b], want[a:b]) if k < 2 else (out[m:m + 1], want[m:m + 1]) for m, (a, b) in enumerate(zip(offsets, offsets[1:]))]
        top, worst = float(want.abs().max()), 0.0
        for o, r in rows:
            if r.numel():
                scale = float(r.abs().max())
                worst = max(worst, float((o.double() - r).abs().max()) / (scale if scale >= 1e-6 * top else top))
        figures.append(worst)
    print(f"{label}: dL/dx {figures[0]:.2e}  dL/dq {figures[1]:.2e}  dL/dg {figures[2]:.2e}")
    assert all(f <= bar for f, bar in zip(figures, BARS[term])), (label, figures)


@pytest.mark.parametrize("name", list(judge.DIRECT_CASES))
def test_direct_against_float64(name):
    case = judge.batch(**judge.DIRECT_CASES[name])
    g, (v, w) = upstream(case), f64.cotangents(len(case[1]), 7, torch.float32)
    check(f"direct {name}", "direct", case, run("direct", case, g, v, w), reference(direct_energy(case), case, g, v, w),
          default_bits("direct", case, g))


@pytest.mark.parametrize("name", list(judge.RECIP_CASES))
def test_reciprocal_against_float64(name):
    grid, order, sizes, seed, scales = judge.RECIP_CASES[name]
    case = judge.batch(sizes, seed, scales, excl="none")
    g, (v, w) = upstream(case), f64.cotangents(len(case[1]), 8, torch.float32)
    check(f"reciprocal {name}", "reciprocal", case, run("reciprocal", case, g, v, w, grid, order),
          reference(recip_energy(case, grid, order), case, g, v, w), default_bits("reciprocal", case, g, grid, order))


SMALL = dict(sizes=(17, 0, 5, 33, 300), seed=81, scales=(1.0, 2.0))
GRID, ORDER = (8, 8, 16), 5


@pytest.mark.parametrize("term", ["direct", "reciprocal"])
def test_zero_upstream_gradient_gives_exact_zeros(term):
    case = judge.batch(**SMALL)
    v, w = f64.cotangents(len(case[1]), 9, torch.float32)
    out = run(term, case, [1.5, 2.0, 0.0, 0.0, 0.75], v, w, GRID, ORDER)
    a, b = case[3][2], case[3][4]
    assert not out[3][a:b].any() and not out[4][a:b].any() and bool(out[3][:a].any()) and float(out[5][3]) != 0


def test_equal_cotangents_inside_every_frame_give_exact_zeros_from_the_direct_term():
    case = judge.batch(**SMALL)
    offsets = case[3]
    v = torch.cat([torch.full((b - a, 3), 0.3 + m).mul(torch.tensor([1.0, -2.0, 0.5])) for m, (a, b) in enumerate(zip(offsets, offsets[1:]))])
    out = run("direct", case, upstream(case), v.float(), torch.zeros(len(case[1])))
    assert not out[3].any() and not out[4].any() and bool(out[1].any())


@pytest.mark.parametrize("term", ["direct", "reciprocal"])
def test_a_frame_has_the_same_bits_alone_in_company_reversed_and_in_a_second_call(term):
    case, B = judge.batch(**SMALL), 5
    g, (v, w) = upstream(case), f64.cotangents(len(case[1]), 10, torch.float32)
    offsets = case[3]

    def rows(order):                                                          # frame -> (dL/dx, dL/dq, dL/dg) of that frame
        idx = torch.cat([torch.arange(offsets[m], offsets[m + 1]) for m in order]).long()
        sub = judge.reorder(case, order)
        out = run(term, sub, [g[m] for m in order], v[idx], w[idx], GRID, ORDER)
        return {m: (out[3][a:b], out[4][a:b], out[5][k]) for k, (m, a, b) in enumerate(zip(order, sub[3], sub[3][1:]))}
    first, again, reverse = rows(range(B)), rows(range(B)), rows(range(B - 1, -1, -1))
    for m in range(B):
        alone = rows([m])
        for other in (again, reverse, alone):
            assert all(torch.equal(p, r) for p, r in zip(first[m], other[m])), (term, m)
    assert bool(first[4][0].any())


@pytest.mark.parametrize("term", ["direct", "reciprocal"])
def test_force_loss_through_the_class(term):
    pos, q, boxes, offsets, excl = case = judge.batch((17, 0, 33), seed=121, scales=(1.0, 2.0))
    pme = PME(*GRID, ORDER, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True)
    f_ref = f64.cotangents(len(q), 11, torch.float32)[0]
    tb = torch.tensor(boxes, device=DEV)

    def loss_gradients(x, c, total, charge_loss=False):
        F, C = torch.autograd.grad(total, (x, c), create_graph=True)
        loss = (C ** 2).sum() if charge_loss else ((-F - f_ref.to(x)) ** 2).sum()
        return [t.detach().double().cpu() for t in torch.autograd.grad(loss, (x, c))]
    if term == "direct":
        call = lambda x, c: pme.compute_direct_frames(x, c, CUTOFF, tb, offsets, twice_differentiable=True).sum()  # noqa: E731
        frame = direct_energy(case)
    else:
        call = lambda x, c: pme.compute_reciprocal_frames(x, c, tb, offsets, twice_differentiable=True).sum()  # noqa: E731
        spme, self_k = recip_energy(case, GRID, ORDER), COULOMB * ALPHA / torch.pi ** 0.5
        frame = lambda m, x, c: spme(m, x, c) - self_k * (c * c).sum()  # noqa: E731
    total64 = lambda x, c: sum(frame(m, x[a:b], c[a:b]) for m, (a, b) in enumerate(zip(offsets, offsets[1:])) if b > a)  # noqa: E731
    for charge_loss in (False, True):                                        # (the second: the self energy differentiates itself)
        x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV, requires_grad=True)
        x64, c64, _ = f64.leaves(pos, q, torch.float64)
        got, ref = loss_gradients(x, c, call(x, c), charge_loss), loss_gradients(x64, c64, total64(x64, c64), charge_loss)
        figures = [f64.rel(a, r) for a, r in zip(got, ref) if float(r.abs().max()) > 0]
        print(f"force loss through the class, {term}, charge loss {charge_loss}: d loss/dx, d loss/dq {figures}")
        assert all(f <= bar for f, bar in zip(figures, CLASS_BARS[term])), (term, figures)


def test_graph_capture_of_a_force_loss_step_follows_inputs_written_in_place():
    first, second = judge.batch((17, 0, 33), seed=111), judge.batch((17, 0, 33), seed=112, scales=(2.0, 1.0))
    pme = PME(*GRID, ORDER, ALPHA, COULOMB, torch.tensor(first[4]), reciprocal=True)
    x, c, tb = (torch.tensor(t, device=DEV) for t in first[:3])
    x.requires_grad_(); c.requires_grad_()
    offsets, f_ref = first[3], f64.cotangents(len(first[1]), 12, torch.float32)[0].to(DEV)

    def step():
        e = pme.compute_direct_frames(x, c, CUTOFF, tb, offsets, twice_differentiable=True) + \
            pme.compute_reciprocal_frames(x, c, tb, offsets, twice_differentiable=True)
        F = -torch.autograd.grad(e.sum(), x, create_graph=True)[0]
        return torch.autograd.grad(((F - f_ref) ** 2).sum(), (x, c))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()                                                               # warm-up: tables, moduli, FFT plans
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        in_graph = step()
    with torch.no_grad():
        x.copy_(torch.tensor(second[0], device=DEV)); c.copy_(torch.tensor(second[1], device=DEV)); tb.copy_(torch.tensor(second[2], device=DEV))
    eager = step()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(in_graph, eager)) and bool(eager[0].any()) and bool(eager[1].any())


def test_refusals():
    pos, q, boxes, offsets, excl = judge.batch((9, 5), seed=141)
    x, c = torch.tensor(pos, device=DEV, requires_grad=True), torch.tensor(q, device=DEV, requires_grad=True)
    tb = torch.tensor(boxes, device=DEV)
    pme = PME(*GRID, ORDER, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True)
    for call in (lambda **kw: pme.compute_direct_frames(x, c, CUTOFF, kw.pop("box", tb), offsets, twice_differentiable=True, **kw),
                 lambda **kw: pme.compute_reciprocal_frames(x, c, kw.pop("box", tb), offsets, twice_differentiable=True, **kw)):
        with pytest.raises(RuntimeError, match="box_gradient"):
            call(box_gradient=True)
        with pytest.raises(RuntimeError, match="box"):
            call(box=tb.clone().requires_grad_())
        P = torch.autograd.grad(call().sum(), x, create_graph=True)[0]
        H = torch.autograd.grad((P ** 2).sum(), x, create_graph=True)[0]
        with pytest.raises(RuntimeError, match="third derivatives"):
            torch.autograd.grad(H.sum(), x)
    with pytest.raises(ValueError, match="order 4 or 5"):
        PME(8, 8, 16, 6, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True).compute_reciprocal_frames(x, c, tb, offsets, twice_differentiable=True)
