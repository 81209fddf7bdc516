"""Every reciprocal pass of PME over frames on the MI355X (pme_frames.hip, pme_frames_second_order.hip) against float64, frame by frame,
at the edges of the passes' loops: a flush of the spread's LDS slots at partial fill, an exact fill without a flush, several flushes, a
round and a wave that keep nothing, the convolution's and the box gradient's second trip round their capped stride, and every regime of
the cyclic stencil test.  tests/pme_frames_passes_reference.py holds the walk restated on the host and the cases,
tests/test_pme_frames_passes_reference_cpu.py the proof that each case reaches its event; this file runs
capi.pme_reciprocal_frames_passes on them.

Each pass is judged with the DEVICE's own input to that pass, widened to float64, so an error belongs to one kernel: the spread from the
positions, the convolution from the device's rfftn of that frame, the interpolation from the device's potential grid.  Every frame is
judged in its own box -- neighbouring frames never share one -- so a pass that read another frame's box or slab would show.  Every
figure is max|device - float64| / max|float64| over one frame (energies: relative), the worst frame is reported, and every figure is
printed before anything is asserted.  A bar is the worst figure measured on the MI355X over all cases x 10, one digit, and never looser
than the single-system passes' bar (DESIGN.md s8e lists the measurements); the 10 x is for the seed-to-seed variation of float32
sums.

The transforms between the passes are torch's, taken in two steps (real along z, complex over (x, y)) by the wrapper and the ops alike:
the library's single batched 3-D real transform returned wrong values for some shapes after transforms of other shapes in the same
process, which this file's sweep was the first to show (docs/LAB_NOTEBOOK_pme_frames_passes.md)."""
import functools
import math

import pytest
import torch

import pme_float64 as f64
import pme_frames_passes_reference as fr
import pme_recip_passes_reference as ref
from nnpops_amd import capi

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ALPHA, COULOMB = fr.ALPHA, fr.COULOMB

# bars: worst figure measured on the MI355X over all cases (in the comment, with the case that set it) x 10, one digit, capped by the
# single-system passes' bars (tests/test_pme_reciprocal_passes_gpu.py: 2e-4, 2e-6, 2e-6, (7e-5, 1e-5))
BAR_SPREAD = 1e-4                        # real grid, and its sum: measured 1.00e-5 (stride-5), 5.9e-8 (empty-round)
BAR_SCALED = 2e-6                        # scaled complex grid: measured 2.58e-7 (stride-5)
BAR_CONVOLVE_ENERGY = 2e-6               # energy from the device's rfftn: measured 1.62e-7 (partial-flush)
BAR_INTERPOLATE = (7e-5, 1e-5)           # dE/dpositions, dE/dcharges from the device's potential grid: measured 1.52e-5 (the three-atom
                                         # frame of empty-round; at most 4.65e-6 in every other frame: 10 x would pass the cap, which
                                         # stays), 1.13e-6 (partial-flush-4)
assert (BAR_SPREAD, BAR_SCALED, BAR_CONVOLVE_ENERGY, BAR_INTERPOLATE) == (fr.BAR_SPREAD, fr.BAR_SCALED, fr.BAR_CONVOLVE_ENERGY,
                                                                          fr.BAR_INTERPOLATE)        # the sensitivity tests' bars
assert BAR_SPREAD <= ref.BAR_SPREAD and BAR_SCALED <= ref.BAR_SCALED and BAR_CONVOLVE_ENERGY <= ref.BAR_CONVOLVE_ENERGY and \
    all(a <= b for a, b in zip(BAR_INTERPOLATE, ref.BAR_INTERPOLATE))      # none looser than the single-system pass it restates
# no pass may be given more room than the whole: the project's end-to-end bars for the same kind of quantity
BAR_END_ENERGY, BAR_END_DERIVATIVE = 1e-5, 1e-4
assert BAR_CONVOLVE_ENERGY <= BAR_END_ENERGY and max(BAR_INTERPOLATE) <= BAR_END_DERIVATIVE
BAR_BOX = 1e-4                           # dE/dbox of a frame, of its largest entry (tests/test_pme_frames_box_gpu.py)
                                         # measured 4.66e-6 (stride-4)
BAR_SECOND = (1e-4, 1e-5, 3e-5)          # dL/dx, dL/dq, dL/dg of pme_reciprocal_frames_twice on the loop cases: measured 1.11e-5
                                         # (stride-4), 1.32e-6 (stride-5), 3.47e-6 (partial-flush-4); 10 x, capped at 1e-4


def on_device(c):
    return tuple(torch.tensor(c[k], device=DEV) for k in ("pos", "q", "boxes")) + (capi.pme_frames_table(c["offsets"]).to(DEV),)


def passes(c, box=False):
    out = capi.pme_reciprocal_frames_passes(*on_device(c), *c["grid"], c["order"], ALPHA, COULOMB, *[m.to(DEV) for m in fr.moduli(c)], box=box)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


@functools.lru_cache(maxsize=None)
def device_passes(name):
    """capi.pme_reciprocal_frames_passes twice on a case -> the two calls' outputs on the host"""
    return [passes(fr.case(name)) for _ in range(2)]


def worst(figures):
    return max(figures) if figures else 0.0


def check_spread(label, c, real32, spread64):
    """the worst frame's figures of a batch's spread grids, after the checks every spread passes whatever its figure"""
    assert not bool(torch.isnan(real32).any()), f"{label}: a grid point was not written"
    figures, totals = [], []
    for m, a, b in fr.frames_of(c):
        if b == a:
            assert not real32[m].any(), f"{label}: the empty frame {m} is not all zeros"
            continue
        f = fr.frame_case(c, m)
        q = torch.tensor(f["q"]).double()
        figures.append(ref.rel(real32[m].double(), spread64[m]))
        totals.append(abs(float(real32[m].double().sum()) - float((q * math.sqrt(COULOMB)).sum())) / float((q.abs() * math.sqrt(COULOMB)).sum()))
        visible = ref.smallest_atom_at_a_point(f) / float(spread64[m].abs().max())
        print(f"{label} frame {m}: spread {figures[-1]:.2e}  grid sum (of sum |q| sqrt(coulomb)) {totals[-1]:.2e}  one atom at one point {visible:.2e}")
        assert BAR_SPREAD <= 0.1 * visible, (label, m, visible)            # the bar sees one atom missing from one point
    return worst(figures), worst(totals)


def end_to_end_figures(c, energies, pos_deriv, charge_deriv, judged):
    e64, gp, gq = judged[:3]
    fe, fp, fq = [], [], []
    for m, a, b in fr.frames_of(c):
        if b == a:
            assert float(energies[m]) == 0.0
            continue
        fe.append(abs(float(energies[m]) - float(e64[m])) / abs(float(e64[m])))
        fp.append(ref.rel(pos_deriv[a:b].double(), gp[a:b]))
        fq.append(ref.rel(charge_deriv[a:b].double(), gq[a:b]))
    return worst(fe), worst(fp), worst(fq)


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_spread_against_float64(name):
    c = fr.case(name)
    figure, total_figure = check_spread(name, c, device_passes(name)[0][0], fr.spread_of(name))
    print(f"{name}: spread {figure:.2e}  grid sum {total_figure:.2e}")
    assert figure <= BAR_SPREAD and total_figure <= BAR_SPREAD


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_convolve_against_float64_from_the_device_rfftn(name):
    c = fr.case(name)
    _, before, scaled, _, energies, _, _ = device_passes(name)[0]
    assert not bool(torch.isnan(torch.view_as_real(scaled)).any())
    figures, energy_figures = [], []
    for m, a, b in fr.frames_of(c):
        if b == a:
            assert not torch.view_as_real(scaled[m]).any() and float(energies[m]) == 0.0
            continue
        box = torch.tensor(c["boxes"][m]).double()
        scaled64, energy64 = ref.convolve64(before[m].to(torch.complex128), box, c["grid"], ALPHA, fr.moduli(c))
        figures.append(float((scaled[m].to(torch.complex128) - scaled64).abs().max()) / float(scaled64.abs().max()))
        energy_figures.append(abs(float(energies[m]) - float(energy64)) / abs(float(energy64)))
        print(f"{name} frame {m}: scaled grid {figures[-1]:.2e}  energy {energy_figures[-1]:.2e}")
    assert worst(figures) <= BAR_SCALED and worst(energy_figures) <= BAR_CONVOLVE_ENERGY


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_interpolate_against_float64_from_the_device_potential(name):
    c = fr.case(name)
    phi, pos_deriv, charge_deriv = (device_passes(name)[0][k] for k in (3, 5, 6))
    assert not bool(torch.isnan(phi).any())
    figures = [[], []]
    for m, a, b in fr.frames_of(c):
        if b == a:
            continue
        gp, gq = ref.interpolate64(phi[m].double(), *ref.case64(fr.frame_case(c, m)), c["grid"], c["order"], COULOMB)
        figures[0].append(ref.rel(pos_deriv[a:b].double(), gp))
        figures[1].append(ref.rel(charge_deriv[a:b].double(), gq))
        print(f"{name} frame {m}: dE/dpositions {figures[0][-1]:.2e}  dE/dcharges {figures[1][-1]:.2e}")
    assert worst(figures[0]) <= BAR_INTERPOLATE[0] and worst(figures[1]) <= BAR_INTERPOLATE[1]


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_end_to_end_against_autograd_of_spme_energy(name):
    c = fr.case(name)
    figures = end_to_end_figures(c, *device_passes(name)[0][4:], fr.autograd_of(name))
    print(f"{name}: end to end energy {figures[0]:.2e}  dE/dpositions {figures[1]:.2e}  dE/dcharges {figures[2]:.2e}")
    assert figures[0] <= BAR_END_ENERGY and figures[1] <= BAR_END_DERIVATIVE and figures[2] <= BAR_END_DERIVATIVE


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_second_call_equals_the_first_bit_for_bit(name):
    first, second = device_passes(name)
    names = ("real grids", "complex grids", "scaled grids", "potential grids", "energies", "dE/dpositions", "dE/dcharges")
    for what, a, b in zip(names, first, second):
        # (NaN != NaN: a point left unwritten fails here as well as in the spread's test)
        assert torch.equal(a, b), (name, what)


def op_outputs(c, op, box=False):
    pos, q, boxes, table = on_device(c)
    pos.requires_grad_()
    q.requires_grad_()
    boxes.requires_grad_(box)
    e = op(pos, q, boxes, table, *c["grid"], c["order"], ALPHA, COULOMB, *[m.to(DEV) for m in fr.moduli(c)])
    grads = torch.autograd.grad(e.sum(), (pos, q, boxes) if box else (pos, q))
    return (e.detach().cpu(),) + tuple(g.cpu() for g in grads)


@pytest.mark.parametrize("name", ["partial-flush", "stride-4"])
def test_pme_reciprocal_frames_is_the_tail_of_the_passes_and_the_op_returns_the_same_bits(name):
    """capi.pme_reciprocal_frames became a call of pme_reciprocal_frames_passes: torch.ops.pme.pme_reciprocal_frames, which goes through
    neither, still returns the same bits"""
    import NNPOps  # noqa: F401  (loads the torch ops)
    c = fr.case(name)
    first = device_passes(name)[0]
    out = capi.pme_reciprocal_frames(*on_device(c), *c["grid"], c["order"], ALPHA, COULOMB, *[m.to(DEV) for m in fr.moduli(c)])
    torch.cuda.synchronize()
    for a, b in zip(out, first[4:]):
        assert torch.equal(a.cpu(), b)
    for a, b in zip(op_outputs(c, torch.ops.pme.pme_reciprocal_frames), first[4:]):
        assert torch.equal(a, b)


# ---- the loops copied into the box gradient's Pi and the second-order spread and interpolation: end to end, on the loop cases ---------
@pytest.mark.parametrize("name", fr.LOOP_CASES)
def test_box_gradient_against_autograd_of_spme_energy(name):
    """pme_recip_box_pi_frames strides as the convolution does (stride-4, stride-5); pme_recip_box_finish_frames reads the frame's
    atoms 256 at a time.  The pass has no C-level intermediate to cut at: judged end to end with the frame's box as the leaf."""
    import NNPOps  # noqa: F401  (loads the torch ops)
    c = fr.case(name)
    out = passes(c, box=True)
    gb64 = fr.autograd_of(name)[3]
    figures = []
    for m, a, b in fr.frames_of(c):
        if b == a:
            assert not out[7][m].any()
            continue
        figures.append(ref.rel(out[7][m].double(), gb64[m]))
        print(f"{name} frame {m}: dE/dbox {figures[-1]:.2e}")
    first = device_passes(name)[0]
    assert all(torch.equal(a, b) for a, b in zip(out[:7], first)), name       # the box passes leave every other output its bits
    for a, b in zip(op_outputs(c, torch.ops.pme.pme_reciprocal_frames_box, box=True), out[4:]):
        assert torch.equal(a, b), name
    assert worst(figures) <= BAR_BOX


@pytest.mark.parametrize("name", fr.LOOP_CASES)
def test_second_order_against_second_order_of_spme_energy(name):
    """torch.ops.pme.pme_reciprocal_frames_twice: pme_recip_spread_dir_frames walks, ranks and flushes as the spread does,
    pme_recip_interp2_frames reads per-frame slabs, and the convolution between them strides.  dL/dx, dL/dq, dL/dg per frame against
    pme_float64.second_order of spme_energy with the frame's box."""
    import NNPOps  # noqa: F401  (loads the torch ops)
    c = fr.case(name)
    n, B = len(c["q"]), len(c["offsets"]) - 1
    g = [0.5 + 0.125 * m for m in range(B)]
    v, w = f64.cotangents(n, 21, torch.float32)
    pos, q, boxes, table = on_device(c)
    pos.requires_grad_()
    q.requires_grad_()
    gt = torch.tensor(g, dtype=torch.float32, device=DEV, requires_grad=True)
    e = torch.ops.pme.pme_reciprocal_frames_twice(pos, q, boxes, table, *c["grid"], c["order"], ALPHA, COULOMB, *[m.to(DEV) for m in fr.moduli(c)])
    P, C = torch.autograd.grad((gt * e).sum(), (pos, q), create_graph=True)
    gx, gq, gg = (t.detach().cpu() for t in torch.autograd.grad((v.to(DEV) * P).sum() + (w.to(DEV) * C).sum(), (pos, q, gt)))
    first = device_passes(name)[0]
    assert torch.equal(e.detach().cpu(), first[4])                             # the energies: the default path's bits
    figures = [[], [], []]
    for m, a, b in fr.frames_of(c):
        if b == a:
            assert float(gg[m]) == 0.0
            continue
        f = fr.frame_case(c, m)
        x64, c64, box64 = ref.case64(f)
        gm = torch.tensor(g[m], dtype=torch.float64, requires_grad=True)
        want = f64.second_order(lambda xx, cc: fr.spme_energy(xx, cc, box64, c["grid"], c["order"], ALPHA, COULOMB, fr.moduli(c)),
                                x64.requires_grad_(), c64.requires_grad_(), gm, v[a:b].double(), w[a:b].double())[3:]
        figures[0].append(ref.rel(gx[a:b].double(), want[0]))
        figures[1].append(ref.rel(gq[a:b].double(), want[1]))
        figures[2].append(abs(float(gg[m]) - float(want[2])) / abs(float(want[2])))
        print(f"{name} frame {m}: dL/dx {figures[0][-1]:.2e}  dL/dq {figures[1][-1]:.2e}  dL/dg {figures[2][-1]:.2e}")
    assert all(worst(f) <= bar for f, bar in zip(figures, BAR_SECOND)), (name, [worst(f) for f in figures])


# ---- the sweep: the spread and the end-to-end derivatives at every grid ---------------------------------------------------------------
@pytest.mark.parametrize("order", [4, 5])
def test_window_sweep(order):
    worst_spread, worst_end = (-1.0, None), (-1.0, None)
    failed = []
    for _, grid in fr.SWEEP:
        c = fr.sweep_case(grid, order)
        out = passes(c)
        figure, total_figure = check_spread(f"order {order} grid {grid}", c, out[0], fr.spread_frames64(c))
        if fr.has_a_float64_energy(c):
            end = end_to_end_figures(c, *out[4:], fr.autograd_frames64(c))
            print(f"order {order} grid {grid}: end to end energy {end[0]:.2e}  dE/dpositions {end[1]:.2e}  dE/dcharges {end[2]:.2e}")
        else:                                # a one-point axis: the modulus is 0 and the float64 energy infinite too -- the spread alone
            assert 1 in grid, grid
            end = (0.0, 0.0, 0.0)
        worst_spread, worst_end = max(worst_spread, (figure, grid)), max(worst_end, (max(end[1:]), grid))
        if figure > BAR_SPREAD or total_figure > BAR_SPREAD or end[0] > BAR_END_ENERGY or max(end[1:]) > BAR_END_DERIVATIVE:
            failed.append((grid, figure, total_figure, end))
    print(f"window sweep order {order}: worst spread figure {worst_spread[0]:.2e} at {worst_spread[1]}, worst end-to-end derivative "
          f"{worst_end[0]:.2e} at {worst_end[1]}")
    assert not failed, failed
