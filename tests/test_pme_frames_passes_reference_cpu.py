"""The float64 judge of the reciprocal passes of PME over frames (tests/pme_frames_passes_reference.py: meets, slot_walk,
spread64_by_walk and the cases at which the walk of pme_recip_spread_frames flushes), checked where no GPU is needed:

  * meets agrees with the brute-force intersection of the stencil's points with the brick's points, for every K in 1..40;
  * the spread restated as the walk does it equals the scatter, and the three passes composed per frame agree with autograd of
    spme_energy with that frame's box to 1e-11;
  * every named case reaches the event it was built for according to slot_walk, `stride` the convolution's second trip, the sweep every
    regime of the cyclic window on every axis; every atom stays MARGIN cells from a cell edge;
  * a walk with one of its possible defects built in (never into a kernel), a convolution with the neighbouring frame's box and an
    interpolation from the neighbouring frame's slab move the case aimed at them by at least 10 x the bar the device comparison uses.

tests/test_pme_frames_passes_gpu.py compares the device's passes with the same module."""
import numpy as np
import pytest
import torch

import pme_frames_passes_reference as fr
import pme_recip_passes_reference as ref


# ---- meets --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [4, 5])
@pytest.mark.parametrize("width", [4, 16])
def test_meets_against_the_intersection_of_the_two_point_sets(order, width):
    for K in range(1, 41):
        g0 = np.arange(K)
        for lo in range(0, K, width):
            hi = min(lo + width, K) - 1
            brick = set(range(lo, hi + 1))
            brute = np.array([bool({(g + i) % K for i in range(order)} & brick) for g in g0])
            assert np.array_equal(fr.meets(g0, lo, hi, K, order), brute), (K, lo, hi, order)


def test_the_built_in_slips_of_meets_leave_atoms_out_and_never_add_one():
    g0 = np.arange(16)
    true = fr.meets(g0, 0, 3, 16, 5)
    assert list(g0[true & ~fr.meets(g0, 0, 3, 16, 5, wrap_ahead=False)]) == [12, 13, 14, 15]
    assert list(g0[true & ~fr.meets(g0, 0, 3, 16, 5, behind_inclusive=False)]) == [3]
    for how in ({"wrap_ahead": False}, {"behind_inclusive": False}):
        assert not (fr.meets(g0, 0, 3, 16, 5, **how) & ~true).any()


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def frames64(c):
    """(m, pos, q, box) float64 of every frame with atoms"""
    return [(m,) + ref.case64(fr.frame_case(c, m)) for m, a, b in fr.frames_of(c) if b > a]


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_walk_restatement_equals_the_scatter(name):
    c = fr.case(name)
    for m, pos, q, box in frames64(c):
        by_walk = fr.spread64_by_walk(pos, q, box, c["grid"], c["order"], fr.COULOMB)
        assert ref.rel(by_walk, fr.spread_of(name)[m]) <= 1e-13, (name, m)


@pytest.mark.parametrize("order", [4, 5])
def test_sweep_walk_restatement_equals_the_scatter_and_reaches_every_regime_of_the_window(order):
    seen = [set(), set(), set()]
    for axis, grid in fr.SWEEP:
        c = fr.sweep_case(grid, order)
        assert [b - a for _, a, b in fr.frames_of(c)] == [20, 0, 60]
        assert fr.base_of(c)[1] >= fr.MARGIN, grid
        assert len({tuple(b.reshape(-1)) for b in c["boxes"]}) == len(c["boxes"])
        seen[axis] |= ref.window_classes(grid[axis], ref.BRICK[axis], order)
        # the end-to-end judge exists on every grid but those with a one-point axis, whose modulus is exactly 0
        assert fr.has_a_float64_energy(c) == (1 not in grid), grid
        assert bool(torch.isfinite(fr.autograd_frames64(c)[0]).all()) == (1 not in grid), grid
        for m, pos, q, box in frames64(c):
            assert ref.rel(fr.spread64_by_walk(pos, q, box, grid, order, fr.COULOMB), ref.spread64(pos, q, box, grid, order, fr.COULOMB)) <= 1e-13
    assert all(s == ref.ALL_WINDOW_CLASSES for s in seen), seen


@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_composition_of_the_passes_agrees_with_autograd_of_spme_energy_per_frame(name):
    c = fr.case(name)
    e_ref, gp_ref, gq_ref, _ = fr.autograd_of(name)
    for m, pos, q, box in frames64(c):
        a, b = c["offsets"][m], c["offsets"][m + 1]
        scaled, energy = ref.convolve64(torch.fft.rfftn(fr.spread_of(name)[m]), box, c["grid"], fr.ALPHA, fr.moduli(c))
        phi = torch.fft.irfftn(scaled, s=c["grid"], norm="forward")
        gp, gq = ref.interpolate64(phi, pos, q, box, c["grid"], c["order"], fr.COULOMB)
        figures = (abs(float(energy) - float(e_ref[m])) / abs(float(e_ref[m])), ref.rel(gp, gp_ref[a:b]), ref.rel(gq, gq_ref[a:b]))
        print(f"{name} frame {m}: energy {figures[0]:.1e}  dE/dpositions {figures[1]:.1e}  dE/dcharges {figures[2]:.1e}")
        assert max(figures) <= 1e-11, (m, figures)


# ---- the cases reach their events ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.CASE_NAMES)
def test_case_is_built_as_stated(name):
    c = fr.case(name)
    sizes = [b - a for _, a, b in fr.frames_of(c)]
    assert fr.base_of(c)[1] >= fr.MARGIN
    assert float(torch.tensor(c["q"]).abs().min()) >= 0.1 - 1e-7
    boxes = [tuple(b.reshape(-1)) for b in c["boxes"]]
    assert all(x != y for x, y in zip(boxes, boxes[1:]))                    # neighbouring frames never share a box
    assert c["offsets"][-2] % fr.ROUND != 0                                 # the last frame's atoms do not start a per-atom workgroup
    for m, pos, q, box in frames64(c):                                      # a third of a frame's atoms lie outside its box
        s = pos @ torch.linalg.inv(box)
        assert bool(((s < 0) | (s >= 1)).any()) or len(q) < 3, (name, m)
    if name.startswith("partial-flush"):
        assert sizes == [7, 0, 300]


def target(name):
    c = fr.case(name)
    return fr.walk_of(name)[(len(c["offsets"]) - 2, fr.TARGET_BRICK)]


@pytest.mark.parametrize("name", ["partial-flush", "partial-flush-4"])
def test_partial_flush_flushes_partly_filled_slots(name):
    w = target(name)
    assert w.rounds == [250, 44] and w.flushes == [250] and w.final == 44
    assert 0 < w.flushes[0] < fr.ROUND and w.rounds[1] >= 40
    assert len(set(w.waves[0])) > 1                                         # the waves' counts differ: the ranks need them
    # and the bricks around the target flush at other fills, or not at all
    c = fr.case(name)
    fills = {f for (m, _), other in fr.walk_of(name).items() if m == len(c["offsets"]) - 2 for f in other.flushes}
    print(f"{name}: fills at a flush over the frame's bricks {sorted(fills)}")
    assert all(0 < f <= fr.ROUND for f in fills)


def test_exact_fill_fills_the_last_slot_without_a_flush():
    w = target("exact-fill")
    assert w.rounds == [200, 56] and w.flushes == [] and w.final == fr.ROUND and w.last_slot == fr.ROUND - 1


def test_three_flushes_flushes_three_times():
    w = target("three-flushes")
    assert w.rounds == [230, 230, 230, 32] and w.flushes == [230, 230, 230] and w.final == 32


def test_empty_round_keeps_nothing_between_two_rounds_that_keep_some():
    w = target("empty-round")
    assert w.rounds == [100, 0, 50] and w.flushes == [] and w.final == 150
    # several sparse rounds accumulating, over the frame's other bricks too
    c = fr.case("empty-round")
    assert any(len(o.rounds) == 3 and all(0 < r < fr.ROUND for r in o.rounds) and not o.flushes
               for (m, _), o in fr.walk_of("empty-round").items() if m == len(c["offsets"]) - 2)


def test_idle_wave_has_a_wave_that_keeps_nothing_before_waves_that_keep_some():
    w = target("idle-wave")
    assert w.waves == [[64, 0, 30, 44]] and w.flushes == []


@pytest.mark.parametrize("name", ["stride-4", "stride-5"])
def test_stride_takes_the_convolution_round_its_loop_twice(name):
    c = fr.case(name)
    gx, gy, gz = c["grid"]
    points = gx * gy * (gz // 2 + 1)
    assert points == 298656 and fr.CONVOLVE_PASS < points < 2 * fr.CONVOLVE_PASS
    assert [b - a for _, a, b in fr.frames_of(c)] == [300, 40]
    assert any(len(w.rounds) == 2 and w.rounds[1] > 0 for w in fr.walk_of(name).values())       # some brick keeps atoms of the second round


# ---- sensitivity: each defect moves its pass's figure to at least 10 x that pass's bar ----------------------------------------------
def moved_by(name, **defect):
    c = fr.case(name)
    m = len(c["offsets"]) - 2
    defective = fr.spread64_by_walk(*ref.case64(fr.frame_case(c, m)), c["grid"], c["order"], fr.COULOMB, **defect)
    return ref.rel(defective, fr.spread_of(name)[m])


@pytest.mark.parametrize("name,defect", [
    ("partial-flush", "forget_on_flush"), ("partial-flush-4", "forget_on_flush"), ("three-flushes", "forget_on_flush"),
    ("exact-fill", "flush_drops_round"), ("partial-flush", "flush_drops_round"),
    ("idle-wave", "ranks_ignore_waves"), ("partial-flush", "ranks_ignore_waves"), ("exact-fill", "ranks_ignore_waves"),
])
def test_a_defect_of_the_walk_would_be_seen(name, defect):
    moved = moved_by(name, **{defect: True})
    print(f"{name}: {defect}: the spread moves by {moved:.2e}")
    assert moved >= 10 * fr.BAR_SPREAD


@pytest.mark.parametrize("name", ["empty-round", "exact-fill"])
@pytest.mark.parametrize("slip", ["wrap_ahead", "behind_inclusive"])
def test_a_slip_in_meets_would_be_seen(name, slip):
    moved = moved_by(name, **{slip: False})
    print(f"{name}: meets with {slip}=False: the spread moves by {moved:.2e}")
    assert moved >= 10 * fr.BAR_SPREAD


@pytest.mark.parametrize("order", [4, 5])
def test_a_slip_in_meets_would_be_seen_in_the_sweep(order):
    """on every axis some grid of the sweep sees each slip (a folded or whole-axis stencil meets everything and cannot)"""
    for slip in ("wrap_ahead", "behind_inclusive"):
        seen = set()
        for axis, grid in fr.SWEEP:
            c = fr.sweep_case(grid, order)
            for m, pos, q, box in frames64(c):
                moved = ref.rel(fr.spread64_by_walk(pos, q, box, grid, order, fr.COULOMB, **{slip: False}),
                                ref.spread64(pos, q, box, grid, order, fr.COULOMB))
                if moved >= 10 * fr.BAR_SPREAD:
                    seen.add(axis)
        assert seen == {0, 1, 2}, (slip, seen)


@pytest.mark.parametrize("name", ["partial-flush", "exact-fill", "stride-5"])
def test_the_neighbouring_frames_box_or_slab_would_be_seen(name):
    c = fr.case(name)
    live = frames64(c)
    (m, pos, q, box), (other, _, _, other_box) = live[-1], live[-2]
    S = torch.fft.rfftn(fr.spread_of(name)[m])
    scaled, energy = ref.convolve64(S, box, c["grid"], fr.ALPHA, fr.moduli(c))
    wrong, wrong_energy = ref.convolve64(S, other_box, c["grid"], fr.ALPHA, fr.moduli(c))
    figures = ref.rel(wrong, scaled), abs(float(wrong_energy) - float(energy)) / abs(float(energy))
    print(f"{name}: frame {m} convolved with frame {other}'s box: scaled grid moves by {figures[0]:.2e}, energy by {figures[1]:.2e}")
    assert figures[0] >= 10 * fr.BAR_SCALED and figures[1] >= 10 * fr.BAR_CONVOLVE_ENERGY

    def phi_of(k, b):
        s, _ = ref.convolve64(torch.fft.rfftn(fr.spread_of(name)[k]), b, c["grid"], fr.ALPHA, fr.moduli(c))
        return torch.fft.irfftn(s, s=c["grid"], norm="forward")
    gp, gq = ref.interpolate64(phi_of(m, box), pos, q, box, c["grid"], c["order"], fr.COULOMB)
    wp, wq = ref.interpolate64(phi_of(other, other_box), pos, q, box, c["grid"], c["order"], fr.COULOMB)
    figures = ref.rel(wp, gp), ref.rel(wq, gq)
    print(f"{name}: frame {m} interpolated from frame {other}'s slab: dE/dpositions moves by {figures[0]:.2e}, dE/dcharges by {figures[1]:.2e}")
    assert figures[0] >= 10 * fr.BAR_INTERPOLATE[0] and figures[1] >= 10 * fr.BAR_INTERPOLATE[1]
