"""The float64 judge of every pass of reciprocal-space PME (tests/pme_recip_passes_reference.py: spread64, convolve64, interpolate64,
brick_model and the cases at which the loops of pme_recip.hip repeat), checked where no GPU is needed:

  * the composition of the three passes agrees with autograd of spme_energy (tests/pme_float64.py, the restatement the box
    gradient's tests already trust) to 1e-11;
  * every case reaches the loop it was built to reach, and the window sweep reaches every regime of window_bins;
  * a spread64 / convolve64 with one of the loops' possible defects built in (never into a kernel) moves the case aimed at it by at
    least 10 x the bar the device comparison uses: the bars could see it.

tests/test_pme_reciprocal_passes_gpu.py compares the device's passes with the same module."""
import pytest
import torch

import pme_recip_passes_reference as ref


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_composition_of_the_passes_agrees_with_autograd_of_spme_energy(name):
    c = ref.case(name)
    pos, q, box = ref.case64(c)
    Q = ref.spread_of(name)
    scaled, energy = ref.convolve64(torch.fft.rfftn(Q), box, c["grid"], ref.ALPHA, ref.moduli(c))
    phi = torch.fft.irfftn(scaled, s=c["grid"], norm="forward")
    gp, gq = ref.interpolate64(phi, pos, q, box, c["grid"], c["order"], ref.COULOMB)
    e_ref, gp_ref, gq_ref, _ = ref.autograd_of(name)
    figures = (abs(float(energy) - float(e_ref)) / abs(float(e_ref)), ref.rel(gp, gp_ref), ref.rel(gq, gq_ref))
    print(f"{name}: energy {figures[0]:.1e}  dE/dpositions {figures[1]:.1e}  dE/dcharges {figures[2]:.1e}")
    assert max(figures) <= 1e-11, figures


@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_case_reaches_the_loops_it_was_built_for(name):
    c, m = ref.case(name), ref.model_of(name)
    assert ref.margin_of(m) >= ref.MARGIN
    assert float(torch.tensor(c["q"]).abs().min()) >= 0.1 - 1e-7
    assert int(m.counts.sum()) == len(c["q"])
    complex_points = c["grid"][0] * c["grid"][1] * (c["grid"][2] // 2 + 1)
    if name.startswith("dense"):
        assert int(m.counts.min()) > ref.SORT_PASS                          # the rank sort takes more than one pass in every brick
        assert int(m.staged.max()) > 4 * ref.STAGE_PASS                     # 5 or more staging passes
    elif name == "blob":
        assert int(m.counts.max()) > ref.STAGE_PASS
        assert int((m.staged == 0).sum()) >= m.nbins / 2                # a point nothing reaches is still written, as 0
    elif name.startswith("one-brick"):
        n = len(c["q"])
        brick = (1 * m.nb[1] + 1) * m.nb[2] + 0
        assert int(m.counts[brick]) == n and int(m.staged[brick]) == n
    elif name.startswith("big"):
        assert m.nbins == 2448 and 2 * ref.SCAN_PASS < m.nbins < 3 * ref.SCAN_PASS         # three scan passes, the last one partial
        assert complex_points == 298656 and ref.CONVOLVE_PASS < complex_points < 2 * ref.CONVOLVE_PASS
        assert len(c["q"]) > 256
        assert int(m.counts[2 * ref.SCAN_PASS:].sum()) > 0 and int(m.counts[ref.SCAN_PASS:2 * ref.SCAN_PASS].sum()) > 0
    elif name == "scan-edge":
        assert m.nbins == ref.SCAN_PASS + 1 and int(m.counts[ref.SCAN_PASS]) > 0            # one brick alone in the second pass, with atoms


@pytest.mark.parametrize("order", [4, 5])
def test_window_sweep_reaches_every_regime_of_the_window(order):
    seen = [set(), set(), set()]
    came_back = [False, False, False]
    for a, grid in ref.SWEEP:
        c = ref.sweep_case(grid, order)
        pos, q, box = ref.case64(c)
        m = ref.brick_model(pos, box, grid, order)
        assert ref.margin_of(m) >= ref.MARGIN
        seen[a] |= ref.window_classes(grid[a], ref.BRICK[a], order)
        came_back[a] |= m.comes_back[a]
        for axis in m.windows:
            assert all(len(w) <= 4 and len(set(w)) == len(w) for w in axis)         # kMaxBinsPerAxis, every brick once
        # the owner's view (windows, folding) and the scatter's view of the same spread agree
        assert ref.rel(ref.spread64_by_owner(pos, q, box, grid, order, ref.COULOMB, m),
                       ref.spread64(pos, q, box, grid, order, ref.COULOMB)) <= 1e-13
    assert all(s == ref.ALL_WINDOW_CLASSES for s in seen), seen
    # a window that wraps onto a brick it already holds: along z only (along x and y a window of 4 + order - 1 cells that begins
    # inside a brick of 4 and ends in the same brick covers the whole axis)
    assert came_back == [False, False, True], came_back


@pytest.mark.parametrize("name", ["dense-5", "blob", "one-brick-257", "scan-edge"])
def test_owner_computes_restatement_equals_the_scatter(name):
    c = ref.case(name)
    owner = ref.spread64_by_owner(*ref.case64(c), c["grid"], c["order"], ref.COULOMB, ref.model_of(name))
    assert ref.rel(owner, ref.spread_of(name)) <= 1e-13


# Sensitivity: a defect in one of the loops, built into the restatement (never into a kernel), moves the case aimed at it by at least
# 10 x the bar the device comparison uses.
@pytest.mark.parametrize("name", ["dense-4", "dense-5", "blob", "one-brick-257"])
def test_dropping_the_staged_atoms_beyond_the_first_pass_would_be_seen(name):
    c = ref.case(name)
    defective = ref.spread64_by_owner(*ref.case64(c), c["grid"], c["order"], ref.COULOMB, ref.model_of(name), stage_limit=ref.STAGE_PASS)
    moved = ref.rel(defective, ref.spread_of(name))
    print(f"{name}: only the first {ref.STAGE_PASS} staged atoms of a window: the spread moves by {moved:.2e}")
    assert moved >= 10 * ref.BAR_SPREAD


@pytest.mark.parametrize("name", ["dense-4", "dense-5", "one-brick-65"])
def test_dropping_the_atoms_beyond_the_first_sort_pass_would_be_seen(name):
    c, m = ref.case(name), ref.model_of(name)
    defective = ref.spread64(*ref.case64(c), c["grid"], c["order"], ref.COULOMB, keep=ref.rank_in_brick(m) < ref.SORT_PASS)
    moved = ref.rel(defective, ref.spread_of(name))
    print(f"{name}: only the first {ref.SORT_PASS} atoms of a brick: the spread moves by {moved:.2e}")
    assert moved >= 10 * ref.BAR_SPREAD


@pytest.mark.parametrize("name", ["scan-edge", "big-4"])
def test_restarting_the_brick_prefix_every_scan_pass_would_be_seen(name):
    """Without the carry the ranges of the bricks from the 1024th on start again at 0: their atoms are written over the first
    bricks' (here: the later brick wins), and a range whose end lies before its start is empty."""
    c, m = ref.case(name), ref.model_of(name)
    start = torch.zeros(m.nbins + 1, dtype=torch.long)
    for c0 in range(0, m.nbins, ref.SCAN_PASS):
        chunk = m.counts[c0:c0 + ref.SCAN_PASS]
        start[c0:c0 + len(chunk)] = torch.cumsum(chunk, 0) - chunk
    start[m.nbins] = start[m.nbins - 1] + m.counts[m.nbins - 1]
    by_brick = torch.argsort(m.brick, stable=True)
    true_start = torch.cumsum(m.counts, 0) - m.counts
    array = torch.zeros(len(by_brick), dtype=torch.long)
    for b in range(m.nbins):
        array[start[b]:start[b] + m.counts[b]] = by_brick[true_start[b]:true_start[b] + m.counts[b]]
    defective = ref.spread64_by_owner(*ref.case64(c), c["grid"], c["order"], ref.COULOMB, m, ranges=(array, start))
    moved = ref.rel(defective, ref.spread_of(name))
    print(f"{name}: the brick prefix restarted every {ref.SCAN_PASS} bricks: the spread moves by {moved:.2e}")
    assert moved >= 10 * ref.BAR_SPREAD


@pytest.mark.parametrize("name", ["big-4", "big-5"])
def test_leaving_the_points_beyond_the_first_stride_unscaled_would_be_seen(name):
    c = ref.case(name)
    _, _, box = ref.case64(c)
    S = torch.fft.rfftn(ref.spread_of(name))
    scaled, _ = ref.convolve64(S, box, c["grid"], ref.ALPHA, ref.moduli(c))
    defective, _ = ref.convolve64(S, box, c["grid"], ref.ALPHA, ref.moduli(c), scaled_points=ref.CONVOLVE_PASS)
    moved = ref.rel(defective, scaled)
    print(f"{name}: the points from {ref.CONVOLVE_PASS} on left unscaled: the scaled grid moves by {moved:.2e}")
    assert moved >= 10 * ref.BAR_SCALED
