"""Direct-space PME on the MI355X at the edges of its two summation paths, against float64.

The delivering path (pme_direct_pairs + pme_direct_gather: incoming rows of `cap` entries, a float-atomic spill array behind
them, a per-wave segmented scan over runs of equal first atoms) and the indexed path (pme_direct_terms +
pme_direct_gather_indexed) are run through capi.pme_direct on the inputs of tests/pme_direct_reference.py -- exactly at cap, a
dense cluster among lonely atoms, an all-pairs list beyond the clamp of cap and of the slot kernels' grid, more atoms than the
atom kernels' grid serves, hand-made runs over wave and workgroup boundaries, exclusion rows longer than a group of 16 lanes,
lists without a pair -- and judged by that module's float64 sums over the SAME list:

* the project's bars (test_pme_gpu.py): the energy within 1e-5 of the sum of |pair energies|, the derivatives within 1e-4 of the
  largest component;
* per atom and component |got - ref| <= c 2^-23 sum_k |term_k| + one float32 ulp of the result, which a wrong or missing term of
  a weakly loaded atom cannot hide under.  c = 16 is measured, not chosen: the float32-term, float64-sum oracle reaches a ratio
  of 3.78 against the judge over all these inputs (test_pme_direct_reference_cpu.py::test_per_atom_bar_is_the_measured_one);
  times 4 for the device's erfcf / expf, rounded up to a power of two.  Atoms nothing contributes to get exact zeros;
* the same bits on a second call wherever nothing spills (the energy and the indexed path: always); both paths within 2e-6 of
  the largest component of each other there;
* every call with a workspace of exactly the advertised size, 256-byte aligned, between guard patterns that must survive.
"""
import numpy as np
import pytest
import torch

import pme_direct_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device_list(case):
    """-> ((neighbors, deltas, distances) on the device, from the forward op?)."""
    from nnpops_amd import capi
    if "list" in case:
        nb, dl, ds = case["list"]
        return (torch.tensor(nb, dtype=torch.int32, device=DEV), torch.tensor(dl, device=DEV), torch.tensor(ds, device=DEV)), False
    f = case["forward"]
    box = None if f["box"] is None else torch.tensor(f["box"], device=DEV)
    nb, dl, ds, found = capi.neighbor_pairs_forward(torch.tensor(case["pos"], device=DEV), f["cutoff"], f["slots"], box)
    assert 0 < int(found) <= f["slots"]
    return (nb, dl, ds), True


def _within(name, what, got, want, mag):
    """The project's bar and the per-atom bar on one derivative; the figures are printed first."""
    got = got.double().cpu().numpy()
    top = np.abs(want).max()
    worst = np.abs(got - want).max()
    ratio = ref.per_atom_ratio(got, want, mag)
    print(f"{name} {what}: largest error {worst:.3e} of largest component {top:.3e}; per-atom ratio {ratio:.2f} (bar {ref.PER_ATOM_C:g})")
    assert worst <= ref.DERIV_BAR * top, (name, what)
    assert (got[mag == 0] == 0).all(), (name, what)
    assert (np.abs(got - want) <= ref.PER_ATOM_C * ref.EPS32 * mag + ref.ulp32(want)).all(), (name, what, ratio)


def _check(name, case):
    from nnpops_amd import capi
    n = len(case["pos"])
    (nb, dl, ds), compacted = _device_list(case)
    pos, q = torch.tensor(case["pos"], device=DEV), torch.tensor(case["q"], device=DEV)
    excl = torch.tensor(case["excl"], dtype=torch.int32, device=DEV)
    host = [t.cpu().numpy() for t in (nb, dl, ds)]
    j = ref.judge(case["pos"], case["q"], *host, case["excl"], case["alpha"], case["coulomb"])
    spilling = ref.spilling_atoms(host[0], case["excl"], n)
    paths = {"delivering": None}
    if compacted:
        paths["indexed"] = capi.neighbor_pairs_build_index(n, nb)
    results = {}
    for path, index in paths.items():
        run = lambda: capi.pme_direct(pos, q, nb, dl, ds, excl, case["alpha"], case["coulomb"], index=index, workspace_guard=True)
        e, pd, cd = run()
        e2, pd2, cd2 = run()
        print(f"{name} {path}: energy error {abs(float(e) - j['energy']):.3e} of {j['energy_mag']:.3e}; {len(spilling)} atoms spill")
        assert abs(float(e) - j["energy"]) <= ref.ENERGY_BAR * j["energy_mag"], (name, path)
        _within(f"{name} {path}", "dE/dpositions", pd, j["pos_deriv"], j["pos_mag"])
        _within(f"{name} {path}", "dE/dcharges", cd, j["charge_deriv"], j["charge_mag"])
        assert torch.equal(e, e2), (name, path)
        if path == "indexed" or len(spilling) == 0:
            assert torch.equal(pd, pd2) and torch.equal(cd, cd2), (name, path)
        results[path] = (e, pd, cd)
    if compacted and len(spilling) == 0:
        (e_d, pd_d, cd_d), (e_i, pd_i, cd_i) = results["delivering"], results["indexed"]
        assert float((pd_i - pd_d).abs().max()) <= ref.PATHS_BAR * float(pd_d.abs().max()), name
        assert float((cd_i - cd_d).abs().max()) <= ref.PATHS_BAR * float(cd_d.abs().max()), name
    return results, host, spilling


@pytest.mark.parametrize("k", ref.CAP_CASE_K)
def test_row_exactly_at_its_capacity(k):
    """64 atoms, 64 slots, pairs (j, 0) for j = 1..k: atom 0's row of 36 entries not yet full, just full, one entry spilled, 27
    spilled -- and each entry is at least 10 bars of the largest component, atom 0's own."""
    _, _, spilling = _check(f"cap-{k}", ref.cap_case(k))
    assert list(spilling) == ([0] if k > 36 else [])


def test_dense_cluster_spills_naturally():
    """200 atoms within the cutoff of each other among 5 800 lonely ones, 20 000 slots (cap 48): the cluster's atoms receive up to
    199 entries; both paths."""
    case = ref.cluster_case()
    results, host, spilling = _check("cluster", case)
    assert len(spilling) > 100 and np.isin(spilling, case["cluster"]).all()
    assert len(results) == 2


def test_all_pairs_list_beyond_the_clamps():
    """2 100 atoms, all 2 203 950 pairs in a compacted list: cap clamps at 2 048 (atoms 0..50 and a few more spill) and the slot
    kernels stride three times over real pairs; both paths."""
    case = ref.clamp_case()
    results, host, spilling = _check("clamp", case)
    assert (host[0] > -1).all() and host[0].shape[1] == 2100 * 2099 // 2
    assert len(spilling) >= 51 and list(spilling) == list(range(len(spilling)))
    assert len(results) == 2


def test_more_atoms_than_the_atom_kernels_grid():
    """65 536 + 21 atoms, periodic: the atoms from 65 536 on are served by the second trip of pme_direct_gather's loop, the last
    group of 16 lanes is ragged; they carry non-zero derivatives and each is held to the per-atom bar like every other atom."""
    case = ref.many_case()
    results, host, spilling = _check("many", case)
    assert len(spilling) == 0 and len(results) == 2
    for e, pd, cd in results.values():
        assert bool((pd[65536:] != 0).all()) and bool((cd[65536:] != 0).all())


@pytest.mark.parametrize("variant", ref.RUN_VARIANTS)
@pytest.mark.parametrize("total,length,first", ref.run_shapes())
def test_runs_over_wave_and_workgroup_boundaries(total, length, first, variant):
    """Hand-made lists of 1, 255, 256 and 257 slots in which one first atom owns 1 to 129 consecutive slots from lane 0, from lane
    37, or up to the end of the list; with an excluded slot in the middle of the run, with -1 slots interleaved, and shuffled."""
    _check(f"run-{variant}-{total}-{length}-{first}", ref.run_case(total, length, first, variant))


@pytest.mark.parametrize("max_excl", ref.EXCLUSION_WIDTHS)
def test_exclusion_rows_of_every_fill(max_excl):
    """300 atoms, periodic, exclusion rows of 0 to max_excl entries (padding from every column on), excluded pairs in the list,
    beyond the cutoff, and listed with a wrapped delta (the erf() part is taken un-wrapped), a self entry; both paths."""
    results, _, spilling = _check(f"excl-{max_excl}", ref.exclusion_case(max_excl))
    assert len(spilling) == 0 and len(results) == 2


@pytest.mark.parametrize("slots", ref.EMPTY_SLOTS)
def test_list_without_a_pair(slots):
    """No pair (0 slots; 7 slots of -1) and a table of exclusions: only the erf() terms remain, atoms without any get exact zeros."""
    case = ref.empty_case(slots)
    results, _, _ = _check(f"empty-{slots}", case)
    e, pd, cd = results["delivering"]
    lonely = torch.tensor(case["lonely"], device=DEV)
    assert bool((pd[lonely] == 0).all()) and bool((cd[lonely] == 0).all()) and float(e) != 0.0
