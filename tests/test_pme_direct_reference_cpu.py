"""The float64 judge of the direct-space PME edge tests (tests/pme_direct_reference.py), and the inputs of those tests, checked
without a GPU: the judge against the reference-made vectors, against the float32 oracle and against autograd of its own energy;
every input against the conditions it was built to meet; and the per-atom bar measured where the GPU test takes it from."""
import math

import numpy as np
import pytest
import torch

import pme_direct_reference as ref
import pme_float64 as f64
from oracle import pme_direct_oracle

_lists = {}


def _case(name):
    """(case, host list, judge's answer) of a named input, built once."""
    if name not in _lists:
        case = dict(ref.all_cases())[name]()
        nb, dl, ds = ref.host_list(case)
        _lists[name] = (case, (nb, dl, ds), ref.judge(case["pos"], case["q"], nb, dl, ds, case["excl"], case["alpha"], case["coulomb"]))
    return _lists[name]


def test_judge_reproduces_the_reference_vectors(golden_dir):
    g = np.load(f"{golden_dir}/pme_ref.npz")
    for k in range(int(g["num_cases"])):
        c = {name[len(f"c{k}_"):]: g[name] for name in g.files if name.startswith(f"c{k}_")}
        excl = f64.sorted_excl(c["exclusions"]).reshape(len(c["positions"]), -1)
        j = ref.judge(c["positions"], c["charges"], c["neighbors"], c["deltas"], c["distances"], excl, c["alpha"], c["coulomb"])
        assert abs(j["energy"] - float(c["energy"])) <= 1e-5 * max(abs(float(c["energy"])), 1.0), k
        assert np.abs(j["pos_deriv"] - c["pos_grad"]).max() <= 1e-4 * np.abs(c["pos_grad"]).max(), k
        assert np.abs(j["charge_deriv"] - c["charge_grad"]).max() <= 1e-4 * np.abs(c["charge_grad"]).max(), k


def test_judge_reproduces_the_oracle_on_a_salt_box():
    """1 000 atoms at 0.05 / A^3, cutoff 9 A, two exclusions per atom at most: the project's bars."""
    rng = np.random.default_rng(3)
    n, per_side, spacing = 1000, 10, (1 / 0.05) ** (1.0 / 3.0)
    pos = ref._jittered_lattice(n, per_side, spacing, 0.8, rng).astype(np.float32)
    box = (np.eye(3) * per_side * spacing).astype(np.float32)
    q = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)).astype(np.float32)
    excl = np.full((n, 2), -1, np.int64)
    order = rng.permutation(n)
    for a, b in zip(order[0::2], order[1::2]):
        excl[a, 0], excl[b, 0] = b, a
    for a, b in zip(order[1:301:2], order[2:302:2]):
        excl[a, 1], excl[b, 1] = b, a
    excl = f64.sorted_excl(excl)
    nb, dl, ds, found = ref.host_pair_list(pos, 9.0, 100000, box)
    assert 50000 < found < 100000
    e, pd, cd = pme_direct_oracle(pos, q, nb, dl, ds, excl, 0.35, ref.COULOMB)
    j = ref.judge(pos, q, nb, dl, ds, excl, 0.35, ref.COULOMB)
    assert abs(j["energy"] - e) <= ref.ENERGY_BAR * j["energy_mag"]
    assert np.abs(j["pos_deriv"] - pd).max() <= ref.DERIV_BAR * np.abs(pd).max()
    assert np.abs(j["charge_deriv"] - cd).max() <= ref.DERIV_BAR * np.abs(cd).max()
    # the magnitudes bound the sums they belong to
    assert (np.abs(j["pos_deriv"]) <= j["pos_mag"] * (1 + 1e-12)).all() and (np.abs(j["charge_deriv"]) <= j["charge_mag"] * (1 + 1e-12)).all()
    assert abs(j["energy"]) <= j["energy_mag"]


@pytest.mark.parametrize("name", ["excl-17", "run-excluded-257-65-37", "cap-37"])
def test_analytic_derivatives_equal_autograd(name):
    """With deltas and distances formed in float64 from the positions (the listed minimum-image shift kept), the judge's
    derivatives are those of its own energy: 1e-10 of the largest component."""
    case, (nb, dl, ds), _ = _case(name)
    keep = ref.included_slots(nb, case["excl"])
    a1, a2 = torch.as_tensor(nb[0][keep].astype(np.int64)), torch.as_tensor(nb[1][keep].astype(np.int64))
    pos = torch.tensor(case["pos"].astype(np.float64), requires_grad=True)
    q = torch.tensor(case["q"].astype(np.float64), requires_grad=True)
    shift = torch.round((pos.detach()[a1] - pos.detach()[a2]) - torch.as_tensor(dl[keep].astype(np.float64)))       # whole box vectors
    if case.get("forward", {}).get("box") is not None:
        length = torch.as_tensor(np.diag(case["forward"]["box"]).astype(np.float64))
        shift = torch.round(shift / length) * length
    else:
        assert float(shift.abs().max()) == 0.0
    delta = pos[a1] - pos[a2] - shift
    r = delta.norm(dim=1)
    ex_i, ex_j = (torch.as_tensor(a) for a in ref.excluded_pairs(case["excl"]))
    energy = ref.energy_of(pos, q, a1, a2, delta, r, ex_i, ex_j, case["alpha"], case["coulomb"])
    energy.backward()
    full_dl, full_ds = np.zeros((nb.shape[1], 3)), np.ones(nb.shape[1])
    full_dl[keep], full_ds[keep] = delta.detach().numpy(), r.detach().numpy()
    j = ref.judge(case["pos"], case["q"], nb, full_dl, full_ds, case["excl"], case["alpha"], case["coulomb"])
    assert abs(j["energy"] - float(energy.detach())) <= 1e-12 * j["energy_mag"]
    assert np.abs(j["pos_deriv"] - pos.grad.numpy()).max() <= 1e-10 * np.abs(pos.grad.numpy()).max()
    assert np.abs(j["charge_deriv"] - q.grad.numpy()).max() <= 1e-10 * np.abs(q.grad.numpy()).max()


def test_inclusion_rule_is_the_reference_loop():
    """included_slots / excluded_pairs against the reference's loops written out (pmeCPU.cpp:108-111 and :136), on a table with
    a self entry and rows of every fill."""
    case, (nb, _, _), _ = _case("excl-17")
    excl = case["excl"]
    keep = ref.included_slots(nb, excl)
    for s in range(nb.shape[1]):
        a1, a2 = int(nb[0, s]), int(nb[1, s])
        include = a1 > -1
        j = 0
        while include and j < excl.shape[1] and excl[a1, j] >= a2:
            if excl[a1, j] == a2:
                include = False
            j += 1
        assert include == keep[s], s
    pairs = set()
    for a1 in range(len(excl)):
        j = 0
        while j < excl.shape[1] and excl[a1, j] > a1:
            pairs.add((a1, int(excl[a1, j])))
            j += 1
    assert pairs == set(zip(*(a.tolist() for a in ref.excluded_pairs(excl))))
    assert (case["self_atom"], case["self_atom"]) not in pairs


# ---- the inputs meet the conditions they were built for ---------------------------------------------------------------------
@pytest.mark.parametrize("k", ref.CAP_CASE_K)
def test_cap_case_conditions(k):
    case, (nb, dl, ds), j = _case(f"cap-{k}")
    assert nb.shape[1] == 64 and ref.incoming_cap(64, 64) == 36
    entries = ref.delivered_entries(nb, case["excl"], 64)
    assert entries[0] == k and (entries[1:k + 1] == 1).all() and (entries[k + 1:] == 0).all()
    assert list(ref.spilling_atoms(nb, case["excl"], 64)) == ([0] if k > 36 else [])
    assert (nb[:, k:] == -1).all() and np.isnan(ds[k:]).all()
    assert 2.0 <= ds[:k].min() and ds[:k].max() <= 3.0 and (dl[:k, 0] > 0).all() and (case["q"] > 0).all()
    # atom 0's x component is the largest of the system, and every single entry is at least 10 x the derivative bar
    top = np.abs(j["pos_deriv"]).max()
    assert abs(j["pos_deriv"][0, 0]) == top
    r, d = ds[:k].astype(np.float64), dl[:k].astype(np.float64)
    a = case["alpha"] * r
    dedr = case["coulomb"] * case["q"][1:k + 1] * case["q"][0] * (np.vectorize(math.erfc)(a) + ref.TWO_OVER_SQRT_PI * a * np.exp(-a * a)) / r ** 3
    assert (np.abs(dedr * d[:, 0]) >= 10 * ref.DERIV_BAR * top).all()
    charge_entries = case["coulomb"] * np.vectorize(math.erfc)(a) / r * case["q"][1:k + 1]
    assert (charge_entries >= 10 * ref.DERIV_BAR * np.abs(j["charge_deriv"]).max()).all()


def test_cluster_case_conditions():
    case, (nb, dl, ds), j = _case("cluster")
    n, cluster = len(case["pos"]), case["cluster"]
    assert n == 6000 and len(cluster) == 200 and ref.incoming_cap(ref.CLUSTER_SLOTS, n) == 48
    found = int((nb[0] > -1).sum())
    assert found == 200 * 199 // 2 <= ref.CLUSTER_SLOTS                      # every cluster pair and no other
    assert np.isin(nb[:, :found], cluster).all() and ds[:found].max() < ref.CLUSTER_CUTOFF
    assert ref.min_distance(case["pos"][cluster]) >= 0.8
    entries = ref.delivered_entries(nb, case["excl"], n)
    assert entries[cluster[0]] == 199 and (entries[np.setdiff1d(np.arange(n), cluster)] == 0).all()
    spilling = ref.spilling_atoms(nb, case["excl"], n)
    assert len(spilling) > 100 and np.isin(spilling, cluster).all()
    assert (j["pos_mag"][np.setdiff1d(np.arange(n), cluster)] == 0).all()


def test_clamp_case_conditions():
    case, (nb, dl, ds), j = _case("clamp")
    n = len(case["pos"])
    slots = n * (n - 1) // 2
    assert n == 2100 and nb.shape[1] == slots and (nb[0] > -1).all()          # the cutoff spans the cube: all pairs
    assert ref.incoming_cap(slots, n) == 2048 and 4 * ((slots + n - 1) // n) + 32 > 2048
    assert 2 * 4096 * 256 < slots <= 3 * 4096 * 256                           # three strides of the slot kernels
    entries = ref.delivered_entries(nb, case["excl"], n)
    assert entries[0] == n - 1
    spilling = ref.spilling_atoms(nb, case["excl"], n)                         # n - 1 - i entries as second atom + the runs as first
    assert n - 1 - 2048 <= len(spilling) < 64 and list(spilling) == list(range(len(spilling)))
    assert ref.min_distance(case["pos"]) >= 1.7
    # the farthest pairs still contribute more than the bar: the smallest single pair force against the largest component
    r = ds.astype(np.float64)
    a = case["alpha"] * r
    erfc = torch.special.erfc(torch.as_tensor(a)).numpy()
    force = case["coulomb"] * np.abs(case["q"][nb[0]] * case["q"][nb[1]]) * (erfc + ref.TWO_OVER_SQRT_PI * a * np.exp(-a * a)) / r ** 2
    assert force.min() > ref.DERIV_BAR * np.abs(j["pos_deriv"]).max()
    # ... and a stride left out is far above it
    third = slice(2 * 4096 * 256, slots)
    lost = np.zeros((n, 3))
    np.add.at(lost, nb[0][third], (force[third] / r[third])[:, None] * dl[third])
    assert np.abs(lost).max() > 100 * ref.DERIV_BAR * np.abs(j["pos_deriv"]).max()


def test_many_case_conditions():
    case, (nb, dl, ds), j = _case("many")
    n = len(case["pos"])
    assert n == 65536 + 21 and n > 4096 * 16 and n % 16 != 0
    box = case["forward"]["box"]
    assert abs(n / float(np.prod(np.diag(box))) - 0.01) < 0.001 and ref.min_distance(case["pos"], box) >= 1.5
    found = int((nb[0] > -1).sum())
    assert 100000 < found < case["forward"]["slots"]
    assert len(ref.spilling_atoms(nb, case["excl"], n)) == 0
    assert ((case["excl"] > -1).sum(1) == 1)[1:].all() and case["excl"][0, 0] == -1
    tail = slice(65536, n)
    assert (np.abs(j["pos_deriv"][tail]) > 0).all() and (np.abs(j["charge_deriv"][tail]) > 0).all()
    assert np.isin(np.arange(65536, n), nb[:, :found]).sum() >= 15            # most of them have listed pairs, all an excluded one
    assert ref.wrapped_slots(case["pos"], nb, dl).sum() > 100


@pytest.mark.parametrize("variant", ref.RUN_VARIANTS)
def test_run_case_conditions(variant):
    shapes = ref.run_shapes()
    assert {t for t, _, _ in shapes} == set(ref.RUN_TOTALS) and {l for _, l, _ in shapes} == set(ref.RUN_LENGTHS)
    assert any(f % 64 == 37 for _, _, f in shapes) and any(f < 256 < f + l for _, l, f in shapes)
    for total, length, first in shapes:
        case, (nb, dl, ds), _ = _case(f"run-{variant}-{total}-{length}-{first}")
        assert nb.shape[1] == total
        owned = nb[0] == ref.RUN_HUB
        if variant == "shuffled":
            assert owned.sum() == length
            continue
        run = slice(first, first + length)
        assert owned[run].sum() == owned.sum() and owned[first] and owned[first + length - 1]
        assert len(set(nb[1][run][owned[run]].tolist())) == owned.sum()
        keep = ref.included_slots(nb, case["excl"])
        if variant == "plain":
            assert owned[run].all() and keep.all()
        if variant == "excluded":
            assert owned[run].all() and (~keep).sum() == 1 and not keep[first + length // 2]
        if variant == "holes":
            assert total < 8 or ((nb[0] == -1).any() and (nb[0] == -1).sum() == (nb[1] == -1).sum() == np.isnan(ds).sum())
            assert length < 63 or (nb[0][run] == -1).any()


@pytest.mark.parametrize("max_excl", ref.EXCLUSION_WIDTHS)
def test_exclusion_case_conditions(max_excl):
    case, (nb, dl, ds), _ = _case(f"excl-{max_excl}")
    excl, pos, box = case["excl"], case["pos"], case["forward"]["box"]
    n = len(pos)
    assert excl.shape == (n, max_excl) and float(box[0, 0]) >= 2 * ref.EXCLUSION_CUTOFF
    assert (np.diff(excl, axis=1) <= 0).all()                                 # sorted descending, -1 behind
    member = {(i, int(j)) for i in range(n) for j in excl[i] if j >= 0}
    assert all((j, i) in member for i, j in member)                           # symmetric
    fill = (excl > -1).sum(1)
    assert set(fill.tolist()) == set(range(max_excl + 1))                     # padding starts at every column
    assert {int(f) % 16 for f in fill} == set(range(min(16, max_excl + 1)))
    assert (case["self_atom"], case["self_atom"]) in member
    listed = {(int(a), int(b)) for a, b in zip(nb[0], nb[1]) if a > -1}
    wrapped = ref.wrapped_slots(pos, nb, dl)
    listed_wrapped = {(int(a), int(b)) for a, b in zip(nb[0][wrapped], nb[1][wrapped])}
    pairs = {(i, j) for i, j in member if i > j}
    assert len(pairs & listed) - len(pairs & listed_wrapped) >= 3             # excluded and in the list
    assert len(pairs & listed_wrapped) >= 3                                   # ... with a wrapped delta
    assert len(pairs - listed) >= 3                                           # excluded and beyond the cutoff
    assert (~ref.included_slots(nb, excl)).sum() - (nb[0] == -1).sum() == len(pairs & listed)
    assert len(ref.spilling_atoms(nb, excl, n)) == 0


@pytest.mark.parametrize("slots", ref.EMPTY_SLOTS)
def test_empty_case_conditions(slots):
    case, (nb, dl, ds), j = _case(f"empty-{slots}")
    assert nb.shape == (2, slots) and (nb == -1).all()
    assert (case["excl"][case["lonely"]] == -1).all() and (case["excl"][:20] > -1).any(1).all()
    assert (j["pos_mag"][case["lonely"]] == 0).all() and (j["charge_mag"][case["lonely"]] == 0).all()
    assert (j["pos_mag"][:20] > 0).all() and j["energy_mag"] > 0


# ---- the per-atom bar ----------------------------------------------------------------------------------------------------------
def test_per_atom_bar_is_the_measured_one():
    """The float32-term, float64-sum oracle against the judge over every input of the edge tests: the largest ratio
    (|oracle - judge| - one float32 ulp of the result) / (2^-23 sum_k |term_k|), times 4, rounded up to a power of two, is
    PER_ATOM_C.  The oracle also stays inside the project's bars on every input."""
    worst = 0.0
    for name, _ in ref.all_cases():
        case, (nb, dl, ds), j = _case(name)
        e, pd, cd = pme_direct_oracle(case["pos"], case["q"], nb, dl, ds, case["excl"], case["alpha"], case["coulomb"])
        assert abs(e - j["energy"]) <= ref.ENERGY_BAR * j["energy_mag"], name
        assert np.abs(pd - j["pos_deriv"]).max() <= ref.DERIV_BAR * np.abs(j["pos_deriv"]).max(), name
        assert np.abs(cd - j["charge_deriv"]).max() <= ref.DERIV_BAR * np.abs(j["charge_deriv"]).max(), name
        assert (pd[j["pos_mag"] == 0] == 0).all() and (cd[j["charge_mag"] == 0] == 0).all(), name
        ratio = max(ref.per_atom_ratio(pd, j["pos_deriv"], j["pos_mag"]), ref.per_atom_ratio(cd, j["charge_deriv"], j["charge_mag"]))
        worst = max(worst, ratio)
    print(f"largest per-atom ratio of the float32 oracle: {worst:.3f}")
    assert 2.0 ** math.ceil(math.log2(4 * worst)) == ref.PER_ATOM_C, worst
