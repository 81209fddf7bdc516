"""Float64 judge and input builders of test_pme_direct_edges_gpu.py / test_pme_direct_reference_cpu.py (no GPU code).

* ``judge``: direct-space PME on a pair list in float64 (torch on the host): the inclusion rule of the reference
  (pmeCPU.cpp:105-112, as oracle/pme_oracle.py restates it) on the list AS DATA -- neighbors, deltas, distances exactly as the
  kernels read them, promoted to float64 -- and the excluded pairs un-wrapped from the positions, once per pair
  (pmeCPU.cpp:135-157).  Besides the energy and its derivatives it returns, per atom and component, the sum of the MAGNITUDES of
  the contributions: the scale a float32 summation error is measured against.
* ``incoming_cap`` / ``delivered_entries``: what the delivering path of pme.hip does with a list -- the length of an atom's
  incoming row and the number of entries the atom receives (one per included pair it is second in, one per run of
  consecutive included slots it is first in, runs cut at multiples of 64 slots) -- so that a test knows which atoms spill.
* the inputs of the edge tests, each built in float64 and cast to float32 ONCE, with the conditions they were built to meet
  asserted by test_pme_direct_reference_cpu.py.  Hand-made lists come as data; lists the forward op of getNeighborPairs is to
  make come as (cutoff, slots, box), with ``host_pair_list`` as its host-side stand-in (the reference's order and float32 arithmetic).
"""
import math

import numpy as np
import torch

COULOMB = 332.063713
EPS32 = 2.0 ** -23
ENERGY_BAR = 1e-5                # of the sum of |pair energies|     (test_pme_gpu.py)
DERIV_BAR = 1e-4                 # of the largest component          (test_pme_gpu.py)
PATHS_BAR = 2e-6                 # delivering against indexed        (test_pme_gpu.py)
# per atom and component: |got - ref| <= PER_ATOM_C * 2^-23 * sum_k |term_k| + one float32 ulp of the result.
# MEASURED (test_pme_direct_reference_cpu.py::test_per_atom_bar_is_the_measured_one): the largest ratio the float32-term oracle
# reaches against the judge over every input below, times 4 (device erfcf / expf are other few-ulp implementations than the
# host's), rounded up to a power of two.  Measured ratio: 3.78.
PER_ATOM_C = 16.0
TWO_OVER_SQRT_PI = 2.0 / math.sqrt(math.pi)


# ---------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------
def included_slots(neighbors, exclusions):
    """bool [slots]: the reference's rule -- the first atom is not -1 and the second is not met in the first's exclusion row
    before an entry below it (rows sorted descending)."""
    nb = np.asarray(neighbors, np.int64)
    ex = np.asarray(exclusions, np.int64)
    a1, a2 = nb[0], nb[1]
    keep = a1 > -1
    if ex.ndim == 2 and ex.shape[1] and keep.any():
        rows = ex[np.maximum(a1, 0)]
        walking = np.cumprod(rows >= a2[:, None], axis=1).astype(bool)          # the loop is still running at column j
        keep &= ~((rows == a2[:, None]) & walking).any(1)
    return keep


def excluded_pairs(exclusions):
    """(i, j) with j > i, once per pair: row i walked while its entries are above i (pmeCPU.cpp:136)."""
    ex = np.asarray(exclusions, np.int64)
    if ex.ndim != 2 or ex.shape[1] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    own = np.arange(len(ex))[:, None]
    walking = np.cumprod(ex > own, axis=1).astype(bool)
    i, col = np.nonzero(walking)
    return i.astype(np.int64), ex[i, col]


def _pair_energies(q, a1, a2, r, alpha, coulomb):
    return coulomb * q[a1] * q[a2] * torch.special.erfc(alpha * r) / r


def _excluded_energies(pos, q, i, j, alpha, coulomb):
    r = (pos[i] - pos[j]).norm(dim=1)
    return -coulomb * q[i] * q[j] * torch.special.erf(alpha * r) / r


def energy_of(pos, q, a1, a2, delta, r, ex_i, ex_j, alpha, coulomb):
    """The judge's energy as a function of float64 tensors (differentiable: the autograd check of the analytic derivatives)."""
    return _pair_energies(q, a1, a2, r, alpha, coulomb).sum() + _excluded_energies(pos, q, ex_i, ex_j, alpha, coulomb).sum()


def judge(positions, charges, neighbors, deltas, distances, exclusions, alpha, coulomb):
    """-> dict of float64 numpy: energy, pos_deriv [N,3], charge_deriv [N], pos_mag [N,3], charge_mag [N] (sums of |term|),
    energy_mag (sum of |pair energies|, excluded pairs included)."""
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    pos, q = t64(positions), t64(charges)
    n = len(pos)
    keep = included_slots(neighbors, exclusions)
    nb = np.asarray(neighbors, np.int64)
    a1, a2 = torch.as_tensor(nb[0][keep]), torch.as_tensor(nb[1][keep])
    delta, r = t64(np.asarray(deltas)[keep]).reshape(-1, 3), t64(np.asarray(distances)[keep])
    ex_i, ex_j = (torch.as_tensor(a) for a in excluded_pairs(exclusions))
    alpha, coulomb = float(alpha), float(coulomb)

    pd, cd = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pm, cm = torch.zeros(n, 3, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    # listed pairs: E = k q1 q2 erfc(a r) / r
    ar = alpha * r
    erfc = torch.special.erfc(ar)
    e_pair = coulomb * q[a1] * q[a2] * erfc / r
    dedr = coulomb * q[a1] * q[a2] * (erfc + TWO_OVER_SQRT_PI * ar * torch.exp(-ar * ar)) / r ** 3
    f = dedr[:, None] * delta                                                   # dE/dx of the SECOND atom
    pd.index_add_(0, a1, -f); pd.index_add_(0, a2, f)
    pm.index_add_(0, a1, f.abs()); pm.index_add_(0, a2, f.abs())
    c1, c2 = coulomb * erfc / r * q[a2], coulomb * erfc / r * q[a1]
    cd.index_add_(0, a1, c1); cd.index_add_(0, a2, c2)
    cm.index_add_(0, a1, c1.abs()); cm.index_add_(0, a2, c2.abs())
    # excluded pairs, un-wrapped: E = -k q1 q2 erf(a r) / r
    dr = pos[ex_i] - pos[ex_j]
    rr = dr.norm(dim=1)
    ar = alpha * rr
    erf = torch.special.erf(ar)
    e_excl = -coulomb * q[ex_i] * q[ex_j] * erf / rr
    dedr = coulomb * q[ex_i] * q[ex_j] * (erf - TWO_OVER_SQRT_PI * ar * torch.exp(-ar * ar)) / rr ** 3
    g = dedr[:, None] * dr                                                      # dE/dx of atom i
    pd.index_add_(0, ex_i, g); pd.index_add_(0, ex_j, -g)
    pm.index_add_(0, ex_i, g.abs()); pm.index_add_(0, ex_j, g.abs())
    c1, c2 = -coulomb * erf / rr * q[ex_j], -coulomb * erf / rr * q[ex_i]
    cd.index_add_(0, ex_i, c1); cd.index_add_(0, ex_j, c2)
    cm.index_add_(0, ex_i, c1.abs()); cm.index_add_(0, ex_j, c2.abs())
    return {"energy": float(e_pair.sum() + e_excl.sum()), "energy_mag": float(e_pair.abs().sum() + e_excl.abs().sum()),
            "pos_deriv": pd.numpy(), "charge_deriv": cd.numpy(), "pos_mag": pm.numpy(), "charge_mag": cm.numpy()}


def ulp32(x):
    """One float32 ulp at |x| (float64 array)."""
    x32 = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(x32, np.float32(np.inf)) - x32).astype(np.float64)


def per_atom_ratio(got, ref, mag):
    """max over atoms and components of (|got - ref| - one float32 ulp of the result) / (2^-23 * sum |term|); 0 where nothing
    contributes (there `got` must be exactly 0: the caller asserts that)."""
    got, ref, mag = (np.asarray(a, np.float64) for a in (got, ref, mag))
    excess = np.maximum(np.abs(got - ref) - ulp32(ref), 0.0)
    live = mag > 0
    return float((excess[live] / (EPS32 * mag[live])).max()) if live.any() else 0.0


# ---------------------------------------------------------------------------------------------
# what the delivering path does with a list
# ---------------------------------------------------------------------------------------------
def incoming_cap(slots, atoms):
    """Entries an atom's incoming row holds (pme.hip: incoming_capacity)."""
    return min(4 * ((slots + atoms - 1) // max(atoms, 1)) + 32, 2048)


def delivered_entries(neighbors, exclusions, atoms):
    """int64 [atoms]: entries the delivering path hands each atom -- one per included pair it is second in, one per run of
    consecutive included slots with it as first atom (a run ends at every multiple of 64 slots: one wave)."""
    nb = np.asarray(neighbors, np.int64)
    keep = included_slots(nb, exclusions)
    slots = nb.shape[1]
    entries = np.bincount(nb[1][keep], minlength=atoms).astype(np.int64)
    if slots:
        idx = np.arange(slots)
        last = np.ones(slots, bool)                                             # last slot of its run?
        last[:-1] = (idx[:-1] % 64 == 63) | ~keep[1:] | (nb[0][1:] != nb[0][:-1])
        entries += np.bincount(nb[0][keep & last], minlength=atoms)
    return entries


def spilling_atoms(neighbors, exclusions, atoms):
    return np.nonzero(delivered_entries(neighbors, exclusions, atoms) > incoming_cap(np.asarray(neighbors).shape[1], atoms))[0]


# ---------------------------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------------------------
def list_from_pairs(pos, first, second, slots=None, box=None):
    """The list as data for given (first, second) atoms: float32 deltas = pos[first] - pos[second] (minimum image of an
    orthorhombic box where one is given), float32 distances; padded with (-1, NaN, NaN) up to `slots`."""
    pos = np.asarray(pos, np.float32)
    first, second = np.asarray(first, np.int64), np.asarray(second, np.int64)
    d = pos[first] - pos[second]
    if box is not None:
        box = np.asarray(box, np.float32)
        for axis in (2, 1, 0):
            d = d - np.outer(np.round(d[:, axis] / box[axis, axis]), box[axis]).astype(np.float32)
    r = np.sqrt((d * d).sum(1, dtype=np.float32)).astype(np.float32)
    slots = len(first) if slots is None else slots
    nb = np.full((2, slots), -1, np.int32)
    dl = np.full((slots, 3), np.nan, np.float32)
    ds = np.full(slots, np.nan, np.float32)
    nb[0, :len(first)], nb[1, :len(first)], dl[:len(first)], ds[:len(first)] = first, second, d, r
    return nb, dl, ds


def host_pair_list(pos, cutoff, slots, box=None):
    """Host-side stand-in for the forward op of getNeighborPairs with max_num_pairs = slots: every pair within the cutoff as
    (row, col < row), in the order of the lower triangle, compacted and padded.  -> (neighbors, deltas, distances, found)."""
    from scipy.spatial import cKDTree
    pos = np.asarray(pos, np.float32)
    n = len(pos)
    if n * (n - 1) // 2 <= 3_000_000:
        rows, cols = np.tril_indices(n, -1)
    else:
        p64 = pos.astype(np.float64)
        length = None if box is None else np.diag(np.asarray(box, np.float64))
        tree = cKDTree(p64 if box is None else np.mod(p64, length), boxsize=length)
        pairs = tree.query_pairs(cutoff * (1 + 1e-5), output_type="ndarray")
        rows, cols = pairs.max(1), pairs.min(1)
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
    nb, dl, ds = list_from_pairs(pos, rows, cols, box=box)
    keep = ds <= np.float32(cutoff)
    found = int(keep.sum())
    assert found <= slots, (found, slots)
    out = list_from_pairs(pos, rows[keep], cols[keep], slots=slots, box=box)
    return (*out, found)


# ---------------------------------------------------------------------------------------------
# inputs.  Every builder returns a dict: pos, q (float32), excl (int64 [N, max_excl], rows sorted descending, -1 padded),
# alpha, coulomb, and either "list" = (neighbors, deltas, distances) or "forward" = dict(cutoff, slots, box).
# ---------------------------------------------------------------------------------------------
def _sorted_rows(excl):
    return -np.sort(-np.asarray(excl, np.int64), axis=1)


def _no_exclusions(n):
    return np.zeros((n, 0), np.int64)


def _jittered_lattice(count, per_side, spacing, jitter, rng):
    """`count` of the per_side^3 sites of a cubic lattice, each moved by up to `jitter` along every axis (float64)."""
    sites = np.stack(np.meshgrid(*[np.arange(per_side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pick = rng.permutation(len(sites))[:count]
    return (sites[pick] + 0.5) * spacing + rng.uniform(-jitter, jitter, (count, 3))


def min_distance(pos, box=None):
    from scipy.spatial import cKDTree
    p = np.asarray(pos, np.float64)
    length = None if box is None else np.diag(np.asarray(box, np.float64))
    tree = cKDTree(p if box is None else np.mod(p, length), boxsize=length)
    return float(tree.query(tree.data, k=2)[0][:, 1].min())


CAP_CASE_K = (35, 36, 37, 63)


def cap_case(k):
    """64 atoms, 64 slots (cap 36): pairs (j, 0) for j = 1..k.  The partners sit on the +x side of atom 0 at 2 to 3 A, all
    charges positive: atom 0's x component is the largest of the system and every single entry is a visible part of it."""
    rng = np.random.default_rng(100 + k)
    n = 64
    pos = np.zeros((n, 3))
    radius = rng.uniform(2.0, 3.0, n - 1)
    polar, azimuth = rng.uniform(0, math.pi / 4, n - 1), rng.uniform(0, 2 * math.pi, n - 1)
    pos[1:] = radius[:, None] * np.stack([np.cos(polar), np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth)], 1)
    pos[k + 1:, 0] += 50.0 + 5.0 * np.arange(n - 1 - k)                           # atoms without a pair: far away
    pos = pos.astype(np.float32)
    q = rng.uniform(0.5, 1.0, n).astype(np.float32)
    return {"pos": pos, "q": q, "excl": _no_exclusions(n), "alpha": 0.3, "coulomb": COULOMB,
            "list": list_from_pairs(pos, np.arange(1, k + 1), np.zeros(k, np.int64), slots=64)}


CLUSTER_ATOMS, CLUSTER_CUTOFF, CLUSTER_SLOTS = 200, 10.0, 20000


def cluster_case():
    """6 000 atoms: 200 inside a ball of 9.8 A diameter (every one within the 10 A cutoff of every other, 0.8 A apart at least)
    at indices scattered over the whole range, among 5 800 atoms 16 A apart that meet nobody.  20 000 slots: cap 48."""
    rng = np.random.default_rng(7)
    n, spacing = 6000, 16.0
    sites = np.stack(np.meshgrid(*[np.arange(18)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centre = np.array([9, 9, 9])
    others = sites[(sites != centre).any(1)]
    dilute = others[rng.permutation(len(others))[:n - CLUSTER_ATOMS]] * spacing + rng.uniform(-0.5, 0.5, (n - CLUSTER_ATOMS, 3))
    fine = np.stack(np.meshgrid(*[np.arange(-5, 6)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    fine = fine[np.linalg.norm(fine, axis=1) <= 4.6]                             # 1 A lattice in a ball; + jitter: radius < 4.9
    cluster = centre * spacing + fine[rng.permutation(len(fine))[:CLUSTER_ATOMS]] + rng.uniform(-0.09, 0.09, (CLUSTER_ATOMS, 3))
    where = rng.permutation(n)
    pos = np.empty((n, 3))
    pos[where[:CLUSTER_ATOMS]], pos[where[CLUSTER_ATOMS:]] = cluster, dilute
    q = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)).astype(np.float32)
    return {"pos": pos.astype(np.float32), "q": q, "excl": _no_exclusions(n), "alpha": 0.3, "coulomb": COULOMB,
            "cluster": np.sort(where[:CLUSTER_ATOMS]), "forward": {"cutoff": CLUSTER_CUTOFF, "slots": CLUSTER_SLOTS, "box": None}}


def clamp_case():
    """2 100 atoms in vacuum at liquid density (a 28 A cube), cutoff beyond its diagonal: the compacted list holds all
    n (n - 1) / 2 = 2 203 950 pairs -- cap clamps at 2 048 and atoms 0..50 receive more; the slot kernels take three strides
    (4 096 blocks of 256).  alpha = 0.01 / A keeps erfc at the far corner near one half."""
    rng = np.random.default_rng(21)
    n = 2100
    pos = _jittered_lattice(n, 13, 2.15, 0.2, rng).astype(np.float32)
    q = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.7, 1.0, n)).astype(np.float32)
    return {"pos": pos, "q": q, "excl": _no_exclusions(n), "alpha": 0.01, "coulomb": COULOMB,
            "forward": {"cutoff": 60.0, "slots": n * (n - 1) // 2, "box": None}}


MANY_ATOMS = 65536 + 21


def many_case():
    """65 557 atoms (the atom kernels' 4 096 blocks serve 65 536; the last group of 16 lanes holds 5) in a periodic box at
    0.0095 / A^3, cutoff 5 A, one exclusion per atom: (1, 2), (3, 4), ... wherever the partners happen to be.  alpha = 0.2 / A:
    alpha r <= 1 (see run_case)."""
    rng = np.random.default_rng(33)
    n, per_side, spacing = MANY_ATOMS, 41, 100.0 ** (1.0 / 3.0)
    pos = _jittered_lattice(n, per_side, spacing, 1.5, rng).astype(np.float32)
    box = (np.eye(3) * per_side * spacing).astype(np.float32)
    q = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)).astype(np.float32)
    excl = np.full((n, 1), -1, np.int64)
    odd = np.arange(1, n - 1, 2)
    excl[odd, 0], excl[odd + 1, 0] = odd + 1, odd
    return {"pos": pos, "q": q, "excl": excl, "alpha": 0.2, "coulomb": COULOMB,
            "forward": {"cutoff": 5.0, "slots": 200000, "box": box}}


RUN_TOTALS, RUN_LENGTHS, RUN_STARTS = (1, 255, 256, 257), (1, 63, 64, 65, 128, 129), (0, 37, "tail")
RUN_VARIANTS = ("plain", "excluded", "holes", "shuffled")
RUN_ATOMS, RUN_HUB = 300, 200


def run_shapes():
    """(total slots, run length, first slot of the run): the run starts at lane 0, at lane 37, or ends with the list ("tail":
    over the workgroup boundary of the 257-slot list, into the ragged last wave of the 255-slot one)."""
    shapes = []
    for total in RUN_TOTALS:
        for length in RUN_LENGTHS:
            for start in RUN_STARTS:
                first = total - length if start == "tail" else start
                if first >= 0 and first + length <= total and (total, length, first) not in shapes:
                    shapes.append((total, length, first))
    return shapes


def run_case(total, length, first, variant):
    """A hand-made list of `total` slots in which atom 200 owns the `length` consecutive slots from `first` on (partners: distinct
    lower atoms); the other slots are short runs (1 to 5 slots) of other first atoms.  Variants: "excluded" -- the middle slot of
    the run is an excluded pair; "holes" -- a quarter of the slots are (-1, NaN, NaN), inside the run as well, as in a
    max_num_pairs == -1 list; "shuffled" -- the slots in random order.
    The atoms sit 1.2 A apart in an 8.4 A cube and alpha is 0.15 / A, so alpha r stays below about 2: a float32 alpha r costs
    erfc(alpha r) a relative error of 2 (alpha r)^2 roundings, and an atom with one far pair would carry nothing else.  The
    excluded pair is the run's farthest for the other end: erf(x) - 2 x exp(-x^2) / sqrt(pi) cancels as x goes to 0."""
    rng = np.random.default_rng(1000 * total + 10 * length + first + 7 * RUN_VARIANTS.index(variant))
    n = RUN_ATOMS
    pos = _jittered_lattice(n, 7, 1.2, 0.1, rng).astype(np.float32)
    q = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)).astype(np.float32)
    a1, a2 = np.empty(total, np.int64), np.empty(total, np.int64)
    partners = rng.permutation(RUN_HUB)[:length]
    far = int(np.argmax(np.linalg.norm(pos[partners] - pos[RUN_HUB], axis=1)))
    partners[[length // 2, far]] = partners[[far, length // 2]]                   # (the middle slot: the farthest partner, see above)
    a1[first:first + length], a2[first:first + length] = RUN_HUB, partners
    previous = -1
    for lo, hi in ((0, first), (first + length, total)):
        at = lo
        while at < hi:
            run = min(int(rng.integers(1, 6)), hi - at)
            owner = int(rng.choice([a for a in range(run, n) if a not in (RUN_HUB, previous)]))
            a1[at:at + run], a2[at:at + run] = owner, rng.permutation(owner)[:run]
            previous, at = owner, at + run
        previous = RUN_HUB
    excl = _no_exclusions(n)
    if variant == "excluded":
        excl = np.full((n, 1), -1, np.int64)
        mid = first + length // 2
        excl[a1[mid], 0], excl[a2[mid], 0] = a2[mid], a1[mid]
    nb, dl, ds = list_from_pairs(pos, a1, a2)
    if variant == "holes":
        holes = rng.random(total) < 0.25
        holes[[first, first + length - 1]] = False                            # (the run keeps its ends)
        nb[:, holes], dl[holes], ds[holes] = -1, np.nan, np.nan
    if variant == "shuffled":
        order = rng.permutation(total)
        nb, dl, ds = np.ascontiguousarray(nb[:, order]), dl[order], ds[order]
    return {"pos": pos, "q": q, "excl": excl, "alpha": 0.15, "coulomb": COULOMB, "list": (nb, dl, ds)}


EXCLUSION_WIDTHS = (1, 16, 17, 33)
EXCLUSION_ATOMS, EXCLUSION_CUTOFF = 300, 6.0


def wrapped_slots(pos, nb, dl):
    """bool [slots]: the listed delta is not pos[first] - pos[second] (a box vector was taken off)."""
    pos = np.asarray(pos, np.float64)
    used = nb[0] > -1
    plain = pos[np.maximum(nb[0], 0)] - pos[np.maximum(nb[1], 0)]
    return used & (np.abs(plain - dl).max(1) > 1.0)


def exclusion_case(max_excl):
    """300 atoms in a periodic cube of 18.2 A (cutoff 6 A), a symmetric exclusion table of width max_excl with rows sorted
    descending whose fill runs from 0 to full.  Planted: four excluded pairs within the cutoff directly, four within it only across
    the box (their listed delta is wrapped, the erf() term is not), four beyond it; atom 150's row holds atom 150 itself, which
    the reference's loops pass over (pmeCPU.cpp:109 keeps walking, :136 stops: nothing below it is above the atom)."""
    rng = np.random.default_rng(500 + max_excl)
    n = EXCLUSION_ATOMS
    per_side, spacing = 7, (1 / 0.05) ** (1.0 / 3.0)
    pos = _jittered_lattice(n, per_side, spacing, 0.6, rng).astype(np.float32)
    box = (np.eye(3) * per_side * spacing).astype(np.float32)
    q = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)).astype(np.float32)
    target = rng.permutation(np.arange(n) % (max_excl + 1))                       # wanted row fills: every value 0..max_excl
    rows = [set() for _ in range(n)]
    self_atom = 150
    target[self_atom] = max(target[self_atom], 1)
    rows[self_atom].add(self_atom)

    def link(i, j):
        if i != j and j not in rows[i] and len(rows[i]) < target[i] and len(rows[j]) < target[j]:
            rows[i].add(j); rows[j].add(i)
            return True
        return False

    nb, dl, ds, _ = host_pair_list(pos, EXCLUSION_CUTOFF, 12000, box)
    wrapped = wrapped_slots(pos, nb, dl)
    near = np.nonzero((nb[0] > -1) & ~wrapped)[0]
    far = np.nonzero(wrapped)[0]
    for slots in (near, far):
        planted = 0
        for s in rng.permutation(slots):
            planted += link(int(nb[0, s]), int(nb[1, s]))
            if planted == 4:
                break
    planted = 0
    while planted < 4:
        i, j = (int(a) for a in rng.integers(0, n, 2))
        d = pos[i].astype(np.float64) - pos[j]
        d -= np.round(d / np.diag(box)) * np.diag(box)
        if np.linalg.norm(d) > EXCLUSION_CUTOFF + 1.0:
            planted += link(i, j)
    for i in rng.permutation(n):
        for j in rng.permutation(n):
            if len(rows[i]) >= target[i]:
                break
            link(int(i), int(j))
    excl = np.full((n, max_excl), -1, np.int64)
    for i, row in enumerate(rows):
        excl[i, :len(row)] = sorted(row, reverse=True)
    return {"pos": pos, "q": q, "excl": excl, "alpha": 0.35, "coulomb": COULOMB, "self_atom": self_atom,
            "forward": {"cutoff": EXCLUSION_CUTOFF, "slots": 12000, "box": box}}


EMPTY_SLOTS = (0, 7)


def empty_case(slots):
    """40 atoms, no pair at all (a list of 0 slots, or 7 slots of -1) and a table of exclusions: atoms 0..19 in chains
    (i, i + 1), atoms 20..39 alone -- only the erf() terms remain, and the lonely atoms get exact zeros."""
    rng = np.random.default_rng(9 + slots)
    n = 40
    pos = _jittered_lattice(n, 4, 2.5, 0.5, rng).astype(np.float32)
    q = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)).astype(np.float32)
    excl = np.full((n, 2), -1, np.int64)
    for i in range(19):
        excl[i, 0] = i + 1
        excl[i + 1, 1 if i + 1 < 19 else 0] = i
    excl = _sorted_rows(excl)
    return {"pos": pos, "q": q, "excl": excl, "alpha": 0.3, "coulomb": COULOMB, "lonely": np.arange(20, n),
            "list": list_from_pairs(pos, [], [], slots=slots)}


def host_list(case):
    """The case's list on the host: the hand-made one, or the stand-in for the forward op's."""
    if "list" in case:
        return case["list"]
    f = case["forward"]
    return host_pair_list(case["pos"], f["cutoff"], f["slots"], f["box"])[:3]


def all_cases():
    """(name, builder) of every input of the edge tests."""
    out = [(f"cap-{k}", lambda k=k: cap_case(k)) for k in CAP_CASE_K]
    out += [("cluster", cluster_case), ("clamp", clamp_case), ("many", many_case)]
    out += [(f"run-{v}-{t}-{l}-{f}", lambda t=t, l=l, f=f, v=v: run_case(t, l, f, v)) for v in RUN_VARIANTS for t, l, f in run_shapes()]
    out += [(f"excl-{m}", lambda m=m: exclusion_case(m)) for m in EXCLUSION_WIDTHS]
    out += [(f"empty-{s}", lambda s=s: empty_case(s)) for s in EMPTY_SLOTS]
    return out
