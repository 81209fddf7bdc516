"""The pair list's transposed index (nnpops_amd/csrc/pairs_index.hip) and its two consumers, at every bucket size and at the limit.

nnpops_neighbor_pairs_build_index puts 2^shift atoms in a bucket, shift 6..9 by the number of atoms (<= 32 768, 65 536, 131 072,
262 144).  These tests drive the C ABI directly on
  * synthetic COMPACTED lists (rows non-decreasing, then -1 padding) whose columns follow a named policy, decoded in full and
    compared exactly with numpy, on both sides of every shift boundary, at tile edges (4 096 slots), with a last bucket of one atom,
    one atom that is the column of most of the list, and column ids outside the system;
  * buffers sized exactly as the ABI reports, each followed by a 64 KiB guard region that must come back unchanged;
  * the indexed backward (float64 reference, the fixed-point pass, bitwise repeatability) and the indexed PME direct space
    (oracle, delivering path) at shifts 7-9, and the torch op on both sides of NNPOPS_PAIRS_INDEX_MAX_ATOMS."""
import ctypes as C

import numpy as np
import pytest
import torch

from nnpops_amd import workloads
from oracle import neighbor_pairs_backward_oracle, pme_direct_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MAX_ATOMS = 262144                      # NNPOPS_PAIRS_INDEX_MAX_ATOMS
ERR_UNSUPPORTED = -3                    # NNPOPS_ERR_UNSUPPORTED
GUARD, PATTERN = 64 * 1024, 0xA5
TILE = 4096                             # slots per tile of the first level


def _bucket_shift(n):
    shift = 6
    while ((n - 1) >> shift) + 1 > 512:
        shift += 1
    return shift


class _Guarded:
    """`nbytes` of device memory starting 256-byte aligned, followed by GUARD bytes of PATTERN (the whole buffer starts as PATTERN)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + GUARD + 256,), PATTERN, dtype=torch.uint8, device=DEV)
        self.off = (-self.buf.data_ptr()) % 256

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.off)

    def view(self, dtype, count):
        size = torch.empty((), dtype=dtype).element_size()
        return self.buf[self.off:self.off + size * count].view(dtype)

    def tail_intact(self):
        return bool((self.buf[self.off + self.nbytes:self.off + self.nbytes + GUARD] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())


def _lib():
    from nnpops_amd import capi
    return capi.lib()


def _stream():
    from nnpops_amd import capi
    return capi._stream_ptr(torch.device(DEV))


def _build_index(n, nb):
    """The index of `nb` (int32 [2, slots] on the device) in guarded buffers of exactly the sizes the ABI reports."""
    from nnpops_amd import capi
    L, slots = _lib(), nb.shape[1]
    ints = int(L.nnpops_neighbor_pairs_index_ints(n, slots))
    index = _Guarded(4 * ints)
    ws = _Guarded(L.nnpops_neighbor_pairs_index_workspace_bytes(n, slots))
    code = L.nnpops_neighbor_pairs_build_index(n, slots, capi._ptr(nb) if slots else None, index.ptr, ws.ptr, _stream())
    torch.cuda.synchronize()
    return code, index, ws, ints


# ---------------------------------------------------------------------------------------------------------------------------------
# synthetic compacted lists
# ---------------------------------------------------------------------------------------------------------------------------------
POLICIES = ["uniform", "hub", "ends", "outside"]
IN_RANGE = ["uniform", "hub", "ends"]


def _compacted_list(n, slots, used, policy, seed):
    """int32 [2, slots]: `used` pairs with rows non-decreasing, then -1.  Columns by `policy`:
    uniform  every atom alike;
    hub      one atom is the column of ~90 % of the pairs (and the row of a quarter: a row run across many tiles);
    ends     only the first and the last bucket are used, the last one holding ~90 % of the list;
    outside  uniform, with ids >= n sprinkled in, at the head of every tile among them (dropped like unused slots)."""
    rng = np.random.default_rng(seed)
    hub = int(rng.integers(n))
    rows = rng.integers(0, n, used)
    if policy == "hub":
        rows = np.where(rng.random(used) < 0.25, hub, rows)
    rows = np.sort(rows)
    if policy in ("uniform", "outside"):
        cols = rng.integers(0, n, used)
    elif policy == "hub":
        cols = np.where(rng.random(used) < 0.9, hub, rng.integers(0, n, used))
    elif policy == "ends":
        shift = _bucket_shift(n)
        first_hi, last_lo = min(n, 1 << shift), ((n - 1) >> shift) << shift
        cols = np.where(rng.random(used) < 0.1, rng.integers(0, first_hi, used), rng.integers(last_lo, n, used))
    else:
        raise ValueError(policy)
    if policy == "outside" and used:
        far = rng.random(used) < 0.05
        cols = np.where(far, n + rng.integers(0, 3 * n + 1000, used), cols)
        cols[::TILE] = n
        cols[used // 2] = 2**31 - 1
    nb = np.full((2, slots), -1, np.int32)
    nb[0, :used] = rows
    nb[1, :used] = cols
    return nb


# (slots, used): empty, one pair, the tile edges, a list whose tiles behind the pairs hold nothing but -1 (one starts exactly at
# a tile), a padded list of a few tiles
SLOT_CASES = [(0, 0), (1, 1), (4095, 4095), (4096, 4096), (4097, 4097), (8193, 4096), (40000, 36000)]
# every shift, both sides of each boundary, the limit, and last buckets of one atom (65, 32 769, 65 537, 131 073)
ATOMS = [1, 2, 64, 65, 32767, 32768, 32769, 65536, 65537, 131073, 200000, 262143, 262144]
BIG = [(100000, 3000000, 2900000), (262144, 3000000, 2900000)]


def _index_cases():
    for n in ATOMS:
        for slots, used in SLOT_CASES:
            for policy in (["uniform"] if used == 0 else ["uniform", "outside"] if used == 1 else POLICIES):
                yield n, slots, used, policy
    for n, slots, used in BIG:
        for policy in POLICIES:
            yield n, slots, used, policy


INDEX_CASES = list(_index_cases())


def _check_index(n, nb, order_rows_cols):
    order, row_seg, col_seg = order_rows_cols
    rows, cols = nb[0].astype(np.int64), nb[1].astype(np.int64)
    # order[:m]: the slots of columns inside the system, stably sorted by column; everything else is dropped
    used = np.flatnonzero((cols >= 0) & (cols < n))
    m = len(used)
    assert np.array_equal(order[:m], used[np.argsort(cols[used], kind="stable")])
    # col_seg: atom i owns order[start_i : start_i + count_i] with start_i = the pairs of the atoms before it -- together with the line
    # above, exactly its slots, ascending
    counts = np.bincount(cols[used], minlength=n)
    starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
    assert np.array_equal(col_seg[:, 0], starts)
    assert np.array_equal(col_seg[:, 1] - col_seg[:, 0], counts)
    # row_seg: an atom with rows owns its contiguous run of slots, an atom without has an empty segment
    r = rows[rows >= 0]
    atoms = np.arange(n)
    has = np.bincount(r, minlength=n) > 0
    want = np.stack([np.searchsorted(r, atoms, "left"), np.searchsorted(r, atoms, "right")], 1)
    assert np.array_equal(row_seg[has], want[has])
    assert np.array_equal(row_seg[~has, 1] - row_seg[~has, 0], np.zeros(int((~has).sum()), np.int64))


def _decode(index, ints, n, slots):
    flat = index.view(torch.int32, ints).cpu().numpy().astype(np.int64)
    at = (slots + 1) & ~1
    return flat[:slots], flat[at:at + 2 * n].reshape(n, 2), flat[at + 2 * n:at + 4 * n].reshape(n, 2)


@pytest.mark.parametrize("n,slots,used,policy", INDEX_CASES, ids=[f"{n}-{s}-{u}-{p}" for n, s, u, p in INDEX_CASES])
def test_build_index_exact_and_in_bounds(n, slots, used, policy):
    """The whole index against numpy, bit for bit, in buffers of exactly nnpops_neighbor_pairs_index_ints /
    _index_workspace_bytes, whose guard regions must come back unchanged (an empty list once wrote 1.5 KiB past its workspace)."""
    nb = _compacted_list(n, slots, used, policy, seed=n * 31 + slots * 7 + POLICIES.index(policy))
    code, index, ws, ints = _build_index(n, torch.tensor(nb, device=DEV))
    assert code == 0
    assert ws.tail_intact(), "nnpops_neighbor_pairs_build_index wrote past its workspace"
    assert index.tail_intact(), "nnpops_neighbor_pairs_build_index wrote past the index"
    _check_index(n, nb, _decode(index, ints, n, slots))


def test_build_index_refuses_one_atom_more_than_the_limit():
    """262 145 atoms: NNPOPS_ERR_UNSUPPORTED, and neither the index nor the workspace is touched (nothing is launched)."""
    from nnpops_amd import capi
    n = MAX_ATOMS + 1
    nb = torch.tensor(_compacted_list(n, 5000, 4500, "uniform", seed=3), device=DEV)
    code, index, ws, _ = _build_index(n, nb)
    assert code == ERR_UNSUPPORTED
    assert index.untouched() and ws.untouched()
    with pytest.raises(capi.NNPOpsHipError) as err:
        capi.neighbor_pairs_build_index(n, nb)
    assert err.value.code == ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------------
# the indexed backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _backward_indexed_guarded(n, nb, dl, ds, gd, gs, index):
    """nnpops_neighbor_pairs_backward_indexed with its workspace and grad_positions in guarded buffers."""
    from nnpops_amd import capi
    L, slots = _lib(), ds.numel()
    dtype = 1 if ds.dtype == torch.float64 else 0
    ws = _Guarded(L.nnpops_neighbor_pairs_backward_indexed_workspace_bytes(dtype, slots))
    out = _Guarded(3 * n * ds.element_size())
    code = L.nnpops_neighbor_pairs_backward_indexed(dtype, n, slots, capi._ptr(nb), capi._ptr(dl), capi._ptr(ds), capi._ptr(gd),
                                                    capi._ptr(gs), index, out.ptr, ws.ptr, _stream())
    torch.cuda.synchronize()
    assert code == 0
    assert ws.tail_intact(), "nnpops_neighbor_pairs_backward_indexed wrote past its workspace"
    assert out.tail_intact(), "nnpops_neighbor_pairs_backward_indexed wrote past grad_positions"
    return out.view(ds.dtype, 3 * n).reshape(n, 3).clone()


def _check_backward(n, nb, dl, ds, gd, gs):
    """Indexed backward vs the gradient accumulated in float64 from the same inputs, vs the fixed-point pass, and the same bits
    with a freshly built index; every buffer at exactly the size the ABI reports."""
    from nnpops_amd import capi
    code, index, ws, _ = _build_index(n, nb)
    assert code == 0 and ws.tail_intact() and index.tail_intact()
    got = _backward_indexed_guarded(n, nb, dl, ds, gd, gs, index.ptr)
    code, fresh, _, _ = _build_index(n, nb)
    assert code == 0
    assert torch.equal(_backward_indexed_guarded(n, nb, dl, ds, gd, gs, fresh.ptr), got)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    ref = neighbor_pairs_backward_oracle(n, nb.cpu().numpy(), f64(dl), f64(ds), f64(gd), f64(gs))
    tol = 1e-5 if ds.dtype == torch.float32 else 1e-12
    # (the bar is relative to the largest gradient -- or, where a list of self pairs cancels to rounding noise, to the largest term)
    used = nb[0].cpu().numpy() >= 0
    terms = f64(gd)[used] + f64(dl)[used] / f64(ds)[used][:, None] * f64(gs)[used][:, None]
    scale = max(float(np.abs(ref).max()), float(np.abs(terms).max(initial=0.0)), np.finfo(np.float64).tiny)
    got = got.cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * scale)
    fixed = capi.neighbor_pairs_backward(n, nb, dl, ds, gd, gs).cpu().numpy()
    np.testing.assert_allclose(got, fixed, rtol=tol, atol=tol * scale)


BACKWARD_CASES = [(n, slots, used, IN_RANGE[i % len(IN_RANGE)]) for i, n in enumerate(ATOMS) for slots, used in SLOT_CASES] + \
                 [(n, slots, used, policy) for n, slots, used in BIG for policy in ("uniform", "hub")]


@pytest.mark.parametrize("n,slots,used,policy", BACKWARD_CASES, ids=[f"{n}-{s}-{u}-{p}" for n, s, u, p in BACKWARD_CASES])
def test_backward_indexed_synthetic(n, slots, used, policy):
    """On the synthetic lists (columns inside the system), both dtypes."""
    nb = _compacted_list(n, slots, used, policy, seed=n * 13 + slots)
    rng = np.random.default_rng(n + slots)
    dl = rng.standard_normal((slots, 3))
    ds = rng.uniform(0.5, 5.0, slots)
    gd = rng.standard_normal((slots, 3))
    gs = rng.standard_normal(slots)
    tnb = torch.tensor(nb, device=DEV)
    for dtype in (torch.float32, torch.float64):
        t = lambda a: torch.tensor(a, dtype=dtype, device=DEV).contiguous()
        _check_backward(n, tnb, t(dl), t(ds), t(gd), t(gs))


def _box_list(n, density, cutoff, capacity, seed, dtype):
    from nnpops_amd import capi
    pos, _, box = workloads.random_box(n, density=density, seed=seed)
    nb, dl, ds, found = capi.neighbor_pairs_forward(torch.tensor(pos, dtype=dtype, device=DEV), cutoff, capacity,
                                                    torch.tensor(box, dtype=dtype, device=DEV))
    assert 0 < int(found) <= capacity
    return nb, dl, ds, int(found)


# n, density, cutoff, capacity: a liquid at shift 7, BASELINE config 5 (shift 8, ~2.9 M pairs), a sparse box at the limit (shift 9)
FORWARD_CASES = {"liquid_40000": (40000, 0.1, 5.2, 32 * 40000), "config5_100000": (100000, 0.1, 5.2, 32 * 100000),
                 "sparse_262144": (MAX_ATOMS, 0.01, 4.0, 4 * MAX_ATOMS)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("case", list(FORWARD_CASES))
def test_backward_indexed_on_forward_lists(case, dtype):
    """On lists the forward op emitted."""
    n, density, cutoff, capacity = FORWARD_CASES[case]
    nb, dl, ds, found = _box_list(n, density, cutoff, capacity, seed=6, dtype=dtype)
    if case == "config5_100000":
        assert 2_700_000 < found < 3_100_000
    rng = np.random.default_rng(n)
    gd = torch.tensor(rng.standard_normal(tuple(dl.shape)), dtype=dtype, device=DEV)
    gs = torch.tensor(rng.standard_normal(tuple(ds.shape)), dtype=dtype, device=DEV)
    _check_backward(n, nb, dl, ds, gd, gs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the indexed PME direct space
# ---------------------------------------------------------------------------------------------------------------------------------
def _pme_indexed_guarded(pos, q, nb, dl, ds, excl, alpha, coulomb, index):
    """nnpops_pme_direct_indexed with its workspace in a guarded buffer of exactly nnpops_pme_direct_indexed_workspace_bytes."""
    from nnpops_amd import capi
    L, n, pairs, max_excl = _lib(), pos.shape[0], nb.shape[1], excl.shape[1]
    ws = _Guarded(L.nnpops_pme_direct_indexed_workspace_bytes(pairs, n))
    energy = torch.empty((1,), dtype=torch.float32, device=DEV)
    pd = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    cd = torch.empty((n,), dtype=torch.float32, device=DEV)
    code = L.nnpops_pme_direct_indexed(n, pairs, max_excl, capi._ptr(pos), capi._ptr(q), capi._ptr(nb) if pairs else None,
                                       capi._ptr(dl) if pairs else None, capi._ptr(ds) if pairs else None,
                                       capi._ptr(excl) if max_excl else None, index, float(alpha), float(coulomb), capi._ptr(energy),
                                       capi._ptr(pd), capi._ptr(cd), ws.ptr, _stream())
    torch.cuda.synchronize()
    assert code == 0
    assert ws.tail_intact(), "nnpops_pme_direct_indexed wrote past its workspace"
    return energy, pd, cd


def _incoming_capacity(slots, n):
    return min(4 * ((slots + n - 1) // n) + 32, 2048)


def _partners(nb, n):
    nb = nb.cpu().numpy()
    used = nb[0] >= 0
    return np.bincount(nb[0][used], minlength=n) + np.bincount(nb[1][used], minlength=n)


def _check_pme(pos, q, nb, dl, ds, excl, alpha, coulomb):
    """Indexed vs the delivering path (2e-6 of the largest component) and vs the oracle (energy 1e-5 of the sum of |pair energies|,
    derivatives 1e-4 of the largest component), with inputs the oracle takes as they are (it computes every term in float32, as the
    kernels do, and accumulates in float64)."""
    from nnpops_amd import capi
    n = pos.shape[0]
    code, index, ws, _ = _build_index(n, nb)
    assert code == 0 and ws.tail_intact() and index.tail_intact()
    e_i, pd_i, cd_i = _pme_indexed_guarded(pos, q, nb, dl, ds, excl, alpha, coulomb, index.ptr)
    e_d, pd_d, cd_d = capi.pme_direct(pos, q, nb, dl, ds, excl, alpha, coulomb)
    e_ref, pd_ref, cd_ref = pme_direct_oracle(pos.cpu().numpy(), q.cpu().numpy(), nb.cpu().numpy(), dl.cpu().numpy(), ds.cpu().numpy(),
                                              excl.cpu().numpy().astype(np.int64), alpha, coulomb)
    terms = float(np.abs(cd_ref * q.cpu().numpy()).sum())
    assert abs(float(e_i) - e_ref) <= 1e-5 * max(terms, abs(e_ref))
    assert abs(float(e_i) - float(e_d)) <= 1e-6 * max(terms, abs(e_ref))
    # (an atom with more partners than the delivering path's incoming row holds -- pme.hip: incoming_capacity, 2 048 at most -- gets
    #  the rest through float32 atomics there; only then is that path held to the oracle's bar instead)
    deliver = 2e-6 if _partners(nb, n).max(initial=0) <= _incoming_capacity(nb.shape[1], n) else 1e-4
    assert float((pd_i - pd_d).abs().max()) <= deliver * float(pd_d.abs().max())
    assert float((cd_i - cd_d).abs().max()) <= deliver * float(cd_d.abs().max())
    assert np.abs(pd_i.cpu().numpy() - pd_ref).max() <= 1e-4 * np.abs(pd_ref).max()
    assert np.abs(cd_i.cpu().numpy() - cd_ref).max() <= 1e-4 * np.abs(cd_ref).max()


PME_SYNTHETIC = [(n, slots, used) for n in (2, 32769, 65537, 131073, 262144) for slots, used in SLOT_CASES[1:]] + \
                [(262144, 3000000, 2900000)]


@pytest.mark.parametrize("n,slots,used", PME_SYNTHETIC, ids=[f"{n}-{s}-{u}" for n, s, u in PME_SYNTHETIC])
def test_pme_indexed_synthetic(n, slots, used):
    """On synthetic lists at every shift (columns inside the system, distances 1-8 A, no exclusions)."""
    nb = _compacted_list(n, slots, used, "uniform", seed=n + 5 * slots)
    rng = np.random.default_rng(n * 3 + slots)
    t = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device=DEV).contiguous()
    pos = t(20 * rng.random((n, 3)))
    q = t(rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n))
    dl = rng.standard_normal((slots, 3))
    ds = rng.uniform(1.0, 8.0, slots)
    _check_pme(pos, q, t(nb, torch.int32), t(dl), t(ds), torch.zeros((n, 0), dtype=torch.int32, device=DEV), 0.35, 332.063713)


def _salt_box(n, seed, max_excl):
    """tests/test_pme_gpu.py's salt box: +-0.2..1 charges at 0.05 atoms/A^3, disjoint excluded pairs (symmetric by construction)."""
    rng = np.random.default_rng(seed)
    pos, _, box = workloads.random_box(n, density=0.05, seed=seed)
    charges = rng.choice([-1.0, 1.0], size=n).astype(np.float32) * rng.uniform(0.2, 1.0, n).astype(np.float32)
    excl = -np.ones((n, max_excl), np.int64)
    fill = np.zeros(n, int)
    order = rng.permutation(n)
    for a, b in zip(order[0::2], order[1::2]):
        for i, j in ((a, b), (b, a)):
            if fill[i] < max_excl:
                excl[i, fill[i]] = j
                fill[i] += 1
    excl = -np.sort(-excl, axis=1) if max_excl else excl
    return pos, charges, box, excl


# n, cutoff, exclusions per atom: shift 7, 8 (with and without exclusions), 9
PME_BOX_CASES = [(40000, 8.0, 2), (40000, 8.0, 0), (100000, 8.0, 2), (100000, 8.0, 0), (200000, 5.0, 2)]


@pytest.mark.parametrize("n,cutoff,max_excl", PME_BOX_CASES)
def test_pme_indexed_on_salt_boxes(n, cutoff, max_excl):
    """tests/test_pme_gpu.py::test_indexed_path_matches_the_oracle_and_the_delivering_path at shifts 7-9 (the full oracle: its pair
    sums are vectorised; its per-atom exclusion loop stays within a few seconds at these sizes)."""
    from nnpops_amd import capi
    pos, charges, box, excl = _salt_box(n, seed=70 + n, max_excl=max_excl)
    tpos, tq, tbox = torch.tensor(pos, device=DEV), torch.tensor(charges, device=DEV), torch.tensor(box, device=DEV)
    texcl = torch.tensor(excl, dtype=torch.int32, device=DEV).reshape(n, max_excl).contiguous()
    slots = int(2 * n * 0.05 * 4.19 * cutoff ** 3 / 2)
    nb, dl, ds, found = capi.neighbor_pairs_forward(tpos, cutoff, slots, tbox)
    assert 0 < int(found) < slots
    _check_pme(tpos, tq, nb, dl, ds, texcl, 0.35, 332.063713)


# ---------------------------------------------------------------------------------------------------------------------------------
# the torch op across NNPOPS_PAIRS_INDEX_MAX_ATOMS
# ---------------------------------------------------------------------------------------------------------------------------------
def _sparse_box(n, seed):
    pos, _, box = workloads.random_box(n, density=0.01, seed=seed)
    return pos, box


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [MAX_ATOMS, MAX_ATOMS + 1])
def test_torch_op_gradient_across_the_limit(n, dtype):
    """getNeighborPairs with positions that require a gradient: up to the limit the backward is the indexed gather, one atom more it
    is the fixed-point pass -- each bit for bit what its C ABI entry point gives, both the float64 reference's gradient."""
    from nnpops_amd import capi
    from NNPOps.neighbors import getNeighborPairs
    pos, box = _sparse_box(n, seed=21)
    p = torch.tensor(pos, dtype=dtype, device=DEV).requires_grad_(True)
    tbox = torch.tensor(box, dtype=dtype, device=DEV)
    nb, dl, ds, found = getNeighborPairs(p, 4.0, 4 * n, tbox)
    assert 0 < int(found) <= 4 * n
    rng = np.random.default_rng(n)
    gd = torch.tensor(rng.standard_normal(tuple(dl.shape)), dtype=dtype, device=DEV)
    gs = torch.tensor(rng.standard_normal(tuple(ds.shape)), dtype=dtype, device=DEV)
    # (the unused slots' deltas / distances are NaN: their terms are skipped by the backward, not multiplied by zero here)
    used = nb[0] >= 0
    loss = (gd[used] * dl[used]).sum() + (gs[used] * ds[used]).sum()
    (grad,) = torch.autograd.grad(loss, p)
    gd, gs = gd * used[:, None], gs * used
    nb, dl, ds = nb.detach(), dl.detach(), ds.detach()
    if n <= MAX_ATOMS:
        same = capi.neighbor_pairs_backward_indexed(n, nb, dl, ds, gd, gs, capi.neighbor_pairs_build_index(n, nb))
    else:
        same = capi.neighbor_pairs_backward(n, nb, dl, ds, gd, gs)
    assert torch.equal(grad, same)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    ref = neighbor_pairs_backward_oracle(n, nb.cpu().numpy(), f64(dl), f64(ds), f64(gd), f64(gs))
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    np.testing.assert_allclose(grad.cpu().numpy(), ref, rtol=tol, atol=tol * np.abs(ref).max())


def test_pme_direct_never_takes_an_index_cached_for_another_list():
    """A differentiable getNeighborPairs at 40 000 atoms caches its list's index; one at 262 145 atoms builds none, so pme_direct on
    the second list must take the path that assumes nothing, and give the C ABI's non-indexed result."""
    from nnpops_amd import capi
    from NNPOps.neighbors import getNeighborPairs
    small, box_s = _sparse_box(40000, seed=4)
    getNeighborPairs(torch.tensor(small, device=DEV).requires_grad_(True), 4.0, 4 * 40000, torch.tensor(box_s, device=DEV))
    n = MAX_ATOMS + 1
    pos, box = _sparse_box(n, seed=5)
    p = torch.tensor(pos, device=DEV).requires_grad_(True)
    nb, dl, ds, found = getNeighborPairs(p, 4.0, 4 * n, torch.tensor(box, device=DEV))
    assert 0 < int(found) <= 4 * n
    rng = np.random.default_rng(8)
    q = torch.tensor((rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 1.0, n)).astype(np.float32), device=DEV).requires_grad_(True)
    excl = torch.zeros((n, 0), dtype=torch.int32, device=DEV)
    pp = p.detach().clone().requires_grad_(True)
    energy = torch.ops.pme.pme_direct(pp, q, nb, dl.detach(), ds.detach(), excl, 0.35, 332.063713)
    pd, cd = torch.autograd.grad(energy, (pp, q))
    e_d, pd_d, cd_d = capi.pme_direct(pp.detach(), q.detach(), nb, dl.detach(), ds.detach(), excl, 0.35, 332.063713)
    energy = energy.detach()
    assert abs(float(energy) - float(e_d)) <= 1e-6 * float((cd_d * q.detach()).abs().sum())
    assert float((pd - pd_d).abs().max()) <= 2e-6 * float(pd_d.abs().max())
    assert float((cd - cd_d).abs().max()) <= 2e-6 * float(cd_d.abs().max())
