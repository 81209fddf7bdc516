"""Second derivatives and box-vector gradients of torch.ops.neighbors.getNeighborPairs on the device (pairs_second_order.hip).

Checked against torch's finite differences (small systems, all-pairs and compacted/indexed lists), against a pure-torch composition
on the op's own neighbour list (cell-grid sizes, periodic triclinic boxes, an indexed list beyond 32 768 atoms), against a numpy
restatement of the formulas (the C ABI through capi), for bitwise reproducibility, and for first-order results bitwise equal to the
kernels that ran before."""
import numpy as np
import pytest
import torch

from nnpops_amd import workloads

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LOWER = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]


@pytest.fixture(scope="module")
def get_pairs():
    import NNPOps  # noqa: F401
    from NNPOps.neighbors import getNeighborPairs
    return getNeighborPairs


def _system(n, seed, dtype, cutoff=5.0):
    pos, _, box = workloads.triclinic_box(n, seed=seed)
    return (torch.tensor(pos, device=DEV, dtype=dtype).requires_grad_(), torch.tensor(box, device=DEV, dtype=dtype).requires_grad_())


def composed(pos, box, nb):
    """deltas / distances of the op's own list as differentiable torch ops: positions[row] - positions[col], the z -> y -> x
    round-based minimum image, the norm."""
    keep = nb[0] >= 0
    row, col = nb[0][keep].long(), nb[1][keep].long()
    d = pos[row] - pos[col]
    if box is not None:
        for a in (2, 1, 0):
            d = d - torch.outer(torch.round(d[:, a] / box[a, a]), box[a])
    return d, d.norm(dim=1)


def _energy(dl, ds, theta):
    c = torch.tensor([0.3, -0.2, 0.9], dtype=dl.dtype, device=dl.device)
    return (theta[0] * torch.exp(-theta[1] * ds ** 2)).sum() + theta[2] * ((dl * c).sum(1) ** 2).sum()


def _op(get_pairs, pos, box, cutoff, slots):
    nb, dl, ds, cnt = get_pairs(pos, cutoff, slots, box)
    assert int(cnt) <= (slots if slots > 0 else nb.shape[1])
    keep = nb[0] >= 0
    return nb, dl[keep], ds[keep]


# ---- finite differences, small systems ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [-1, 600])
def test_gradgradcheck_and_box_gradcheck(get_pairs, mode):
    pos = (9.0 * torch.rand(40, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))).to(DEV).requires_grad_()
    box0 = torch.tensor([[8.0, 0, 0], [1.0, 9.0, 0], [0.5, -1.0, 10.0]], dtype=torch.float64)
    lower = torch.tensor([box0[r, c] for r, c in LOWER], dtype=torch.float64, device=DEV, requires_grad=True)
    rows, cols = torch.tensor([r for r, _ in LOWER], device=DEV), torch.tensor([c for _, c in LOWER], device=DEV)

    def f(p, lw):
        box = torch.zeros(3, 3, dtype=lw.dtype, device=DEV).index_put((rows, cols), lw)
        nb, dl, ds, _ = get_pairs(p, 2.5, mode, box)
        keep = nb[0] >= 0
        return dl[keep], ds[keep]

    assert torch.autograd.gradcheck(lambda lw: f(pos.detach(), lw), (lower,))     # the box alone requiring grad
    assert torch.autograd.gradcheck(f, (pos, lower))
    assert torch.autograd.gradgradcheck(f, (pos, lower))
    assert torch.autograd.gradgradcheck(lambda p: f(p, lower.detach()), (pos,))


# ---- against the composition at cell-grid sizes ---------------------------------------------------------------------------------
def _hvp_and_box(get_pairs, n, seed, dtype, slots):
    pos, box = _system(n, seed, dtype)
    theta = torch.tensor([1.3, 0.1, 0.2], dtype=dtype, device=DEV)
    v = torch.randn(n, 3, dtype=dtype, generator=torch.Generator().manual_seed(seed)).to(DEV)

    def run(dl, ds):
        gx, gb = torch.autograd.grad(_energy(dl, ds, theta), (pos, box), create_graph=True)
        return (gb,) + torch.autograd.grad((gx * v).sum() + (gb * gb).sum(), (pos, box))

    nb, dl, ds = _op(get_pairs, pos, box, 5.0, slots)
    got = run(dl, ds)
    want = run(*composed(pos, box, nb))
    return got, want


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-3)], ids=["float64", "float32"])
def test_cell_grid_hessian_vector_product_and_box_gradient(get_pairs, dtype, tol):
    # 12 000 atoms: the cell-grid search, a compacted list, the indexed first-order gather; float32 to 1e-3 of the largest entry
    got, want = _hvp_and_box(get_pairs, 12000, 31, dtype, 12000 * 40)
    for name, a, b in zip(("dE/dbox", "Hv (positions)", "Hv (box)"), got, want):
        err = float((a - b).abs().max() / b.abs().max())
        assert err < tol, (name, err)


def test_indexed_list_beyond_32768_atoms(get_pairs):
    # buckets of 128 atoms in the transposed index (the shifts the small cases never take)
    got, want = _hvp_and_box(get_pairs, 40000, 37, torch.float64, 40000 * 40)
    for name, a, b in zip(("dE/dbox", "Hv (positions)", "Hv (box)"), got, want):
        err = float((a - b).abs().max() / b.abs().max())
        assert err < 1e-10, (name, err)


@pytest.mark.parametrize("mode", [-1, 300 * 40])
def test_force_matching_loss(get_pairs, mode):
    pos, box = _system(300, 41, torch.float64)
    f_ref = torch.randn(300, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(DEV)

    def loss_grads(dl, ds):
        theta = torch.tensor([1.3, 0.1, 0.2], dtype=torch.float64, device=DEV, requires_grad=True)
        gx, gb = torch.autograd.grad(_energy(dl, ds, theta), (pos, box), create_graph=True)
        assert gx.grad_fn is not None
        loss = ((-gx - f_ref) ** 2).sum() + (gb ** 2).sum()
        return torch.autograd.grad(loss, (theta, pos, box))

    nb, dl, ds = _op(get_pairs, pos, box, 5.0, mode)
    got = loss_grads(dl, ds)
    want = loss_grads(*composed(pos, box, nb))
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10 * float(b.abs().max()))


# ---- reproducibility and the first-order kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_new_outputs_bitwise_reproducible(get_pairs, dtype):
    from nnpops_amd import capi
    pos, box = _system(12000, 43, dtype)
    f_ref = torch.randn(12000, 3, dtype=dtype, generator=torch.Generator().manual_seed(6)).to(DEV)

    def step():
        theta = torch.tensor([1.3, 0.1, 0.2], dtype=dtype, device=DEV, requires_grad=True)
        _, dl, ds = _op(get_pairs, pos, box, 5.0, 12000 * 40)
        gx, gb = torch.autograd.grad(_energy(dl, ds, theta), (pos, box), create_graph=True)
        return (gx, gb) + torch.autograd.grad(((gx + f_ref) ** 2).sum() + (gb ** 2).sum(), (theta, pos, box))

    nb, dl, ds, _ = capi.neighbor_pairs_forward(pos.detach(), 5.0, 12000 * 40, box.detach())
    g = torch.Generator().manual_seed(7)
    gd, gs, hx, hb = (torch.randn(s, generator=g, dtype=dtype).to(DEV) for s in (dl.shape, ds.shape, (12000, 3), (3, 3)))

    def c_abi():
        return (capi.neighbor_pairs_box_backward(12000, nb, pos.detach(), box.detach(), dl, ds, gd, gs),) + \
            capi.neighbor_pairs_double_backward(12000, nb, dl, ds, gs, hx, hb, pos.detach(), box.detach())

    for fn in (step, c_abi):
        first = fn()
        for _ in range(2):
            for a, b in zip(first, fn()):
                assert torch.equal(a, b)


@pytest.mark.parametrize("mode", [-1, 400 * 40])
def test_first_order_bits_unchanged(get_pairs, mode):
    """with create_graph and a box gradient, grad_positions is still the bits of the first-order kernels on the same list"""
    from nnpops_amd import capi
    pos, box = _system(400, 47, torch.float32)
    nb, dl, ds, cnt = get_pairs(pos, 5.0, mode, box)
    assert int(cnt) <= nb.shape[1]
    keep = nb[0] >= 0
    g = torch.Generator().manual_seed(8)
    a, b = torch.randn(dl.shape, generator=g).to(DEV), torch.randn(ds.shape, generator=g).to(DEV)
    e = (dl[keep] * a[keep]).sum() + (ds[keep] * b[keep]).sum()
    gx, gb = torch.autograd.grad(e, (pos, box), create_graph=True)
    assert gx.grad_fn is not None and gb.dtype == torch.float32
    gd, gs = torch.where(keep[:, None], a, 0.0), torch.where(keep, b, 0.0)
    if mode > 0:
        index = capi.neighbor_pairs_build_index(400, nb)
        ref = capi.neighbor_pairs_backward_indexed(400, nb, dl.detach(), ds.detach(), gd, gs, index)
    else:
        ref = capi.neighbor_pairs_backward(400, nb, dl.detach(), ds.detach(), gd, gs)
    assert torch.equal(gx, ref)
    assert torch.equal(gb, capi.neighbor_pairs_box_backward(400, nb, pos.detach(), box.detach(), dl.detach(), ds.detach(), gd, gs))


# ---- the C ABI against a numpy restatement of the formulas ------------------------------------------------------------------
def _numpy_reference(nb, pos, box, dl, ds, gd, gs, hx, hb):
    used = (nb[0] >= 0) & (nb[1] >= 0)
    i, j = nb[0][used], nb[1][used]
    d, r, g = dl[used], ds[used], gs[used]
    D = pos[i] - pos[j] - d
    n = np.zeros_like(D)
    n[:, 2] = np.round(D[:, 2] / box[2, 2])
    n[:, 1] = np.round((D[:, 1] - n[:, 2] * box[2, 1]) / box[1, 1])
    n[:, 0] = np.round((D[:, 0] - n[:, 2] * box[2, 0] - n[:, 1] * box[1, 0]) / box[0, 0])
    G = gd[used] + d * (g / r)[:, None]
    grad_box = -n.T @ G
    w = np.zeros_like(d)
    if hx is not None:
        w += hx[i] - hx[j]
    if hb is not None:
        w -= n @ hb
    dw = (d * w).sum(1)
    outs = [np.zeros_like(dl), np.zeros_like(ds), np.zeros_like(dl), np.zeros_like(ds)]
    outs[0][used] = w
    outs[1][used] = dw / r
    outs[2][used] = (g / r)[:, None] * w
    outs[3][used] = -g * dw / r ** 2
    return grad_box, outs


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-5)], ids=["float64", "float32"])
@pytest.mark.parametrize("mode", [-1, 500 * 40])
@pytest.mark.parametrize("given", ["both", "positions", "box"])
def test_c_abi_against_numpy(dtype, tol, mode, given):
    from nnpops_amd import capi
    pos, box = _system(500, 53, dtype)
    pos, box = pos.detach(), box.detach()
    nb, dl, ds, _ = capi.neighbor_pairs_forward(pos, 5.0, mode, box)
    g = torch.Generator().manual_seed(9)
    gd, gs, hx, hb = (torch.randn(s, generator=g, dtype=dtype).to(DEV) for s in (dl.shape, ds.shape, (500, 3), (3, 3)))
    hx = hx if given in ("both", "positions") else None
    hb = hb if given in ("both", "box") else None
    grad_box = capi.neighbor_pairs_box_backward(500, nb, pos, box, dl, ds, gd, gs)
    outs = capi.neighbor_pairs_double_backward(500, nb, dl, ds, gs, hx, hb, pos if hb is not None else None,
                                               box if hb is not None else None)
    f64 = (lambda t: None if t is None else t.double().cpu().numpy())
    want_box, want = _numpy_reference(nb.cpu().numpy(), *(f64(t) for t in (pos, box, dl, ds, gd, gs, hx, hb)))
    np.testing.assert_allclose(f64(grad_box), want_box, rtol=tol, atol=tol * np.abs(want_box).max())
    for a, b in zip(outs, want):
        np.testing.assert_allclose(f64(a), b, rtol=tol, atol=tol * np.abs(b).max())
