"""Second derivatives and box-vector gradients of torch.ops.neighbors.getNeighborPairs on HOST tensors (the CPU dispatch key).

The reference's CPU op is a composition of ATen calls (src/pytorch/neighbors/getNeighborPairsCPU.cpp:56-98), so it is twice
differentiable and differentiable with respect to box_vectors; these tests hold this op to the same, against torch's own finite
differences and against a pure-torch composition on the op's own neighbour list.  Runs without a GPU."""
import pytest
import torch

BOX = [[8.0, 0, 0], [1.0, 9.0, 0], [0.5, -1.0, 10.0]]
LOWER = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]


@pytest.fixture(scope="module")
def get_pairs():
    import NNPOps  # noqa: F401  (loads libNNPOpsPyTorch.so)
    from NNPOps.neighbors import getNeighborPairs
    return getNeighborPairs


def _positions(n, seed, dtype=torch.float64, spread=4.0):
    return (spread * torch.rand(n, 3, dtype=dtype, generator=torch.Generator().manual_seed(seed))).requires_grad_()


def _box_from_lower(lower):
    """[3, 3] box whose six lower-triangular entries are `lower` (differentiable), upper entries zero."""
    box = torch.zeros(3, 3, dtype=lower.dtype)
    return box.index_put((torch.tensor([r for r, _ in LOWER]), torch.tensor([c for _, c in LOWER])), lower)


def composed(pos, box, nb):
    """deltas / distances of the op's own list as differentiable torch ops: positions[row] - positions[col], the z -> y -> x
    round-based minimum image, the norm."""
    keep = nb[0] >= 0
    row, col = nb[0][keep].long(), nb[1][keep].long()
    d = pos[row] - pos[col]
    if box is not None:
        for a in (2, 1, 0):
            d = d - torch.outer(torch.round(d[:, a] / box[a, a]), box[a])
    return keep, d, d.norm(dim=1)


def _energy(dl, ds, theta):
    """a small pair potential that uses both outputs: theta0 exp(-theta1 r^2) + theta2 (d . c)^2"""
    c = torch.tensor([0.3, -0.2, 0.9], dtype=dl.dtype)
    return (theta[0] * torch.exp(-theta[1] * ds ** 2)).sum() + theta[2] * ((dl * c).sum(1) ** 2).sum()


@pytest.mark.parametrize("mode", [-1, 400])
@pytest.mark.parametrize("periodic", [False, True], ids=["vacuum", "triclinic"])
def test_gradgradcheck_positions(get_pairs, mode, periodic):
    pos = _positions(16, 1)
    box = torch.tensor(BOX, dtype=torch.float64) if periodic else None

    def f(p):
        nb, dl, ds, _ = get_pairs(p, 2.5, mode, box)
        keep = nb[0] >= 0
        return dl[keep], ds[keep]

    assert torch.autograd.gradcheck(f, (pos,))
    assert torch.autograd.gradgradcheck(f, (pos,))


@pytest.mark.parametrize("mode", [-1, 400])
def test_box_gradcheck_and_gradgradcheck(get_pairs, mode):
    pos = _positions(16, 2, spread=9.0)
    lower = torch.tensor([BOX[r][c] for r, c in LOWER], dtype=torch.float64, requires_grad=True)

    def f_box(lw):
        nb, dl, ds, _ = get_pairs(pos.detach(), 2.5, mode, _box_from_lower(lw))
        keep = nb[0] >= 0
        return dl[keep], ds[keep]

    def f_both(p, lw):
        nb, dl, ds, _ = get_pairs(p, 2.5, mode, _box_from_lower(lw))
        keep = nb[0] >= 0
        return dl[keep], ds[keep]

    assert torch.autograd.gradcheck(f_box, (lower,))              # the box alone requiring grad
    assert torch.autograd.gradcheck(f_both, (pos, lower))
    assert torch.autograd.gradgradcheck(f_both, (pos, lower))


def test_box_gradient_keeps_the_box_dtype(get_pairs):
    pos = _positions(16, 3, spread=9.0)
    box = torch.tensor(BOX, dtype=torch.float32, requires_grad=True)
    nb, dl, ds, _ = get_pairs(pos, 2.5, 200, box)
    keep = nb[0] >= 0
    (ds[keep] ** 2).sum().backward()
    assert box.grad is not None and box.grad.dtype == torch.float32
    assert pos.grad is not None and pos.grad.dtype == torch.float64


@pytest.mark.parametrize("periodic", [False, True], ids=["vacuum", "triclinic"])
def test_force_matching_loss_matches_the_composition(get_pairs, periodic):
    """d/dtheta of |F(theta) - F_ref|^2 (+ |dE/dbox|^2 in the box): the op against the composition on the op's own list"""
    pos = _positions(24, 4, spread=9.0 if periodic else 4.0)
    box = torch.tensor(BOX, dtype=torch.float64, requires_grad=True) if periodic else None
    inputs = (pos, box) if periodic else (pos,)
    f_ref = torch.randn(24, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    nb = get_pairs(pos.detach(), 2.5, 500, box.detach() if periodic else None)[0]
    keep = nb[0] >= 0

    def loss_grads(dl, ds, theta):
        g = torch.autograd.grad(_energy(dl, ds, theta), inputs, create_graph=True)
        assert g[0].grad_fn is not None                            # the forces are differentiable
        loss = ((-g[0] - f_ref) ** 2).sum() + ((g[1] ** 2).sum() if periodic else 0)
        return torch.autograd.grad(loss, (theta,) + inputs)

    theta = torch.tensor([1.3, 0.7, 0.2], dtype=torch.float64, requires_grad=True)
    nb2, dl, ds, _ = get_pairs(pos, 2.5, 500, box)
    assert torch.equal(nb2, nb)
    got = loss_grads(dl[keep], ds[keep], theta)
    _, dl_c, ds_c = composed(pos, box, nb)
    want = loss_grads(dl_c, ds_c, theta)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-10)


def test_hessian_vector_product_and_box_gradient_match_the_composition(get_pairs):
    pos = _positions(40, 6, spread=9.0)
    box = torch.tensor(BOX, dtype=torch.float64, requires_grad=True)
    v = torch.randn(40, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    nb = get_pairs(pos.detach(), 3.0, 900, box.detach())[0]
    theta = torch.tensor([1.3, 0.7, 0.2], dtype=torch.float64)

    def hvp(pairs):
        keep, dl, ds = pairs()
        e = _energy(dl, ds, theta)
        gx, gb = torch.autograd.grad(e, (pos, box), create_graph=True)
        return (gb,) + torch.autograd.grad((gx * v).sum() + (gb * gb).sum(), (pos, box))

    def op():
        _, dl, ds, _ = get_pairs(pos, 3.0, 900, box)
        keep = nb[0] >= 0
        return keep, dl[keep], ds[keep]

    for a, b in zip(hvp(op), hvp(lambda: composed(pos, box, nb))):
        torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11)


def test_third_derivatives_are_refused(get_pairs):
    pos = _positions(12, 8)
    nb, dl, ds, _ = get_pairs(pos, 2.5, -1, None)
    keep = nb[0] >= 0
    e = (ds[keep] ** 3).sum()
    g = torch.autograd.grad(e, pos, create_graph=True)[0]
    h = torch.autograd.grad((g ** 2).sum(), pos, create_graph=True)[0]
    with pytest.raises(RuntimeError, match="third derivatives are not implemented"):
        torch.autograd.grad(h.sum(), pos)
