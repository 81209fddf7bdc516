"""The float64 judge of the CFConv second derivatives, and what pins it (CPU only).

`SecondOrder` restates the convolution in torch float64 over a FIXED pair list with frozen shifts -- d_ij = x_j - x_i + n_ij B, the
pairs and n_ij B taken once from the restatement of tests/test_cfconv_box_gradient_reference_cpu.py (loaded from that file) -- as a
differentiable function of positions, input and output gradient.  Autograd with create_graph gives the backward pass (gx, gp) and,
for cotangents V of gx and Q of gp, the gradients of M = <V, gx> + <Q, gp> with respect to (g, x, positions): what
nnpops_cfconv_double_backward returns.  tests/test_cfconv_second_order_gpu.py loads it from this file.

What pins it:
    out, gx, gp            against the float32 CFConvOracle at OUT_RTOL / OUT_ATOL_FRAC / FORCE_RTOL of the box-gradient reference.
    dM/dg, dM/dx, dM/dpos  against the closed-form expressions the kernels implement (`closed_form` below writes them
        out pair by pair with explicit gamma'', act'', fc'' and F''), both activations.  Both sides are float64 and algebraically
        equal: bar 1e-12 of the largest entry (measured 2e-16 ... 7e-16).
    dM/dpos                against central differences of the first backward, M(p + h e) - M(p - h e) over 2h, Richardson-extrapolated
        from h = 2^-14 and 2^-15, for 36 single coordinates and two random directions over all atoms.  F'' jumps where a pair
        crosses the cutoff, so the test asserts that the pair list at every displaced position is the undisplaced one.  Left:
        truncation O(h^4) and rounding eps |M| / h ~ 1e-16 * 1e2 / 3e-5 ~ 3e-10 absolute, 3e-11 of the largest entry.  Measured: single
        coordinates 1.1e-11 ... 2.0e-11 of the largest entry, directional derivatives 3.1e-11 ... 5.7e-11 of their own value.  Bars,
        ten times the worst, one digit: 2e-10 (FD_RTOL) and 6e-10 (FD_DIRECTION_RTOL).
    the library exports nnpops_cfconv_double_backward, reports a null handle, and the two _twice ops and the module's flag exist.
"""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from oracle import CFConvNeighborsOracle, CFConvOracle

_spec = importlib.util.spec_from_file_location("cfconv_box_reference", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  "test_cfconv_box_gradient_reference_cpu.py"))
_box = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_box)
Restatement, frame, weights = _box.Restatement, _box.frame, _box.weights
OUT_RTOL, OUT_ATOL_FRAC, FORCE_RTOL = _box.OUT_RTOL, _box.OUT_ATOL_FRAC, _box.FORCE_RTOL

CLOSED_FORM_RTOL = 1e-12
FD_RTOL = 2e-10
FD_DIRECTION_RTOL = 6e-10


def _wide(a):
    return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))


class SecondOrder:
    """The convolution over a fixed half list (i, j) with frozen shifts [P][3] (d = x_j - x_i + shift), float64, differentiable.
    `judge` is the Restatement that holds the layer."""

    def __init__(self, judge, i, j, shift):
        self.judge = judge
        self.i, self.j = torch.as_tensor(np.asarray(i), dtype=torch.int64), torch.as_tensor(np.asarray(j), dtype=torch.int64)
        self.shift = torch.as_tensor(np.asarray(shift, dtype=np.float64))

    @classmethod
    def periodic(cls, judge, pos, box):
        """pairs and shifts of a periodic frame, by the restatement's own rule"""
        p64, b64 = np.asarray(pos, np.float32).astype(np.float64), np.asarray(box, np.float32).astype(np.float64).reshape(3, 3)
        i, j, n = judge.pairs(p64, b64)
        return cls(judge, i, j, n @ b64)

    @classmethod
    def open(cls, judge, pos):
        """pairs of a non-periodic frame: every i < j below the cutoff"""
        p = np.asarray(pos, np.float32).astype(np.float64)
        r2 = ((p[None] - p[:, None]) ** 2).sum(-1)
        i, j = np.nonzero(np.triu(r2 < judge.cutoff ** 2, 1))
        return cls(judge, i, j, np.zeros((len(i), 3)))

    def margin(self, pos):
        """smallest cutoff - r over the listed pairs"""
        d = _wide(pos)[self.j] - _wide(pos)[self.i] + self.shift
        return float((self.judge.cutoff - d.norm(dim=1)).min()) if len(self.i) else float("inf")

    def forward(self, p, x):
        d = p[self.j] - p[self.i] + self.shift
        y2 = self.judge.filters(d)
        out = torch.zeros_like(x)
        return out.index_add(0, self.i, y2 * x[self.j]).index_add(0, self.j, y2 * x[self.i])

    def first(self, pos, x, g, create_graph=False):
        """-> (out, gx, gp, leaves): leaves = (p, x, g) float64 tensors that require a gradient"""
        p, xin, gin = (_wide(a).requires_grad_(True) for a in (pos, x, g))
        out = self.forward(p, xin)
        gx, gp = torch.autograd.grad((out * gin).sum(), [xin, p], create_graph=create_graph)
        return out, gx, gp, (p, xin, gin)

    def second(self, pos, x, g, V=None, Q=None):
        """-> dict(out, gx, gp, dg, dx, dp) as float64 numpy arrays; a cotangent that is None is zero"""
        out, gx, gp, (p, xin, gin) = self.first(pos, x, g, create_graph=True)
        M = 0.0
        if V is not None:
            M = M + (_wide(V) * gx).sum()
        if Q is not None:
            M = M + (_wide(Q) * gp).sum()
        dg, dx, dp = torch.autograd.grad(M, [gin, xin, p], allow_unused=True)
        z = lambda t, like: (torch.zeros_like(like) if t is None else t).numpy()
        return dict(out=out.detach().numpy(), gx=gx.detach().numpy(), gp=gp.detach().numpy(), dg=z(dg, gin), dx=z(dx, xin), dp=z(dp, p),
                    M=float(M.detach()))


def closed_form(so, pos, x, g, V, Q):
    """dM/dg, dM/dx, dM/dpos pair by pair from the written-out derivatives (no autograd)"""
    J = so.judge
    p, xin, gin, Vt, Qt = (_wide(a) for a in (pos, x, g, V, Q))
    i, j = so.i, so.j
    d = p[j] - p[i] + so.shift
    r = d.norm(dim=1)
    u = d / r[:, None]
    t = r[:, None] - J.mu[None, :]
    s2i = 1.0 / J.sigma ** 2
    gam = torch.exp(-0.5 * t * t * s2i)
    dgam = -t * s2i * gam
    ddgam = (t * t * s2i - 1.0) * s2i * gam
    s1, ds1, dds1 = gam @ J.w1.T + J.b1, dgam @ J.w1.T, ddgam @ J.w1.T
    if J.act == 0:
        sg = torch.sigmoid(s1)
        y, a1, a2 = torch.log(0.5 * torch.exp(s1) + 0.5), sg, sg * (1.0 - sg)
    else:
        th = torch.tanh(s1)
        y, a1, a2 = th, 1.0 - th * th, -2.0 * th * (1.0 - th * th)
    dy, ddy = a1 * ds1, a2 * ds1 * ds1 + a1 * dds1
    S, dS, ddS = y @ J.w2.T + J.b2, dy @ J.w2.T, ddy @ J.w2.T
    k = math.pi / J.cutoff
    fc, dfc, ddfc = 0.5 * torch.cos(k * r) + 0.5, -0.5 * k * torch.sin(k * r), -0.5 * k * k * torch.cos(k * r)
    F = fc[:, None] * S
    F1 = dfc[:, None] * S + fc[:, None] * dS
    F2 = ddfc[:, None] * S + 2.0 * dfc[:, None] * dS + fc[:, None] * ddS
    dQ = Qt[j] - Qt[i]
    a = (u * dQ).sum(1)
    A = Vt[j] * gin[i] + Vt[i] * gin[j]
    B = xin[j] * gin[i] + xin[i] * gin[j]
    F1A, F1B, F2B = (F1 * A).sum(1), (F1 * B).sum(1), (F2 * B).sum(1)
    dg = torch.zeros_like(gin).index_add(0, i, F * Vt[j] + a[:, None] * F1 * xin[j]).index_add(0, j, F * Vt[i] + a[:, None] * F1 * xin[i])
    dx = torch.zeros_like(xin).index_add(0, i, a[:, None] * F1 * gin[j]).index_add(0, j, a[:, None] * F1 * gin[i])
    T = (F1A + a * F2B - a / r * F1B)[:, None] * u + (F1B / r)[:, None] * dQ
    dp = torch.zeros_like(p).index_add(0, i, -T).index_add(0, j, T)
    terms = dict(F1A=float(F1A.abs().max()), aF2B=float((a * F2B).abs().max()))
    return dg.numpy(), dx.numpy(), dp.numpy(), terms


def cotangents(n, W, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, W)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)


PIN_CASES = [("triclinic80", 8, 6, 4.0, 0.5, "ssp"), ("triclinic80", 8, 6, 4.0, 0.5, "tanh"), ("cubic100", 12, 9, 4.5, 0.4, "tanh")]
PIN_IDS = [c[0] + "-" + c[5] for c in PIN_CASES]


def _setup(tag, W, G, cutoff, sigma, act):
    pos, box = frame(tag)
    w1, b1, w2, b2, x, gy = weights(W, G, len(pos), 17)
    judge = Restatement(W, G, cutoff, sigma, act, w1, b1, w2, b2)
    return pos, box, (w1, b1, w2, b2), x, gy, judge, SecondOrder.periodic(judge, pos, box)


@pytest.mark.parametrize("tag,W,G,cutoff,sigma,act", PIN_CASES, ids=PIN_IDS)
def test_restatement_is_the_oracle(tag, W, G, cutoff, sigma, act):
    pos, box, (w1, b1, w2, b2), x, gy, judge, so = _setup(tag, W, G, cutoff, sigma, act)
    n = len(pos)
    onb = CFConvNeighborsOracle(n, cutoff, True)
    onb.build(pos, box)
    ocf = CFConvOracle(n, W, G, cutoff, sigma, act, w1, b1, w2, b2, periodic=True)
    y_ref = ocf.forward(onb, pos, x, box)
    xg_ref, pg_ref = ocf.backward(onb, pos, x, gy, box)
    out, gx, gp, _ = so.first(pos, x, gy)
    out, gx, gp = out.detach().numpy(), gx.numpy(), gp.numpy()
    np.testing.assert_allclose(y_ref, out, rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(out).max())
    np.testing.assert_allclose(xg_ref, gx, rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(gx).max())
    err = np.abs(pg_ref - gp).max() / np.abs(gp).max()
    print(f"\n[cfconv-second-reference] {tag} {act}: oracle position gradient {err:.2e} of max")
    assert err <= FORCE_RTOL


@pytest.mark.parametrize("tag,W,G,cutoff,sigma,act", PIN_CASES, ids=PIN_IDS)
def test_closed_form_is_autograd(tag, W, G, cutoff, sigma, act):
    pos, box, _, x, gy, judge, so = _setup(tag, W, G, cutoff, sigma, act)
    V, Q = cotangents(len(pos), W, 3)
    ref = so.second(pos, x, gy, V, Q)
    dg, dx, dp, terms = closed_form(so, pos, x, gy, V, Q)
    for name, got in (("dg", dg), ("dx", dx), ("dp", dp)):
        top = np.abs(ref[name]).max()
        err = np.abs(got - ref[name]).max() / top
        print(f"\n[cfconv-second-reference] {tag} {act}: closed form {name} {err:.2e} of max {top:.3e}")
        assert top > 0 and err <= CLOSED_FORM_RTOL
    print(f"[cfconv-second-reference] {tag} {act}: largest |F'.A| {terms['F1A']:.3e}, largest |a F''.B| {terms['aF2B']:.3e}")
    # each cotangent alone: the other's terms vanish exactly
    only_v = so.second(pos, x, gy, V, None)
    assert np.array_equal(only_v["dx"], np.zeros_like(only_v["dx"]))
    fwd_v = so.forward(_wide(pos), _wide(V)).numpy()
    assert np.abs(only_v["dg"] - fwd_v).max() <= CLOSED_FORM_RTOL * np.abs(fwd_v).max()


@pytest.mark.parametrize("tag,W,G,cutoff,sigma,act", PIN_CASES[:2], ids=PIN_IDS[:2])
def test_position_gradient_against_finite_differences(tag, W, G, cutoff, sigma, act):
    pos, box, _, x, gy, judge, so = _setup(tag, W, G, cutoff, sigma, act)
    n = len(pos)
    V, Q = cotangents(n, W, 3)
    ref = so.second(pos, x, gy, V, Q)
    p64, b64 = pos.astype(np.float64), box.astype(np.float64)
    base = judge.pairs(p64, b64)
    Vt, Qt, xt, gt = (_wide(a) for a in (V, Q, x, gy))

    def M(p_np):
        pi, pj, pn = judge.pairs(p_np, b64)
        assert np.array_equal(pi, base[0]) and np.array_equal(pj, base[1]) and np.array_equal(pn, base[2]), \
            "a pair crosses the cutoff (or changes its image) inside the finite-difference step"
        p = torch.tensor(p_np, requires_grad=True)
        xin = xt.clone().requires_grad_(True)
        out = so.forward(p, xin)
        gx, gp = torch.autograd.grad((out * gt).sum(), [xin, p])
        return float((Vt * gx).sum() + (Qt * gp).sum())

    def richardson(direction):
        def central(h):
            return (M(p64 + h * direction) - M(p64 - h * direction)) / (2 * h)
        return (4.0 * central(2.0 ** -15) - central(2.0 ** -14)) / 3.0

    top = np.abs(ref["dp"]).max()
    worst, worst_dir = 0.0, 0.0
    rng = np.random.default_rng(5)
    for atom in rng.choice(n, 12, replace=False):
        for c in range(3):
            e = np.zeros_like(p64)
            e[atom, c] = 1.0
            worst = max(worst, abs(richardson(e) - ref["dp"][atom, c]))
    for _ in range(2):
        v = rng.standard_normal(p64.shape)
        v /= np.abs(v).max()
        got, want = richardson(v), float((ref["dp"] * v).sum())
        worst_dir = max(worst_dir, abs(got - want) / abs(want))
    print(f"\n[cfconv-second-reference] {tag} {act}: dM/dpos vs finite differences {worst / top:.2e} of max {top:.3e}; "
          f"directional derivatives {worst_dir:.2e} of their value")
    assert worst <= FD_RTOL * top and worst_dir <= FD_DIRECTION_RTOL


# ---------------------------------------------------------------------------------------------- the symbol, the ops, the flag exist
def test_library_exports_double_backward_and_reports_a_null_handle():
    from nnpops_amd import capi
    L = capi.lib()
    assert hasattr(L, "nnpops_cfconv_double_backward")
    null = ctypes.c_void_p()
    code = L.nnpops_cfconv_double_backward(null, null, null, null, null, null, null, null, null, null)
    assert code < 0 and b"NULL" in L.nnpops_last_error()


def test_twice_ops_are_registered():
    from nnpops_amd import torch_binding
    torch_binding.load()
    for name, tensors in (("operation_twice", 3), ("operation_periodic_twice", 4)):
        assert hasattr(torch.ops.NNPOpsCFConv, name)
        schema = str(getattr(torch.ops.NNPOpsCFConv, name).default._schema)
        assert schema.count("Tensor") >= tensors, schema


def test_module_takes_the_flag_and_scripts():
    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    W, G = 8, 6
    w1, b1, w2, b2, _, _ = weights(W, G, 4, 1)
    args = (0.5, "ssp", torch.tensor(w1).reshape(G, W), torch.tensor(b1), torch.tensor(w2), torch.tensor(b2))
    assert CFConv(*args).twice_differentiable is False

    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.neighbors = CFConvNeighbors(4.0)
            self.conv = CFConv(*args, twice_differentiable=True)

        def forward(self, positions: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
            self.neighbors.build(positions)
            return self.conv(self.neighbors, positions, x)

    layer = Layer()
    assert layer.conv.twice_differentiable is True
    scripted = torch.jit.script(layer)
    assert "operation_twice" in scripted.conv.code and "operation_periodic_twice" in scripted.conv.code
