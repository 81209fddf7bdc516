"""What pins the float64 judge of the CFConv second derivatives (CPU only).

The judge itself is `SecondOrder` of tests/cfconv_float64.py, over the pairs and shifts of that module's `Restatement`; its head says
what both compute.

What pins it:
    out, gx, gp            against the float32 CFConvOracle at OUT_RTOL / OUT_ATOL_FRAC / FORCE_RTOL of tests/cfconv_float64.py.
    dM/dg, dM/dx, dM/dpos  against the closed-form expressions the kernels implement (`closed_form` of that module writes them
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

import numpy as np
import pytest
import torch

from cfconv_float64 import (FORCE_RTOL, OUT_ATOL_FRAC, OUT_RTOL, Restatement, SecondOrder, _wide, closed_form, cotangents, frame,
                            weights)
from oracle import CFConvNeighborsOracle, CFConvOracle

CLOSED_FORM_RTOL = 1e-12
FD_RTOL = 2e-10
FD_DIRECTION_RTOL = 6e-10

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
