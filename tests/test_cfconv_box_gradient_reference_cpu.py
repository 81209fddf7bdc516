"""What pins the float64 restatement of the periodic CFConv that the box-gradient tests compare against (CPU only).

The restatement itself is `Restatement` of tests/cfconv_float64.py; its head says what it computes.

What pins it:
    output, dL/dx, dL/dpos   against the float32 CFConvOracle at the tolerances of tests/test_cfconv_gpu.py (the oracle is the float32
        party here: 2e-5 relative + 2e-6 of the largest entry on output and input gradient, 1e-4 of the largest force).
    dL/dB, all nine entries  against central differences of the restatement's own L in the box entry, positions held fixed and the
        shifts RECOMPUTED at every displaced box, Richardson-extrapolated from the steps h = 2^-14 and 2^-15.  The cosine cutoff
        keeps L continuous when a pair enters or leaves, but its second derivative jumps there, which a difference quotient sees
        and no extrapolation removes -- so the test asserts that the pair list and the shifts at every displaced box are those of
        the undisplaced one (the frames are chosen so; nothing about the code under test enters that choice).  What is left:
        truncation of order h^4, rounding eps |L| / h ~ 1e-16 * 1e2 / 3e-5 ~ 3e-10 absolute.  Bar: 1e-6 of the largest entry, two
        orders below the 1e-4 gate of the GPU tests.
What it also measures (printed, pytest -s): the kernel's formula on float32 records -- float64 products of the float64 pair scalars
    with float32-rounded displacements, the shifts recovered the way image_shift does (three float32 roundings per axis).  The
    recovered shifts are asserted to be the builder's exactly; the distance of that figure from the full float64 value is printed
    (2e-8 ... 3e-8 of the largest entry), and again with 1e-5 of independent relative noise on every pair scalar (8e-6 ... 3e-5):
    the 1e-4 bar of the GPU tests leaves room for the float32 filter arithmetic behind the pair scalars.
"""
import ctypes

import numpy as np
import pytest
import torch

from cfconv_float64 import FORCE_RTOL, OUT_ATOL_FRAC, OUT_RTOL, Restatement, frame, recovered_shifts, weights
from oracle import CFConvNeighborsOracle, CFConvOracle

FD_RTOL = 1e-6


# ---------------------------------------------------------------------------------------------- the pinning tests
PIN_CASES = [("triclinic80", 8, 6, 4.0, 0.5, "ssp"), ("cubic100", 12, 9, 4.5, 0.4, "tanh")]
PIN_IDS = [c[0] + "-" + c[5] for c in PIN_CASES]


@pytest.mark.parametrize("tag,W,G,cutoff,sigma,act", PIN_CASES, ids=PIN_IDS)
def test_restatement_is_the_oracle(tag, W, G, cutoff, sigma, act):
    pos, box = frame(tag)
    n = len(pos)
    w1, b1, w2, b2, x, gy = weights(W, G, n, 17)
    onb = CFConvNeighborsOracle(n, cutoff, True)
    onb.build(pos, box)
    ocf = CFConvOracle(n, W, G, cutoff, sigma, act, w1, b1, w2, b2, periodic=True)
    y_ref = ocf.forward(onb, pos, x, box)
    xg_ref, pg_ref = ocf.backward(onb, pos, x, gy, box)
    out = Restatement(W, G, cutoff, sigma, act, w1, b1, w2, b2).evaluate(pos, box, x, gy)
    start, other, _ = onb.export()
    assert np.array_equal(np.repeat(np.arange(n), np.diff(start)), out["i"]) and np.array_equal(other, out["j"])      # the same half list
    assert np.abs(out["n"]).max() == 1 and np.abs(out["gbox"]).max() > 0                                              # wrapped pairs exist
    np.testing.assert_allclose(y_ref, out["out"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(out["out"]).max())
    np.testing.assert_allclose(xg_ref, out["gx"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(out["gx"]).max())
    err = np.abs(pg_ref - out["g"]).max() / np.abs(out["g"]).max()
    print(f"\n[cfconv-box-reference] {tag} {act}: oracle position gradient {err:.2e} of max")
    assert err <= FORCE_RTOL


@pytest.mark.parametrize("tag,W,G,cutoff,sigma,act", PIN_CASES, ids=PIN_IDS)
def test_box_gradient_against_finite_differences(tag, W, G, cutoff, sigma, act):
    pos, box = frame(tag)
    w1, b1, w2, b2, x, gy = weights(W, G, len(pos), 17)
    judge = Restatement(W, G, cutoff, sigma, act, w1, b1, w2, b2)
    base = judge.evaluate(pos, box, x, gy)
    pos64, box64 = pos.astype(np.float64), box.astype(np.float64)

    def energy(b):
        L, (pi, pj, pn) = judge.energy(pos64, b, x, gy)
        assert np.array_equal(pi, base["i"]) and np.array_equal(pj, base["j"]) and np.array_equal(pn, base["n"]), \
            "a pair crosses the cutoff (or changes its image) inside the finite-difference step"
        return L

    worst, top = 0.0, np.abs(base["gbox"]).max()
    for k in range(3):
        for c in range(3):
            def central(h):
                plus, minus = box64.copy(), box64.copy()
                plus[k, c] += h; minus[k, c] -= h
                return (energy(plus) - energy(minus)) / (2 * h)
            fd = (4.0 * central(2.0 ** -15) - central(2.0 ** -14)) / 3.0
            worst = max(worst, abs(fd - base["gbox"][k, c]))
    smallest = np.abs(base["gbox"]).min()
    print(f"\n[cfconv-box-reference] {tag} {act}: box gradient vs finite differences {worst / top:.2e} of max {top:.3e} "
          f"(smallest entry {smallest / top:.1e} of max)")
    assert worst <= FD_RTOL * top, (tag, worst, top)


# ---------------------------------------------------------------------------------------------- the kernel's formula on float32 records
@pytest.mark.parametrize("tag", ["triclinic350", "liquid1500", "dense1100", "liquid600_shifted"])
def test_formula_on_float32_records(tag):
    pos, box = frame(tag)
    W, G = 16, 8
    w1, b1, w2, b2, x, gy = weights(W, G, len(pos), 23)
    out = Restatement(W, G, 5.0, 0.4, "ssp", w1, b1, w2, b2).evaluate(pos, box, x, gy)
    rec = out["d"].astype(np.float32)
    n_rec = recovered_shifts(pos, box, out["i"], out["j"], rec)
    assert np.array_equal(n_rec, out["n"]), "image_shift's three roundings do not recover the builder's shifts"
    wrapped = float((np.abs(out["n"]).sum(axis=1) > 0).mean())
    top = np.abs(out["gbox"]).max()
    gB_rec = n_rec.T @ (out["s"][:, None] * rec.astype(np.float64))
    noise = 1.0 + 1e-5 * np.random.default_rng(1).standard_normal(len(out["s"]))
    gB_noise = n_rec.T @ ((out["s"] * noise)[:, None] * rec.astype(np.float64))
    x64, B64 = pos.astype(np.float64), box.astype(np.float64)
    stress = x64.T @ out["g"] + B64.T @ out["gbox"]
    print(f"\n[cfconv-box-reference] {tag}: {len(out['i'])} pairs, {wrapped:.0%} wrapped; records-only {np.abs(gB_rec - out['gbox']).max() / top:.2e}, "
          f"with 1e-5 noise on s {np.abs(gB_noise - out['gbox']).max() / top:.2e} of max {top:.3e}; smallest entry "
          f"{np.abs(out['gbox']).min() / top:.1e} of max; antisymmetric stress {np.abs(stress - stress.T).max() / 2 / np.abs(stress).max():.1e}")
    assert wrapped > 0 and np.isfinite(out["gbox"]).all()
    assert np.abs(gB_rec - out["gbox"]).max() <= 1e-6 * top          # float32 displacements: 6e-8 relative each, far below the bar
    assert np.abs(stress - stress.T).max() / 2 <= 1e-10 * np.abs(stress).max()      # rotation invariance, float64


# ---------------------------------------------------------------------------------------------- the symbol and the op exist
def test_library_exports_backprop_box_and_reports_a_null_handle():
    from nnpops_amd import capi
    L = capi.lib()
    assert hasattr(L, "nnpops_cfconv_backprop_box")
    null = ctypes.c_void_p()
    code = L.nnpops_cfconv_backprop_box(null, null, null, null, null, null, null, null, null)
    assert code < 0 and b"NULL" in L.nnpops_last_error()


def test_operation_periodic_is_registered():
    from nnpops_amd import torch_binding
    torch_binding.load()
    assert hasattr(torch.ops.NNPOpsCFConv, "operation_periodic")
    schema = str(torch.ops.NNPOpsCFConv.operation_periodic.default._schema)
    assert schema.count("Tensor") >= 4, schema
