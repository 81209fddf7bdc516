"""What pins the float64 restatement of the AEV that the box-gradient tests compare against: oracle.AniOracle64 (CPU only).

The restatement itself is `Restatement` of tests/ani_float64.py; its head says what it computes.

What pins it (both angle modes, a ~60-atom triclinic and a ~100-atom cubic frame, cutoffs below half the box):
    values, position gradient   max |x - oracle| <= 1e-10 max |oracle|      (AniOracle64: oracle/ani_oracle.c in double precision)
    cell gradient (lower triangle)  against central finite differences of L = <w_r, radial> + <w_a, angular> evaluated with
        AniOracle64, Richardson-extrapolated from the steps h = 2^-13 and 2^-14 Angstrom.  The oracle rounds its box to float32, so
        the steps are powers of two, exactly representable next to a ~10 Angstrom entry (ulp 2^-20).  A pair that crosses a cutoff
        inside the step does so with value and slope zero (cosine cutoff) but with a jump J ~ 0.1 |w| in the SECOND derivative,
        which a difference quotient sees as an error of up to J h / 2 and no extrapolation removes: with h = 2^-8 the triclinic
        frame was 4e-6 .. 7e-6 of its largest entry off, hence the small steps (J h / 2 ~ 3e-6 absolute, 2e-7 of the largest
        entry, should a pair cross at all).  The rest is smaller: truncation of order h^4 after the extrapolation, rounding
        eps |L| / h ~ 2e-9 absolute.  Bar: 1e-6 of the largest entry, two orders below the 1e-4 gate of the GPU tests; measured
        3e-12 .. 1e-11.
"""
import numpy as np
import pytest

from ani_float64 import Restatement, system, weights
from nnpops_amd import workloads
from oracle import AniOracle64

# ---------------------------------------------------------------------------------------------- the pinning tests
PIN_RTOL = 1e-10
FD_RTOL = 1e-6


@pytest.mark.parametrize("torchani", [True, False], ids=["torchani", "paper"])
@pytest.mark.parametrize("tag", ["triclinic60", "cubic100"])
def test_restatement_is_the_oracle(tag, torchani):
    n_species, rcr, rca, species, pos, box = system(tag)
    rf, af = workloads.ani2x_functions()
    oracle = AniOracle64(n_species, rcr, rca, species, rf, af, periodic=True, torchani=torchani)
    r_ref, a_ref = oracle.forward(pos, box)
    wr, wa = weights(r_ref.shape, a_ref.shape, 17)
    g_ref = oracle.backward(wr, wa)
    out = Restatement(n_species, rcr, rca, species, rf, af, torchani).evaluate(pos, box, wr, wa)
    assert np.abs(a_ref).max() > 0 and np.abs(out["gbox"]).max() > 0          # (triples and wrapped pairs exist)
    for name, x, x_ref in (("radial", out["r"], r_ref), ("angular", out["a"], a_ref), ("position gradient", out["g"], g_ref)):
        err = np.abs(x - x_ref).max() / np.abs(x_ref).max()
        print(f"\n[ani-box-reference] {tag} torchani={torchani}: {name} {err:.2e} of max")
        assert err <= PIN_RTOL, (tag, name, err)


@pytest.mark.parametrize("torchani", [True, False], ids=["torchani", "paper"])
@pytest.mark.parametrize("tag", ["triclinic60", "cubic100"])
def test_cell_gradient_against_finite_differences_of_the_oracle(tag, torchani):
    n_species, rcr, rca, species, pos, box = system(tag)
    rf, af = workloads.ani2x_functions()
    oracle = AniOracle64(n_species, rcr, rca, species, rf, af, periodic=True, torchani=torchani)
    r0, a0 = oracle.forward(pos, box)
    wr, wa = weights(r0.shape, a0.shape, 17)
    w_r, w_a = wr.astype(np.float64), wa.astype(np.float64)

    def energy(b):
        assert np.array_equal(b.astype(np.float32).astype(np.float64), b)       # (the oracle's float32 box is the box meant)
        r, a = oracle.forward(pos, b)
        return float((r * w_r).sum() + (a * w_a).sum())

    out = Restatement(n_species, rcr, rca, species, rf, af, torchani).evaluate(pos, box, wr, wa)
    box64 = np.asarray(box, dtype=np.float64)
    worst, top = 0.0, np.abs(np.tril(out["gbox"])).max()
    for k in range(3):
        for c in range(k + 1):                     # the lower triangle: the entries the minimum-image rule reads
            def central(h):
                plus, minus = box64.copy(), box64.copy()
                plus[k, c] += h; minus[k, c] -= h
                return (energy(plus) - energy(minus)) / (2 * h)
            fd = (4.0 * central(2.0 ** -14) - central(2.0 ** -13)) / 3.0
            worst = max(worst, abs(fd - out["gbox"][k, c]))
    print(f"\n[ani-box-reference] {tag} torchani={torchani}: cell gradient vs finite differences {worst / top:.2e} of max {top:.3e}")
    assert worst <= FD_RTOL * top, (tag, worst, top)
