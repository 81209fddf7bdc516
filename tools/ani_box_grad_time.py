"""The AEV backward with and without its box-gradient pass (C ABI), on the headline frame (10 000-atom ANI-2x liquid) and on the
dense 64-slot frame of the tests: stream time per call of backprop() and of backprop_box(), interleaved, and their difference --
what the pass (one launch over rows, records and leg forces + the finishing launch) adds.  Prints the measured error of the cell
gradient's stress symmetry as a sanity figure, no reference evaluation.

    python tools/ani_box_grad_time.py [atoms]
    python tools/ani_box_grad_time.py --profile [atoms]      (a few calls only, for rocprofv3 --kernel-trace --stats)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import workloads  # noqa: E402
from nnpops_amd.capi import AniSymmetryFunctions  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def frame(label, pos, species, box, profile):
    rf, af = workloads.ani2x_functions()
    sym = AniSymmetryFunctions(7, 5.1, 3.5, species, rf, af, periodic=True)
    tpos, tbox = torch.tensor(pos, device=dev), torch.tensor(box, device=dev)
    radial, angular = sym.compute(tpos, tbox)
    gen = torch.Generator(device=dev).manual_seed(0)
    wr = torch.randn(radial.shape, device=dev, generator=gen)
    wa = torch.randn(angular.shape, device=dev, generator=gen)
    g, gb = torch.empty_like(tpos), torch.empty((3, 3), device=dev)
    plain = lambda: sym.backprop(wr, wa, g)
    with_box = lambda: sym.backprop_box(tpos, tbox, wr, wa, g, gb)
    if profile:
        for _ in range(5):
            plain()
            with_box()
        torch.cuda.synchronize()
        return
    rounds = [(timed(plain), timed(with_box)) for _ in range(5)]      # interleaved: both see the same clocks
    t0, t1 = (float(np.median([r[k] for r in rounds])) for k in (0, 1))
    x, B = tpos.double(), tbox.double()
    W = x.T @ g.double() + B.T @ gb.double()
    what = sym.describe()
    print(f"{label}: backprop {t0:.1f} us, backprop_box {t1:.1f} us, box pass {t1 - t0:+.1f} us  (bwd_mode={what['bwd_mode']} "
          f"scatter={what['scatter']} cells={what['cells']}; antisymmetric stress {float((W - W.T).abs().max() / 2 / W.abs().max()):.1e} of max)")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    profile = "--profile" in sys.argv
    n = int(args[0]) if args else 10000
    frame(f"liquid {n}", *workloads.random_box(n, seed=1), profile)
    if not args:
        frame("dense 900 (64-slot records)", *workloads.random_box(900, density=0.2, seed=33), profile)
