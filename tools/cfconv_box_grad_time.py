"""The CFConv backward with and without its box-gradient pass (C ABI) at the periodic config-3 shape (10 000 atoms, W = 128,
G = 50, the frame and weights of bench.py's cfconv workload): stream time per call of backprop() and of backprop_box(), interleaved,
and their difference -- what the pass (one launch over rows, pair slots and pair scalars + the finishing launch) adds.  Both follow
a forward call on the same build, as in a training step.  Prints the stress symmetry of the result as a sanity figure, no
reference evaluation.

    python tools/cfconv_box_grad_time.py [atoms] [--width W] [--gaussians G]
    python tools/cfconv_box_grad_time.py --lib other/libnnpops_hip.so      (and the backprop() of ANOTHER BUILD of the library, e.g.
                                                                            the parent commit's, in the same interleaved rounds)
    python tools/cfconv_box_grad_time.py --profile                         (a few calls only, for rocprofv3 --kernel-trace --stats)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import capi, workloads  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=100, warm=10):
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


def other_build(path):
    """another build of the library (an older one: it need not export every symbol of this one)"""
    other = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        if hasattr(other, name):
            fn = getattr(other, name)
            fn.restype, fn.argtypes = restype, argtypes
    return other


def handles(n, W, G, w, library=None):
    product = capi.lib()
    if library is not None:
        capi._lib = library
    try:
        nb = capi.CFConvNeighbors(n, 5.0, periodic=True)
        cf = capi.CFConv(n, W, G, 5.0, 0.1, "ssp", *w, periodic=True)
    finally:
        capi._lib = product
    return nb, cf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("atoms", nargs="?", type=int, default=10000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--gaussians", type=int, default=50)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    n, W, G = args.atoms, args.width, args.gaussians
    pos, _, box = workloads.random_box(n, density=0.1, seed=3)
    rng = np.random.default_rng(4)
    w = ((0.1 * rng.standard_normal((W, G))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32),
         (0.1 * rng.standard_normal((W, W))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32))
    tpos, tbox = torch.tensor(pos, device=dev), torch.tensor(box, device=dev)
    tx = torch.tensor(rng.standard_normal((n, W)).astype(np.float32), device=dev)
    tg = torch.tensor(rng.standard_normal((n, W)).astype(np.float32), device=dev)

    def prepared(library=None):
        nb, cf = handles(n, W, G, w, library)
        nb.build(tpos, tbox)
        cf.compute(nb, tpos, tx, tbox)
        return nb, cf

    nb, cf = prepared()
    plain = lambda: cf.backprop(nb, tpos, tx, tg, tbox)
    with_box = lambda: cf.backprop_box(nb, tpos, tx, tg, tbox)
    variants = [("backprop", plain), ("backprop_box", with_box)]
    if args.lib:
        nb0, cf0 = prepared(other_build(args.lib))
        variants.append((f"backprop of {args.lib}", lambda: cf0.backprop(nb0, tpos, tx, tg, tbox)))
    if args.profile:
        for _ in range(5):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        return
    rounds = [[timed(fn) for _, fn in variants] for _ in range(args.rounds)]      # interleaved: all see the same clocks
    med = [float(np.median([r[k] for r in rounds])) for k in range(len(variants))]
    spread = [float(np.max([r[k] for r in rounds]) - np.min([r[k] for r in rounds])) for k in range(len(variants))]
    xg, pg, gb = with_box()
    x, B = tpos.double(), tbox.double()
    Wm = x.T @ pg.double() + B.T @ gb.double()
    print(f"cfconv {n} atoms W={W} G={G}, {nb.num_pairs()} pairs, medians of {args.rounds} interleaved rounds (spread = max - min):")
    for (name, _), m, s in zip(variants, med, spread):
        print(f"  {name:40s} {m:8.1f} us  (spread {s:.1f})")
    print(f"  box pass = backprop_box - backprop     {med[1] - med[0]:+8.1f} us"
          + (f";  backprop against the other build {med[0] - med[2]:+.1f} us" if args.lib else ""))
    print(f"  antisymmetric stress {float((Wm - Wm.T).abs().max() / 2 / Wm.abs().max()):.1e} of max; max |dL/dbox| {float(gb.abs().max()):.3e}")


if __name__ == "__main__":
    main()
