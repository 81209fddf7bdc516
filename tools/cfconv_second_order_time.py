"""The CFConv second-order path at the config-3 shape (10 000 atoms, W = 128, G = 50, the frame and weights of bench.py's cfconv
workload): stream time per call, cases interleaved, medians of several rounds.

    C ABI      compute + backprop                  what a first-order training step costs
               backprop alone, after a compute
               double_backward alone               the new kernel (cfconv_second_order.h), both cotangents
    torch      forward + backward, plain op        CFConv(...)
               forward + backward, _twice op       CFConv(..., twice_differentiable=True), nothing differentiated twice
               force-loss step, _twice op          E -> dE/dpos (create_graph) -> |F - F_ref|^2 -> its gradient
Prints sum_i dM/dpos_i of the double backward as a sanity figure, no reference evaluation.

    python tools/cfconv_second_order_time.py [atoms] [--width W] [--gaussians G]
    python tools/cfconv_second_order_time.py --lib other/libnnpops_hip.so   (and compute + backprop of ANOTHER BUILD of the library,
                                                                             e.g. the parent commit's, in the same interleaved rounds)
    python tools/cfconv_second_order_time.py --profile                      (a few calls only, for rocprofv3 --kernel-trace --stats)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import capi, workloads  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=30, warm=5):
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


class OtherBuild:
    """compute + backprop through ANOTHER build of the library (an older one: it need not export every symbol of this one), called by
    its own C entries: the handles of nnpops_amd.capi belong to the library that module loaded"""

    def __init__(self, path, n, W, G, w):
        self.lib = L = ctypes.CDLL(os.path.abspath(path))
        for name, (restype, argtypes) in capi.SIGNATURES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        self.w = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in w]
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self.nb, self.cf = ctypes.c_void_p(), ctypes.c_void_p()
        self.ok(L.nnpops_cfconv_neighbors_create(ctypes.byref(self.nb), n, 5.0, 1, 0))
        self.ok(L.nnpops_cfconv_create(ctypes.byref(self.cf), n, W, G, 5.0, 1, 0.1, 0, *[ptr(a) for a in self.w], 0))
        self.out = torch.empty((n, W), dtype=torch.float32, device=dev)
        self.xg, self.pg = torch.empty_like(self.out), torch.empty((n, 3), dtype=torch.float32, device=dev)

    def ok(self, code):
        if code != 0:
            raise RuntimeError(self.lib.nnpops_last_error().decode())

    def build(self, pos, box):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ok(self.lib.nnpops_cfconv_neighbors_set_stream(self.nb, stream))
        self.ok(self.lib.nnpops_cfconv_set_stream(self.cf, stream))
        for _ in range(8):
            self.ok(self.lib.nnpops_cfconv_neighbors_build(self.nb, pos.data_ptr(), box.data_ptr()))
            if self.lib.nnpops_cfconv_neighbors_check(self.nb, None) == 0:
                return
        raise RuntimeError("neighbour buffers kept overflowing")

    def step(self, pos, box, x, g):
        L = self.lib
        self.ok(L.nnpops_cfconv_compute(self.cf, self.nb, pos.data_ptr(), box.data_ptr(), x.data_ptr(), self.out.data_ptr()))
        self.ok(L.nnpops_cfconv_backprop(self.cf, self.nb, pos.data_ptr(), box.data_ptr(), x.data_ptr(), g.data_ptr(), self.xg.data_ptr(),
                                         self.pg.data_ptr()))

    def __del__(self):
        self.lib.nnpops_cfconv_destroy(self.cf)
        self.lib.nnpops_cfconv_neighbors_destroy(self.nb)


def handles(n, W, G, w):
    return capi.CFConvNeighbors(n, 5.0, periodic=True), capi.CFConv(n, W, G, 5.0, 0.1, "ssp", *w, periodic=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("atoms", nargs="?", type=int, default=10000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--gaussians", type=int, default=50)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    n, W, G = args.atoms, args.width, args.gaussians
    pos, _, box = workloads.random_box(n, density=0.1, seed=3)
    rng = np.random.default_rng(4)
    w = ((0.1 * rng.standard_normal((W, G))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32),
         (0.1 * rng.standard_normal((W, W))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32))
    tpos, tbox = torch.tensor(pos, device=dev), torch.tensor(box, device=dev)
    rnd = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32), device=dev)
    tx, tg, tV, tQ, tF = rnd(n, W), rnd(n, W), rnd(n, W), rnd(n, 3), rnd(n, 3)

    nb, cf = handles(n, W, G, w)
    nb.build(tpos, tbox)
    cf.compute(nb, tpos, tx, tbox)

    def step_c():
        cf.compute(nb, tpos, tx, tbox)
        cf.backprop(nb, tpos, tx, tg, tbox)

    variants = [("C: compute + backprop", step_c),
                ("C: backprop", lambda: cf.backprop(nb, tpos, tx, tg, tbox)),
                ("C: double_backward", lambda: cf.double_backward(nb, tpos, tx, tg, tV, tQ))]
    if args.lib:
        other = OtherBuild(args.lib, n, W, G, w)
        other.build(tpos, tbox)
        variants.append((f"C: compute + backprop of {args.lib}", lambda: other.step(tpos, tbox, tx, tg)))

    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    neighbors = CFConvNeighbors(5.0)
    module = lambda twice: CFConv(0.1, "ssp", torch.tensor(w[0]).reshape(G, W), torch.tensor(w[1]), torch.tensor(w[2]), torch.tensor(w[3]),
                                  twice_differentiable=twice)
    plain, twice = module(False), module(True)
    ppos, px = tpos.clone().requires_grad_(True), tx.clone().requires_grad_(True)
    neighbors.build(ppos, tbox)

    def first_order(conv):
        return torch.autograd.grad((conv(neighbors, ppos, px, tbox) * tg).sum(), [ppos, px])

    def force_loss():
        energy = (twice(neighbors, ppos, px, tbox) * tg).sum()
        force, = torch.autograd.grad(energy, ppos, create_graph=True)
        return torch.autograd.grad(((force - tF) ** 2).sum(), [ppos, px])

    variants += [("torch: forward + backward, plain op", lambda: first_order(plain)),
                 ("torch: forward + backward, _twice op", lambda: first_order(twice)),
                 ("torch: force-loss step, _twice op", force_loss)]
    if args.profile:
        for _ in range(3):
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        return
    rounds = [[timed(fn) for _, fn in variants] for _ in range(args.rounds)]      # interleaved: all see the same clocks
    med = [float(np.median([r[k] for r in rounds])) for k in range(len(variants))]
    spread = [float(np.max([r[k] for r in rounds]) - np.min([r[k] for r in rounds])) for k in range(len(variants))]
    print(f"cfconv {n} atoms W={W} G={G}, {nb.num_pairs()} pairs, medians of {args.rounds} interleaved rounds (spread = max - min):")
    for (name, _), m, s in zip(variants, med, spread):
        print(f"  {name:50s} {m:9.1f} us  (spread {s:.1f})")
    print(f"  double_backward / backprop                         {med[2] / med[1]:9.2f}")
    dg, dx, dp = cf.double_backward(nb, tpos, tx, tg, tV, tQ)
    print(f"  |sum_i dM/dpos_i| {float(dp.double().sum(0).abs().max() / dp.abs().max()):.1e} of the largest entry; max |dM/dpos| {float(dp.abs().max()):.3e}")


if __name__ == "__main__":
    main()
