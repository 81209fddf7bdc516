"""The CFConv weight gradients at the config-3 shape (10 000 atoms, W = 128, G = 50, the frame and weights of bench.py's cfconv
workload): stream time per call, cases interleaved, medians of several rounds.

    C ABI      compute + backprop                  what a step with fixed filters costs
               backprop_weights alone              the new kernels (cfconv_weight_grad.h): partial rows, then their float64 sum
               set_weights                         host time as well: it blocks (wall clock, not stream time)
               training step                       build, compute, backprop, backprop_weights, set_weights (wall clock)
    torch      weight gradients by restatement     the filter network written in plain float32 torch over the exported pair list on the
                                                   device, L = <g, out>, torch.autograd.grad for the four arrays: what a user had to do
               forward + backward, trainable       CFConv(..., trainable=True): out, then gradients of positions, input and the weights
Prints the largest difference between the kernel's and the restatement's gradients, as a fraction of the largest entry, as a sanity
figure (both are float32).

    python tools/cfconv_weight_grad_time.py [atoms] [--width W] [--gaussians G] [--rounds R]
    python tools/cfconv_weight_grad_time.py --profile          (a few calls only, for rocprofv3 --kernel-trace --stats)"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import capi, workloads  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=20, warm=3):
    """stream time per call, us"""
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


def walled(fn, reps=10, warm=2):
    """wall clock per call with the device drained, us"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("atoms", nargs="?", type=int, default=10000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--gaussians", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    n, W, G, cutoff, sigma = args.atoms, args.width, args.gaussians, 5.0, 0.1
    pos, _, box = workloads.random_box(n, density=0.1, seed=3)
    rng = np.random.default_rng(4)
    w = ((0.1 * rng.standard_normal((W, G))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32),
         (0.1 * rng.standard_normal((W, W))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32))
    tpos, tbox = torch.tensor(pos, device=dev), torch.tensor(box, device=dev)
    rnd = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32), device=dev)
    tx, tg = rnd(n, W), rnd(n, W)

    nb = capi.CFConvNeighbors(n, cutoff, periodic=True)
    cf = capi.CFConv(n, W, G, cutoff, sigma, "ssp", *w, periodic=True)
    nb.build(tpos, tbox)
    cf.compute(nb, tpos, tx, tbox)
    cf.backprop_weights(nb, tx, tg)

    def step_c():
        cf.compute(nb, tpos, tx, tbox)
        cf.backprop(nb, tpos, tx, tg, tbox)

    def training_step():
        nb.build(tpos, tbox, check=False)
        step_c()
        cf.backprop_weights(nb, tx, tg)
        cf.set_weights(*w)

    # the restatement: the exported half list on the device, the layer in plain float32 torch
    atoms, dist = nb.export()
    pi, pj = torch.tensor(atoms[0].astype(np.int64), device=dev), torch.tensor(atoms[1].astype(np.int64), device=dev)
    r = torch.tensor(dist, device=dev)
    mu = torch.arange(G, device=dev, dtype=torch.float32) * (cutoff / (G - 1))
    leaves = [torch.tensor(a, device=dev, requires_grad=True) for a in w]

    def restated():
        w1, b1, w2, b2 = leaves
        gamma = torch.exp(-0.5 * ((r[:, None] - mu[None, :]) / sigma) ** 2)
        y1 = torch.log(0.5 * torch.exp(gamma @ w1.T + b1) + 0.5)
        y2 = (0.5 * torch.cos(math.pi * r / cutoff) + 0.5)[:, None] * (y1 @ w2.T + b2)
        L = (y2 * (tx[pj] * tg[pi] + tx[pi] * tg[pj])).sum()          # <g, out> without forming out
        return torch.autograd.grad(L, leaves)

    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    neighbors = CFConvNeighbors(cutoff)
    conv = CFConv(sigma, "ssp", torch.tensor(w[0]).reshape(G, W), torch.tensor(w[1]), torch.tensor(w[2]), torch.tensor(w[3]),
                  trainable=True).to(dev)
    ppos, px = tpos.clone().requires_grad_(True), tx.clone().requires_grad_(True)
    neighbors.build(ppos, tbox)

    def module_step():
        return torch.autograd.grad((conv(neighbors, ppos, px, tbox) * tg).sum(), [ppos, px, *conv.parameters()])

    stream = [("C: compute + backprop", step_c),
              ("C: backprop_weights", lambda: cf.backprop_weights(nb, tx, tg)),
              ("torch: weight gradients by float32 restatement", restated),
              ("torch: forward + backward, trainable=True", module_step)]
    wall = [("C: set_weights (wall clock)", lambda: cf.set_weights(*w)),
            ("C: training step (wall clock)", training_step)]
    if args.profile:
        for _ in range(3):
            for _, fn in stream + wall:
                fn()
        torch.cuda.synchronize()
        return
    rounds = [[timed(fn) for _, fn in stream] + [walled(fn) for _, fn in wall] for _ in range(args.rounds)]      # interleaved
    names = [name for name, _ in stream + wall]
    med = [float(np.median([q[k] for q in rounds])) for k in range(len(names))]
    spread = [float(np.max([q[k] for q in rounds]) - np.min([q[k] for q in rounds])) for k in range(len(names))]
    print(f"cfconv {n} atoms W={W} G={G}, {nb.num_pairs()} pairs, path {cf.describe()['path']}, medians of {args.rounds} interleaved rounds "
          "(spread = max - min):")
    for name, m, s in zip(names, med, spread):
        print(f"  {name:50s} {m:9.1f} us  (spread {s:.1f})")
    print(f"  restatement / backprop_weights                     {med[2] / med[1]:9.2f}")
    mine, theirs = cf.backprop_weights(nb, tx, tg), restated()
    for name, a, b in zip(("w1", "b1", "w2", "b2"), mine, theirs):
        print(f"  {name}: max |kernel - restatement| / max |restatement| = {float((a - b.reshape(a.shape)).abs().max() / b.abs().max()):.2e}")


if __name__ == "__main__":
    main()
