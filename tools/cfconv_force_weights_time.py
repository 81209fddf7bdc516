"""The CFConv weight gradients of a force loss at the config-3 shape (10 000 atoms, W = 128, G = 50, the frame and weights of bench.py's
cfconv workload) and on a batched list of 64 molecules of 21 atoms: stream time per call after a warm-up, event brackets, cases
interleaved, medians of several rounds.

    (a) C ABI   double_backward_weights            the new kernels (cfconv_weight_grad_second.h): pair scalars, partial rows, float64 sum
    (b) C ABI   backprop_weights                   the first-order weight gradients (cfconv_weight_grad.h), in the same run
    (c) torch   the same sums by restatement       the filter network in plain float32 torch over the exported pair list on the device,
                                                   autograd twice: a create_graph first backward, M = <V, gx> + <Q, gp>, then the four arrays
    (d) torch   force-loss training step           CFConv(..., force_trainable=True): E, F = -grad(E, pos, create_graph=True),
                                                   (E^2 + |F|^2).backward() -> positions, input and the four parameters; against the
                                                   same step with twice_differentiable=True and fixed weights
Prints the largest difference between the kernel's and the restatement's gradients, as a fraction of the largest entry, as a sanity
figure (both are float32).

    python tools/cfconv_force_weights_time.py [--rounds R] [--shape config3|batch|both]"""
import argparse
import math
import os
import sys

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


def measure(title, pos, box, offsets, W, G, rounds):
    n, cutoff, sigma = len(pos), 5.0, 0.1
    periodic = box is not None
    rng = np.random.default_rng(4)
    w = ((0.1 * rng.standard_normal((W, G))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32),
         (0.1 * rng.standard_normal((W, W))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32))
    tpos = torch.tensor(pos, device=dev)
    tbox = torch.tensor(box, device=dev) if periodic else None
    rnd = lambda *shape: torch.tensor(rng.standard_normal(shape).astype(np.float32), device=dev)
    tx, tg, tV, tQ = rnd(n, W), rnd(n, W), rnd(n, W), rnd(n, 3)

    nb = capi.CFConvNeighbors(n, cutoff, periodic=periodic)
    if offsets is not None:
        nb.set_molecules(offsets)
    cf = capi.CFConv(n, W, G, cutoff, sigma, "ssp", *w, periodic=periodic)
    nb.build(tpos, tbox)
    cf.compute(nb, tpos, tx, tbox)
    cf.backprop_weights(nb, tx, tg)
    cf.double_backward_weights(nb, tx, tg, tV, tQ)

    # (c) the restatement: the exported half list on the device, displacements from the positions (orthorhombic minimum image)
    atoms, _ = nb.export()
    pi, pj = torch.tensor(atoms[0].astype(np.int64), device=dev), torch.tensor(atoms[1].astype(np.int64), device=dev)
    d0 = tpos[pj] - tpos[pi]
    if periodic:
        diag = torch.diagonal(tbox)
        d0 = d0 - torch.round(d0 / diag) * diag
    mu = torch.arange(G, device=dev, dtype=torch.float32) * (cutoff / (G - 1))
    leaves = [torch.tensor(a, device=dev, requires_grad=True) for a in w]
    dQ = tQ[pj] - tQ[pi]

    def restated():
        w1, b1, w2, b2 = leaves
        d = d0.clone().requires_grad_(True)
        x = tx.clone().requires_grad_(True)
        r = d.norm(dim=1)
        gamma = torch.exp(-0.5 * ((r[:, None] - mu[None, :]) / sigma) ** 2)
        y1 = torch.log(0.5 * torch.exp(gamma @ w1.T + b1) + 0.5)
        y2 = (0.5 * torch.cos(math.pi * r / cutoff) + 0.5)[:, None] * (y1 @ w2.T + b2)
        L = (y2 * (x[pj] * tg[pi] + x[pi] * tg[pj])).sum()            # <g, out> without forming out
        gx, gd = torch.autograd.grad(L, [x, d], create_graph=True)
        M = (tV * gx).sum() + (gd * dQ).sum()
        return torch.autograd.grad(M, leaves)

    # (d) the training step through the module
    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    neighbors = CFConvNeighbors(cutoff)
    if offsets is not None:
        neighbors.set_molecules(list(offsets))
    layer = lambda **kw: CFConv(sigma, "ssp", torch.tensor(w[0]).reshape(G, W), torch.tensor(w[1]), torch.tensor(w[2]), torch.tensor(w[3]),
                                **kw).to(dev)
    learning, fixed = layer(force_trainable=True), layer(twice_differentiable=True)
    ppos, px = tpos.clone().requires_grad_(True), tx.clone().requires_grad_(True)
    neighbors.build(ppos.detach(), tbox)

    def step(conv):
        E = (conv(neighbors, ppos, px, tbox) * tg).sum()
        F = -torch.autograd.grad(E, ppos, create_graph=True)[0]
        return torch.autograd.grad(E * E + (F * F).sum(), [ppos, px, *conv.parameters()])

    cases = [("(a) C: double_backward_weights", lambda: cf.double_backward_weights(nb, tx, tg, tV, tQ)),
             ("(a') C: double_backward_weights, Q = NULL", lambda: cf.double_backward_weights(nb, tx, tg, tV, None)),
             ("(b) C: backprop_weights", lambda: cf.backprop_weights(nb, tx, tg)),
             ("(c) torch: float32 restatement, autograd twice", restated),
             ("(d) torch: force-loss step, force_trainable=True", lambda: step(learning)),
             ("(d') torch: force-loss step, twice_differentiable=True", lambda: step(fixed))]
    table = [[timed(fn) for _, fn in cases] for _ in range(rounds)]      # interleaved
    med = [float(np.median([q[k] for q in table])) for k in range(len(cases))]
    spread = [float(np.max([q[k] for q in table]) - np.min([q[k] for q in table])) for k in range(len(cases))]
    print(f"{title}: {n} atoms W={W} G={G}, {nb.num_pairs()} pairs, medians of {rounds} interleaved rounds (spread = max - min):")
    for (name, _), m, s in zip(cases, med, spread):
        print(f"  {name:56s} {m:9.1f} us  (spread {s:.1f})")
    print(f"  (c) / (a) {med[3] / med[0]:6.2f}    (a) / (b) {med[0] / med[2]:6.2f}    (d) - (d') {med[4] - med[5]:9.1f} us")
    mine, theirs = cf.double_backward_weights(nb, tx, tg, tV, tQ), restated()
    for name, a, b in zip(("w1", "b1", "w2", "b2"), mine, theirs):
        print(f"  {name}: max |kernel - restatement| / max |restatement| = {float((a - b.reshape(a.shape)).abs().max() / b.abs().max()):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", choices=("config3", "batch", "both"), default="both")
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--gaussians", type=int, default=50)
    args = ap.parse_args()
    if args.shape in ("config3", "both"):
        pos, _, box = workloads.random_box(10000, density=0.1, seed=3)
        measure("config 3", pos, box, None, args.width, args.gaussians, args.rounds)
    if args.shape in ("batch", "both"):
        pos = np.concatenate([workloads.conformer(21, seed=100 + k)[0] for k in range(64)]).astype(np.float32)
        measure("64 x 21-atom batch", pos, None, [21 * k for k in range(65)], args.width, args.gaussians, args.rounds)


if __name__ == "__main__":
    main()
