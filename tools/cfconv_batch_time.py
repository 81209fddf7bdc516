"""One batched CFConv step against a loop of single-molecule steps: B frames of a 21-atom molecule, W = 128, G = 50, cutoff 5 A.

    batched   one list with molecule offsets (nnpops_cfconv_neighbors_set_molecules), one convolution of B * 21 atoms:
              build + compute + backprop = one launch sequence for the whole batch
    loop      B lists and B convolutions of 21 atoms (the same weights), the same three calls B times

Both go through the C ABI with no host synchronisation inside a step (build without check(), as a captured step runs it), so a
step is launches on one stream: the figure is stream time per step, event-timed, warmed, the two cases interleaved round by round,
medians of the rounds with their spread (max - min).  Prints both columns and their ratio per B; asserts nothing.

    python tools/cfconv_batch_time.py [--frames 8 64 256] [--atoms 21] [--rounds 7]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import capi, workloads  # noqa: E402

dev = torch.device("cuda:0")
CUTOFF, SIGMA = 5.0, 0.1


def timed(fn, reps, warm=3):
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


def frames(B, n, seed=0):
    """B noisy copies of one conformer (frames of a trajectory), each centred on the origin"""
    base = workloads.conformer(n, seed=seed)[0].astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    out = []
    for _ in range(B):
        p = base + rng.normal(0, 0.05, base.shape)
        out.append((p - p.mean(axis=0)).astype(np.float32))
    return np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--atoms", type=int, default=21)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--gaussians", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, W, G = args.atoms, args.width, args.gaussians
    rng = np.random.default_rng(4)
    w = ((0.1 * rng.standard_normal((W, G))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32),
         (0.1 * rng.standard_normal((W, W))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32))
    print(f"cfconv batch: {n}-atom frames, W={W} G={G} cutoff {CUTOFF}; build + compute + backprop per step, stream time, "
          f"medians of {args.rounds} interleaved rounds (spread = max - min)")
    print(f"  {'B':>4s} {'atoms':>6s} {'pairs':>7s} {'batched us':>12s} {'(spread)':>9s} {'loop us':>12s} {'(spread)':>9s} {'loop / batched':>15s} "
          f"{'batched us / frame':>19s}")
    for B in args.frames:
        N = B * n
        pos = torch.tensor(frames(B, n), device=dev)
        x = torch.tensor(rng.standard_normal((N, W)).astype(np.float32), device=dev)
        g = torch.tensor(rng.standard_normal((N, W)).astype(np.float32), device=dev)
        nb, cf = capi.CFConvNeighbors(N, CUTOFF), capi.CFConv(N, W, G, CUTOFF, SIGMA, "ssp", *w)
        nb.set_molecules(np.arange(B + 1) * n)
        out = torch.empty_like(x)
        ones = [(capi.CFConvNeighbors(n, CUTOFF), capi.CFConv(n, W, G, CUTOFF, SIGMA, "ssp", *w)) for _ in range(B)]
        parts = [tuple(t[m * n:(m + 1) * n] for t in (pos, x, g, out)) for m in range(B)]      # (contiguous row blocks: views)

        def batched():
            nb.build(pos, check=False)
            cf.compute(nb, pos, x, out=out)
            cf.backprop(nb, pos, x, g)

        def loop():
            for (nb1, cf1), (p1, x1, g1, o1) in zip(ones, parts):
                nb1.build(p1, check=False)
                cf1.compute(nb1, p1, x1, out=o1)
                cf1.backprop(nb1, p1, x1, g1)

        # one checked step each (row capacities, filter rows), and the two must agree
        nb.build(pos)
        for (nb1, _), (p1, _, _, _) in zip(ones, parts):
            nb1.build(p1)
        batched()
        gx_b, gp_b = cf.backprop(nb, pos, x, g)
        ref = out.clone()
        loop()
        gx_l = torch.cat([c.backprop(l, p1, x1, g1)[0] for (l, c), (p1, x1, g1, _) in zip(ones, parts)])
        torch.cuda.synchronize()
        err = float((out - ref).abs().max() / ref.abs().max()), float((gx_l - gx_b).abs().max() / gx_b.abs().max())
        assert max(err) < 1e-4, err
        reps = max(3, min(30, 2048 // B))
        rounds = [(timed(batched, reps), timed(loop, reps)) for _ in range(args.rounds)]       # interleaved: both see the same clocks
        tb, tl = np.array(rounds).T
        mb, ml = float(np.median(tb)), float(np.median(tl))
        print(f"  {B:4d} {N:6d} {nb.num_pairs():7d} {mb:12.1f} {tb.max() - tb.min():9.1f} {ml:12.1f} {tl.max() - tl.min():9.1f} {ml / mb:15.1f} "
              f"{mb / B:19.2f}")


if __name__ == "__main__":
    main()
