"""One CFConv step over a batch of periodic frames against the loop of single-frame steps it replaces: B frames of a 192-atom water
box (64 waters), every frame in its own box, W = 128, G = 50, cutoff 5 A.

    batched   one periodic list with frame offsets (nnpops_cfconv_neighbors_set_frames), one convolution of B * 192 atoms, boxes
              [B, 3, 3]: build + compute + backprop (or backprop_box) = one launch sequence for the whole batch
    loop      B single-system periodic lists and B convolutions of 192 atoms (the same weights), the same three calls B times --
              the path a minibatch of an NPT trajectory took before frames

Both go through the C ABI with no host synchronisation inside a step (build without check(), as a captured step runs it), so a
step is launches on one stream: the figure is stream time per step, event-timed, every shape warmed, the two cases interleaved round
by round in one process, medians of the rounds with their spread (max - min).  Each B is timed without and with the box gradient.
Before timing, the two paths are compared on the same inputs (output, gradients and the box gradient of every frame).  Prints both
columns and their ratio; asserts nothing about speed.

    python tools/cfconv_frames_time.py [--frames 8 64 256] [--waters 64] [--rounds 7]"""
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


def trajectory(B, waters, seed=0):
    """B frames of one water box as an NPT run leaves them: positions jittered by 0.05 A, positions and box scaled by 0.97 ... 1.04
    -> (positions [B * n, 3], boxes [B, 3, 3])"""
    pos, _, box = workloads.water_box(waters, seed=seed + 11)
    rng = np.random.default_rng(seed + 1)
    ps, bs = [], []
    for _ in range(B):
        s = rng.uniform(0.97, 1.04)
        ps.append(((pos + rng.normal(0, 0.05, pos.shape)) * s).astype(np.float32))
        bs.append((box * np.float32(s)).astype(np.float32))
    return np.concatenate(ps), np.stack(bs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--waters", type=int, default=64)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--gaussians", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, W, G = 3 * args.waters, args.width, args.gaussians
    rng = np.random.default_rng(4)
    w = ((0.1 * rng.standard_normal((W, G))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32),
         (0.1 * rng.standard_normal((W, W))).astype(np.float32), (0.1 * rng.standard_normal(W)).astype(np.float32))
    print(f"cfconv frames: {n}-atom water boxes, W={W} G={G} cutoff {CUTOFF}; build + compute + backprop per step, stream time, "
          f"medians of {args.rounds} interleaved rounds (spread = max - min)")
    print(f"  {'B':>4s} {'atoms':>6s} {'pairs':>8s} {'box grad':>8s} {'batched us':>12s} {'(spread)':>9s} {'loop us':>12s} {'(spread)':>9s} "
          f"{'loop / batched':>15s} {'batched us / frame':>19s}")
    for B in args.frames:
        N = B * n
        host_pos, host_boxes = trajectory(B, args.waters)
        pos, boxes = torch.tensor(host_pos, device=dev), torch.tensor(host_boxes, device=dev)
        x = torch.tensor(rng.standard_normal((N, W)).astype(np.float32), device=dev)
        g = torch.tensor(rng.standard_normal((N, W)).astype(np.float32), device=dev)
        nb, cf = capi.CFConvNeighbors(N, CUTOFF, True), capi.CFConv(N, W, G, CUTOFF, SIGMA, "ssp", *w, periodic=True)
        nb.set_frames(np.arange(B + 1) * n)
        out = torch.empty_like(x)
        ones = [(capi.CFConvNeighbors(n, CUTOFF, True), capi.CFConv(n, W, G, CUTOFF, SIGMA, "ssp", *w, periodic=True)) for _ in range(B)]
        parts = [tuple(t[m * n:(m + 1) * n] for t in (pos, x, g, out)) + (boxes[m],) for m in range(B)]      # (contiguous blocks: views)

        def batched(box_grad):
            nb.build(pos, boxes, check=False)
            cf.compute(nb, pos, x, boxes, out=out)
            return cf.backprop_box(nb, pos, x, g, boxes) if box_grad else cf.backprop(nb, pos, x, g, boxes)

        def loop(box_grad):
            res = []
            for (nb1, cf1), (p1, x1, g1, o1, b1) in zip(ones, parts):
                nb1.build(p1, b1, check=False)
                cf1.compute(nb1, p1, x1, b1, out=o1)
                res.append(cf1.backprop_box(nb1, p1, x1, g1, b1) if box_grad else cf1.backprop(nb1, p1, x1, g1, b1))
            return res

        # one checked step each (row capacities, filter rows, the scratch of the box pass), and the two must agree
        nb.build(pos, boxes)
        for (nb1, _), (p1, _, _, _, b1) in zip(ones, parts):
            nb1.build(p1, b1)
        gx_b, gp_b, gb_b = batched(True)
        ref = out.clone()
        per_frame = loop(True)
        torch.cuda.synchronize()
        gx_l, gp_l, gb_l = (torch.cat([r[k] for r in per_frame]) if k < 2 else torch.stack([r[k] for r in per_frame]) for k in range(3))
        rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
        err = (rel(out, ref), rel(gx_l, gx_b), rel(gp_l, gp_b), rel(gb_l, gb_b))
        assert max(err) < 1e-4, err
        pairs = nb.num_pairs()
        reps_b, reps_l = max(20, min(200, 4096 // B)), max(3, min(30, 512 // B))
        for box_grad in (False, True):
            rounds = [(timed(lambda: batched(box_grad), reps_b), timed(lambda: loop(box_grad), reps_l)) for _ in range(args.rounds)]
            tb, tl = np.array(rounds).T
            mb, ml = float(np.median(tb)), float(np.median(tl))
            print(f"  {B:4d} {N:6d} {pairs:8d} {'yes' if box_grad else 'no':>8s} {mb:12.1f} {tb.max() - tb.min():9.1f} {ml:12.1f} "
                  f"{tl.max() - tl.min():9.1f} {ml / mb:15.1f} {mb / B:19.2f}", flush=True)


if __name__ == "__main__":
    main()
