"""getNeighborPairsFrames against the loop of single-system calls it replaces: forward, and forward + backward (positions, and the box
where there is one), of B frames -- 192-atom water boxes (an NPT trajectory: every frame in its own box) and 21-atom molecules
without a box.  Both sides run in this process, interleaved round by round; stream time, medians.

    python tools/pairs_frames_time.py [--frames 8 64 256] [--rounds 7]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import NNPOps  # noqa: E402,F401
from NNPOps.neighbors import frame_table, getNeighborPairs, getNeighborPairsFrames  # noqa: E402
from nnpops_amd import workloads  # noqa: E402

dev = torch.device("cuda:0")
CUTOFF = 5.0


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


def water_frames(B, seed=0):
    """B frames of a 64-water box as an NPT run leaves them -> positions [B * 192, 3], boxes [B, 3, 3]"""
    pos, _, box = workloads.water_box(64, seed=seed + 11)
    rng = np.random.default_rng(seed + 1)
    scale = rng.uniform(0.97, 1.04, B)
    ps = [((pos + rng.normal(0, 0.05, pos.shape)) * s).astype(np.float32) for s in scale]
    return np.concatenate(ps), np.stack([(box * np.float32(s)).astype(np.float32) for s in scale])


def molecules(B, seed=0):
    """B conformers of a 21-atom molecule (atoms 1.2 A and more apart in a 7 A cube), no box"""
    rng = np.random.default_rng(seed + 5)
    atoms = []
    while len(atoms) < 21:
        p = rng.uniform(0, 7, 3)
        if all(np.linalg.norm(p - q) > 1.2 for q in atoms):
            atoms.append(p)
    base = np.array(atoms)
    return np.concatenate([(base + rng.normal(0, 0.05, base.shape)).astype(np.float32) for _ in range(B)]), None


def energy(dl, ds):
    return (1.3 * torch.exp(-0.1 * ds ** 2)).sum() + 0.2 * ((0.3 * dl[:, 0] - 0.2 * dl[:, 1] + 0.9 * dl[:, 2]) ** 2).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    print(f"getNeighborPairsFrames: float32, cutoff {CUTOFF}, compacted lists; stream time, medians of {args.rounds} interleaved rounds "
          "(spread = max - min)")
    print(f"  {'frames of':>14s} {'B':>4s} {'pairs':>8s} {'step':>18s} {'batched us':>11s} {'(spread)':>9s} {'loop us':>10s} {'(spread)':>9s} "
          f"{'loop / batched':>15s}")
    for name, make, n in (("192-atom water", water_frames, 192), ("21-atom molecule", molecules, 21)):
        for B in args.frames:
            host_pos, host_boxes = make(B)
            pos = torch.tensor(host_pos, device=dev).requires_grad_()
            boxes = None if host_boxes is None else torch.tensor(host_boxes, device=dev).requires_grad_()
            table = frame_table([m * n for m in range(B + 1)], dev)
            with torch.no_grad():
                counts = [int(getNeighborPairs(pos[m * n:(m + 1) * n], CUTOFF, -1, None if boxes is None else boxes[m])[3]) for m in range(B)]
            total, slots1 = sum(counts), max(counts) + 16
            parts = [(pos.detach()[m * n:(m + 1) * n].clone().requires_grad_(),
                      None if boxes is None else boxes.detach()[m].clone().requires_grad_()) for m in range(B)]

            def batched(backward):
                with torch.set_grad_enabled(backward):
                    nb, dl, ds, _ = getNeighborPairsFrames(pos, CUTOFF, table, total, boxes)
                    if backward:
                        return torch.autograd.grad(energy(dl, ds), [pos] if boxes is None else [pos, boxes])
                    return dl, ds

            def loop(backward):
                res = []
                with torch.set_grad_enabled(backward):
                    for (p1, b1), c in zip(parts, counts):
                        nb, dl, ds, _ = getNeighborPairs(p1, CUTOFF, slots1, b1)
                        if backward:
                            res.append(torch.autograd.grad(energy(dl[:c], ds[:c]), [p1] if b1 is None else [p1, b1]))
                        else:
                            res.append((dl, ds))
                return res

            # the two sides must agree before they are timed
            gb, gl = batched(True), loop(True)
            for k in range(len(gb)):
                joined = (torch.cat if k == 0 else torch.stack)([g[k] for g in gl])
                assert float((joined - gb[k]).abs().max()) <= 1e-4 * float(gb[k].abs().max())
            reps_b, reps_l = max(20, min(200, 4096 // B)), max(3, min(30, 512 // B))
            for backward in (False, True):
                rounds = [(timed(lambda: batched(backward), reps_b), timed(lambda: loop(backward), reps_l)) for _ in range(args.rounds)]
                tb, tl = np.array(rounds).T
                mb, ml = float(np.median(tb)), float(np.median(tl))
                print(f"  {name:>14s} {B:4d} {total:8d} {'forward + backward' if backward else 'forward':>18s} {mb:11.1f} "
                      f"{tb.max() - tb.min():9.1f} {ml:10.1f} {tl.max() - tl.min():9.1f} {ml / mb:15.1f}", flush=True)


if __name__ == "__main__":
    main()
