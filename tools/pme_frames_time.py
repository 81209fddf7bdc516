"""PME over frames against the loop of single-frame calls it replaces: direct and reciprocal term, forward + backward (positions and
charges), of B frames of a 192-atom water box, every frame in its own box (an NPT trajectory).  Both sides run in this process,
interleaved round by round; stream time, medians.  The repository's benchmarks hold no PME configuration for such a box: cutoff 5 A,
alpha 0.6 / A, a 24^3 grid, order 5.

    python tools/pme_frames_time.py [--frames 8 64 256] [--rounds 7] [--batched-only]      (--batched-only: for a kernel profile)
    python tools/pme_frames_time.py --box ...       the box gradient as well (box_gradient=True) against the loop of single-frame calls
                                                    with a box that requires a gradient, and against the batch without box gradient
    python tools/pme_frames_time.py --twice ...     the force-loss step E -> grad(E, (x, q), create_graph=True) -> |F - F_ref|^2.backward()
                                                    (twice_differentiable=True per call) against the loop of single-frame steps on a
                                                    PME(..., twice_differentiable=True) object
    python tools/pme_frames_time.py --transform lds [--box] [--grid 24] [--batched-only]
                                                    the reciprocal term with transform="lds" (pme_frames_fft.hip) against the default
                                                    transform="torch", forward + backward; --batched-only runs "lds" alone, and with
                                                    --transform torch the default alone (for kernel profiles)"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import NNPOps  # noqa: E402,F401
from NNPOps.pme import PME  # noqa: E402
from nnpops_amd import workloads  # noqa: E402

dev = torch.device("cuda:0")
CUTOFF, ALPHA, COULOMB, GRID, ORDER, N = 5.0, 0.6, 332.0637, 24, 5, 192


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
    """B frames of a 64-water box as an NPT run leaves them -> positions [B * 192, 3], charges, boxes [B, 3, 3], exclusions (a water's
    atoms exclude each other)"""
    pos, species, box = workloads.water_box(64, seed=seed + 11)
    rng = np.random.default_rng(seed + 1)
    scale = rng.uniform(0.97, 1.04, B)
    ps = [((pos + rng.normal(0, 0.05, pos.shape)) * s).astype(np.float32) for s in scale]
    q1 = np.where(np.asarray(species) == np.max(species), -0.834, 0.417).astype(np.float32)
    atoms = np.arange(B * N)
    mol = atoms - atoms % 3
    excl = np.stack([mol + (atoms % 3 + 1) % 3, mol + (atoms % 3 + 2) % 3], 1).astype(np.int32)
    return np.concatenate(ps), np.tile(q1, B), np.stack([(box * np.float32(s)).astype(np.float32) for s in scale]), excl


def force_loss(energy, x, c, f_ref):
    """the gradients of |F - F_ref|^2 with respect to positions and charges, F = -dE/dx recorded"""
    dx = torch.autograd.grad(energy, (x, c), create_graph=True)[0]
    return torch.autograd.grad(((-dx - f_ref) ** 2).sum(), (x, c))


def transforms(args):
    """transform="lds" against transform="torch": the reciprocal term's forward + backward, with the box gradient under --box"""
    G = args.grid
    print(f"PME reciprocal over frames, transform lds against torch: {N}-atom water boxes, alpha {ALPHA}, grid {G}^3, order {ORDER}; forward + "
          f"backward{' with the box gradient' if args.box else ''}, stream time, medians of {args.rounds} interleaved rounds (spread = max - min)")
    print(f"  {'B':>4s} {'lds us':>9s} {'(spread)':>9s} {'torch us':>9s} {'(spread)':>9s} {'torch / lds':>12s}")
    for B in args.frames:
        host_pos, host_q, host_boxes, excl = water_frames(B)
        offsets = [m * N for m in range(B + 1)]
        pos, q = torch.tensor(host_pos, device=dev).requires_grad_(), torch.tensor(host_q, device=dev).requires_grad_()
        boxes = torch.tensor(host_boxes, device=dev).requires_grad_(args.box)
        pme = PME(G, G, G, ORDER, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True)

        def step(transform):
            e = pme.compute_reciprocal_frames(pos, q, boxes, offsets, box_gradient=args.box, transform=transform)
            return torch.autograd.grad(e.sum(), (pos, q, boxes) if args.box else (pos, q))
        reps = max(20, min(200, 4096 // B))
        if args.batched_only:
            timed(lambda: step(args.transform), reps)
            continue
        for a, b in zip(step("lds"), step("torch")):                     # the two routes must agree before they are timed
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
        tl, tt = np.array([(timed(lambda: step("lds"), reps), timed(lambda: step("torch"), reps)) for _ in range(args.rounds)]).T
        ml, mt = float(np.median(tl)), float(np.median(tt))
        print(f"  {B:4d} {ml:9.1f} {tl.max() - tl.min():9.1f} {mt:9.1f} {tt.max() - tt.min():9.1f} {mt / ml:12.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batched-only", action="store_true")
    ap.add_argument("--box", action="store_true")
    ap.add_argument("--twice", action="store_true")
    ap.add_argument("--transform", choices=["torch", "lds"], default=None)
    ap.add_argument("--grid", type=int, default=GRID)
    args = ap.parse_args()
    if args.transform:
        return transforms(args)
    assert not (args.box and args.twice), "--box and --twice are separate measurements"
    what = "force-loss step" if args.twice else "forward + backward"
    print(f"PME over frames: {N}-atom water boxes, cutoff {CUTOFF}, alpha {ALPHA}, grid {GRID}^3, order {ORDER}; {what}, stream time, "
          f"medians of {args.rounds} interleaved rounds (spread = max - min)")
    print(f"  {'B':>4s} {'term':>11s} {'batched us':>11s} {'(spread)':>9s} {'loop us':>10s} {'(spread)':>9s} {'loop / batched':>15s}" +
          (f" {'no box us':>10s} {'(spread)':>9s} {'batched / no box':>17s}" if args.box else ""))
    for B in args.frames:
        host_pos, host_q, host_boxes, excl = water_frames(B)
        offsets = [m * N for m in range(B + 1)]
        pos, q = torch.tensor(host_pos, device=dev).requires_grad_(), torch.tensor(host_q, device=dev).requires_grad_()
        boxes = torch.tensor(host_boxes, device=dev)
        gboxes = boxes.clone().requires_grad_()                  # --box: the batch's boxes as a leaf
        pme = PME(GRID, GRID, GRID, ORDER, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True)
        one = PME(GRID, GRID, GRID, ORDER, ALPHA, COULOMB, torch.tensor(excl[:N]), reciprocal=True, twice_differentiable=args.twice)
        f_ref = torch.randn(B * N, 3, device=dev, generator=torch.Generator(dev).manual_seed(B))
        parts = [(pos.detach()[m * N:(m + 1) * N].clone().requires_grad_(), q.detach()[m * N:(m + 1) * N].clone().requires_grad_(),
                  boxes[m].clone().requires_grad_(args.box)) for m in range(B)]
        terms = {
            "direct": (lambda: pme.compute_direct_frames(pos, q, CUTOFF, boxes, offsets, twice_differentiable=args.twice),
                       lambda p, c, b: one.compute_direct(p, c, CUTOFF, b)),
            "reciprocal": (lambda: pme.compute_reciprocal_frames(pos, q, boxes, offsets, twice_differentiable=args.twice),
                           lambda p, c, b: one.compute_reciprocal(p, c, b)),
        }
        box_terms = {
            "direct": lambda: pme.compute_direct_frames(pos, q, CUTOFF, gboxes, offsets, box_gradient=True),
            "reciprocal": lambda: pme.compute_reciprocal_frames(pos, q, gboxes, offsets, box_gradient=True),
        }
        for name, (frames_energy, single_energy) in terms.items():
            def no_box():
                return torch.autograd.grad(frames_energy().sum(), (pos, q))

            def with_box():
                return torch.autograd.grad(box_terms[name]().sum(), (pos, q, gboxes))

            def loop():
                if args.twice:
                    return [force_loss(single_energy(p, c, b), p, c, f_ref[m * N:(m + 1) * N]) for m, (p, c, b) in enumerate(parts)]
                return [torch.autograd.grad(single_energy(p, c, b), (p, c, b) if args.box else (p, c)) for p, c, b in parts]

            def twice():
                return force_loss(frames_energy().sum(), pos, q, f_ref)

            batched = twice if args.twice else with_box if args.box else no_box
            gb, gl = batched(), loop()                      # the two sides must agree before they are timed
            for k in range(len(gb)):
                joined = (torch.stack if k == 2 else torch.cat)([g[k] for g in gl])
                assert float((joined - gb[k]).abs().max()) <= 1e-4 * float(gb[k].abs().max()), (name, k)
            reps_b, reps_l = max(20, min(200, 4096 // B)), max(3, min(30, 512 // B))
            if args.batched_only:
                timed(batched, reps_b)
                continue
            rounds = [(timed(batched, reps_b), timed(loop, reps_l), timed(no_box, reps_b) if args.box else 0.0) for _ in range(args.rounds)]
            tb, tl, tn = np.array(rounds).T
            mb, ml, mn = float(np.median(tb)), float(np.median(tl)), float(np.median(tn))
            print(f"  {B:4d} {name:>11s} {mb:11.1f} {tb.max() - tb.min():9.1f} {ml:10.1f} {tl.max() - tl.min():9.1f} {ml / mb:15.1f}" +
                  (f" {mn:10.1f} {tn.max() - tn.min():9.1f} {mb / mn:17.2f}" if args.box else ""), flush=True)


if __name__ == "__main__":
    main()
