"""getNeighborPairs second order at config 5's list (100 000 atoms, cutoff 5, density 0.1, 3 M slots), float32 and float64: the
first-order backward with and without the box gradient, the double-backward and box kernels alone (C ABI), and one whole force-loss
step (forward op, grad(E, x, create_graph=True), backward of |F - F_ref|^2).

    python tools/pairs_second_order_time.py [slots]
    python tools/pairs_second_order_time.py --profile {step,first-order} [dtype]   (a few calls only, for rocprofv3 --kernel-trace)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import NNPOps  # noqa: E402,F401
from NNPOps.neighbors import getNeighborPairs  # noqa: E402
from nnpops_amd import workloads  # noqa: E402
from nnpops_amd.capi import neighbor_pairs_box_backward, neighbor_pairs_double_backward  # noqa: E402

dev = torch.device("cuda:0")
N, CUTOFF = 100000, 5.0


def timed(fn, reps=50, warm=5):
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


def energy(dl, ds, theta):
    c = torch.tensor([0.3, -0.2, 0.9], dtype=dl.dtype, device=dl.device)
    return (theta[0] * torch.exp(-theta[1] * ds ** 2)).sum() + theta[2] * ((dl * c).sum(1) ** 2).sum()


def setup(dt, slots):
    pos, _, box = workloads.random_box(N, density=0.1, seed=3)
    tp = torch.tensor(pos, device=dev, dtype=dt).requires_grad_()
    tb = torch.tensor(box, device=dev, dtype=dt)
    theta = torch.tensor([1.3, 0.1, 0.2], dtype=dt, device=dev, requires_grad=True)
    f_ref = torch.randn(N, 3, dtype=dt, device=dev)
    return tp, tb, theta, f_ref


def force_loss_step(tp, tb, theta, f_ref, slots):
    nb, dl, ds, _ = getNeighborPairs(tp, CUTOFF, slots, tb)
    keep = nb[0] >= 0
    f = torch.autograd.grad(energy(dl[keep], ds[keep], theta), tp, create_graph=True)[0]
    ((f + f_ref) ** 2).sum().backward()


def main(slots):
    for dt in (torch.float32, torch.float64):
        tp, tb, theta, f_ref = setup(dt, slots)
        tbg = tb.clone().requires_grad_()
        nb, dl, ds, cnt = getNeighborPairs(tp, CUTOFF, slots, tb)
        used = int(cnt)
        gd, gs = torch.randn_like(dl), torch.randn_like(ds)
        nb2, dl2, ds2, _ = getNeighborPairs(tp, CUTOFF, slots, tbg)
        hx, hb = torch.randn(N, 3, dtype=dt, device=dev), torch.randn(3, 3, dtype=dt, device=dev)
        x, b = tp.detach(), tb.detach()
        esz = 4 if dt == torch.float32 else 8
        # bytes the double backward streams per used slot: neighbors 8, deltas 3, distances, grad_distances, the four outputs 8
        # (13 elements); unused slots: neighbors 8 + the outputs 8 elements.  The gathers of gg_positions (and of positions with gg_box)
        # are not counted: 18 neighbours per atom on average, they are served by the caches.
        streamed = used * (8 + 13 * esz) + (slots - used) * (8 + 8 * esz)
        print(dt, "pairs", used, "slots", slots)
        t = timed(lambda: torch.autograd.grad((dl, ds), tp, (gd, gs), retain_graph=True))
        print("   first-order backward, positions            %8.1f us" % t)
        t = timed(lambda: torch.autograd.grad((dl2, ds2), (tp, tbg), (gd, gs), retain_graph=True))
        print("   first-order backward, positions + box      %8.1f us" % t)
        t = timed(lambda: neighbor_pairs_box_backward(N, nb, x, b, dl, ds, gd, gs))
        print("   box backward kernels (C ABI)               %8.1f us" % t)
        t = timed(lambda: neighbor_pairs_double_backward(N, nb, dl, ds, gs, hx))
        print("   double backward, gg_positions (C ABI)      %8.1f us   %.2f TB/s streamed" % (t, streamed / t * 1e-6))
        t = timed(lambda: neighbor_pairs_double_backward(N, nb, dl, ds, gs, hx, hb, x, b))
        print("   double backward, gg_positions + gg_box     %8.1f us   %.2f TB/s streamed" % (t, streamed / t * 1e-6))
        t = timed(lambda: force_loss_step(tp, tb, theta, f_ref, slots), reps=20)
        print("   force-loss step (forward .. backward)      %8.1f us" % t)
        del nb, dl, ds, nb2, dl2, ds2
        torch.cuda.empty_cache()


def profile(what, dt):
    slots = 3000000
    tp, tb, theta, f_ref = setup(dt, slots)
    for _ in range(3):
        if what == "step":
            force_loss_step(tp, tb, theta, f_ref, slots)
        else:
            nb, dl, ds, _ = getNeighborPairs(tp, CUTOFF, slots, tb)
            keep = nb[0] >= 0
            (ds[keep] ** 2).sum().backward()
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--profile":
        profile(sys.argv[2], torch.float64 if len(sys.argv) > 3 and sys.argv[3] == "float64" else torch.float32)
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 3000000)
