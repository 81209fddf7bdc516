"""The force-matching step through the twice-differentiable PME ops at 100 000 atoms (bench config 5's system:
random_box(density=0.1, seed=6), its list: cutoff 5.2, max_num_pairs 3.2 M, alpha 0.6 / A; reciprocal at 192^3, order 5), event-timed
and interleaved in one process:
  (a) forward + backward of the existing ops (pme_direct / pme_reciprocal), what every revision of the project can run;
  (b) the same through the _twice ops (the same kernels: the cost of the opt-in when nothing is differentiated twice);
  (c) the force-loss step  E -> grad(E, (x, q), create_graph=True) -> |F - F_ref|^2 .backward()  through the _twice ops,
per term and for both terms together; the list is built once outside the timing.  Under `rocprofv3 --kernel-trace --stats` the
kernel table of the same run gives the device time of each pass.

    python tools/pme_second_order_time.py [reps] [rounds]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import NNPOps  # noqa: E402,F401  (loads the torch ops)
from NNPOps.neighbors import getNeighborPairs  # noqa: E402
from nnpops_amd import workloads  # noqa: E402
from nnpops_amd.pme.pme import bspline_moduli  # noqa: E402

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ALPHA, COULOMB, CUTOFF, MAX_PAIRS, GRID, ORDER = 0.6, 138.935, 5.2, 3_200_000, 192, 5


def timed(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps          # us


def main():
    pos, _, box = workloads.random_box(100000, density=0.1, seed=6)
    n = len(pos)
    q = np.random.default_rng(6).normal(0, 0.4, n).astype(np.float32)
    tp = torch.tensor(pos, device=dev, requires_grad=True)
    tq = torch.tensor(q, device=dev, requires_grad=True)
    tb = torch.tensor(box, device=dev)
    ex = torch.zeros(n, 0, dtype=torch.int32, device=dev)
    f_ref = torch.randn(n, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    # positions that require grad: the list gets its transposed index, as in PME.compute_direct
    nb, d, r, found = getNeighborPairs(tp, CUTOFF, MAX_PAIRS, tb)
    d, r = d.detach(), r.detach()
    print(f"atoms {n}  slots {nb.shape[1]}  pairs {int(found)}")
    mods = [bspline_moduli(GRID, ORDER).to(dev)] * 3
    ops = torch.ops.pme

    def direct(op):
        return lambda: op(tp, tq, nb, d, r, ex, ALPHA, COULOMB)

    def recip(op):
        return lambda: op(tp, tq, tb, GRID, GRID, GRID, ORDER, ALPHA, COULOMB, *mods)

    def first_order(*energies):
        def run():
            torch.autograd.grad(sum(e() for e in energies), (tp, tq))
        return run

    def force_loss(*energies):
        def run():
            (dx,) = torch.autograd.grad(sum(e() for e in energies), tp, create_graph=True)
            torch.autograd.grad(((-dx - f_ref) ** 2).sum(), (tp, tq))
        return run

    cases = {
        "direct      fwd+bwd, existing op": first_order(direct(ops.pme_direct)),
        "direct      fwd+bwd, _twice op": first_order(direct(ops.pme_direct_twice)),
        "direct      force-loss step, _twice op": force_loss(direct(ops.pme_direct_twice)),
        "reciprocal  fwd+bwd, existing op": first_order(recip(ops.pme_reciprocal)),
        "reciprocal  fwd+bwd, _twice op": first_order(recip(ops.pme_reciprocal_twice)),
        "reciprocal  force-loss step, _twice op": force_loss(recip(ops.pme_reciprocal_twice)),
        "both terms  fwd+bwd, existing ops": first_order(direct(ops.pme_direct), recip(ops.pme_reciprocal)),
        "both terms  force-loss step, _twice ops": force_loss(direct(ops.pme_direct_twice), recip(ops.pme_reciprocal_twice)),
    }
    for fn in cases.values():                          # warm-up: FFT plans, allocator
        for _ in range(3):
            fn()
    times = {k: [] for k in cases}
    for _ in range(rounds):                            # interleaved: every round times every case
        for k, fn in cases.items():
            times[k].append(timed(fn, reps))
    for k, t in times.items():
        print(f"{k:44s} median {np.median(t):9.1f} us   rounds {' '.join(f'{x:.1f}' for x in t)}")


if __name__ == "__main__":
    main()
