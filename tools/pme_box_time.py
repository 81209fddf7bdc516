"""PME with and without the box gradient at 100 000 atoms (bench config 5's system: random_box(density=0.1, seed=6), its list:
cutoff 5.2, max_num_pairs 3.2 M, alpha 0.6 / A; reciprocal at 192^3, order 5): event-timed means of the direct term (pme_direct
against pme_direct_box, forward + backward, the list built once outside the timing) and of the reciprocal term (forward + backward
with the box a constant or requiring grad), and the new passes alone through the C ABI.

    python tools/pme_box_time.py [reps]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import NNPOps  # noqa: E402,F401  (loads the torch ops)
from NNPOps.neighbors import getNeighborPairs  # noqa: E402
from nnpops_amd import capi, workloads  # noqa: E402
from nnpops_amd.pme.pme import bspline_moduli  # noqa: E402

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ALPHA, COULOMB, CUTOFF, MAX_PAIRS, GRID, ORDER = 0.6, 138.935, 5.2, 3_200_000, 192, 5


def timed(fn, reps=reps, warm=3):
    for _ in range(warm):
        fn()
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
    q = np.random.default_rng(6).normal(0, 0.4, len(pos)).astype(np.float32)
    tp = torch.tensor(pos, device=dev, requires_grad=True)
    tq = torch.tensor(q, device=dev, requires_grad=True)
    tb = torch.tensor(box, device=dev, requires_grad=True)
    ex = torch.zeros(len(pos), 0, dtype=torch.int32, device=dev)
    # positions that require grad: the list gets its transposed index (the pair-index cache), as in PME.compute_direct, so the
    # direct rows time the indexed path training takes; deltas and distances detached so that only PME's own work is timed
    nb, d, r, found = getNeighborPairs(tp, CUTOFF, MAX_PAIRS, tb.detach())
    d, r = d.detach(), r.detach()
    print(f"atoms {len(pos)}  slots {nb.shape[1]}  pairs {int(found)}")
    mods = [bspline_moduli(GRID, ORDER).to(dev)] * 3
    rows = {}

    def direct(box_grad):
        def run():
            if box_grad:
                e = torch.ops.pme.pme_direct_box(tp, tq, nb, d, r, ex, tb, ALPHA, COULOMB)
                torch.autograd.grad(e, (tp, tq, tb))
            else:
                e = torch.ops.pme.pme_direct(tp, tq, nb, d, r, ex, ALPHA, COULOMB)
                torch.autograd.grad(e, (tp, tq))
        return run

    def recip(box_grad):
        b = tb if box_grad else tb.detach()

        def run():
            e = torch.ops.pme.pme_reciprocal(tp, tq, b, GRID, GRID, GRID, ORDER, ALPHA, COULOMB, *mods)
            torch.autograd.grad(e, (tp, tq, tb) if box_grad else (tp, tq))
        return run

    rows["direct fwd+bwd, indexed list, no box gradient"] = timed(direct(False))
    rows["direct fwd+bwd, indexed list, box gradient"] = timed(direct(True))
    rows["reciprocal fwd+bwd 192^3 o5, no box gradient"] = timed(recip(False))
    rows["reciprocal fwd+bwd 192^3 o5, box gradient"] = timed(recip(True))

    # the new passes alone, through the C entries with preallocated buffers
    pd, bd = tp.detach(), tb.detach()
    L = capi.lib()
    n = len(pos)
    s = capi._stream_ptr(dev)
    nb32 = nb.to(torch.int32).contiguous()
    dws = torch.empty((int(L.nnpops_pme_direct_box_workspace_bytes(nb.shape[1])) // 8,), dtype=torch.float64, device=dev)
    dgb = torch.empty((3, 3), device=dev)
    rows["nnpops_pme_direct_box alone (box pass + finish)"] = timed(
        lambda: capi._check(L.nnpops_pme_direct_box(n, nb.shape[1], 0, capi._ptr(pd), capi._ptr(tq.detach()), capi._ptr(nb32), capi._ptr(d),
                                                    capi._ptr(r), None, capi._ptr(bd), ALPHA, COULOMB, capi._ptr(dgb), capi._ptr(dws), s)))
    ws = torch.empty((int(L.nnpops_pme_reciprocal_workspace_bytes(n, GRID, GRID, GRID, ORDER)),), dtype=torch.uint8, device=dev)
    bws = torch.empty((int(L.nnpops_pme_reciprocal_box_workspace_bytes(n, GRID, GRID, GRID, ORDER)),), dtype=torch.uint8, device=dev)
    real = torch.empty((GRID, GRID, GRID), device=dev)
    energy = torch.empty((1,), device=dev)
    gbox = torch.empty((3, 3), device=dev)
    capi._check(L.nnpops_pme_reciprocal_spread(n, GRID, GRID, GRID, ORDER, capi._ptr(pd), capi._ptr(tq.detach()), capi._ptr(bd),
                                               COULOMB, capi._ptr(real), capi._ptr(ws), s))
    recip_grid = torch.fft.rfftn(real).contiguous()
    fresh = recip_grid.clone()

    def convolve(box_grad):
        def run():
            recip_grid.copy_(fresh)
            if box_grad:
                capi._check(L.nnpops_pme_reciprocal_convolve_box(n, GRID, GRID, GRID, ORDER, capi._ptr(bd), ALPHA, *(capi._ptr(m) for m in mods),
                                                                 capi._ptr(recip_grid), capi._ptr(energy), capi._ptr(ws), capi._ptr(bws), s))
            else:
                capi._check(L.nnpops_pme_reciprocal_convolve(n, GRID, GRID, GRID, ORDER, capi._ptr(bd), ALPHA, *(capi._ptr(m) for m in mods),
                                                             capi._ptr(recip_grid), capi._ptr(energy), capi._ptr(ws), s))
        return run
    copy = timed(lambda: recip_grid.copy_(fresh))
    rows["convolve (no Pi), copy of the grid subtracted"] = timed(convolve(False)) - copy
    rows["convolve_box (with Pi), copy of the grid subtracted"] = timed(convolve(True)) - copy
    pos_deriv = torch.randn((n, 3), device=dev)
    rows["nnpops_pme_reciprocal_box_gradient (X pass + finish)"] = timed(
        lambda: capi._check(L.nnpops_pme_reciprocal_box_gradient(n, GRID, GRID, GRID, ORDER, capi._ptr(pd), capi._ptr(bd), capi._ptr(pos_deriv),
                                                                 capi._ptr(gbox), capi._ptr(bws), s)))
    for k, v in rows.items():
        print(f"{k:60s} {v:9.1f} us")


if __name__ == "__main__":
    main()
