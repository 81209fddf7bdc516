"""Reciprocal-space PME at 100 000 atoms (bench config 5's system: random_box(density=0.1, seed=6), alpha 0.6 / A): event-timed
phases of the forward (spread = spline/bin + sort + gather, rfftn, convolve) and backward (irfftn, interpolate) at 96^3, 128^3 and
192^3, orders 4 and 5, with the bytes each phase must move at least; the kernels inside the spread split by torch.profiler; and, in
this tool only, a float-atomic scatter spread of the same data (torch index_add_) for comparison.

    python tools/pme_recip_time.py [reps]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import capi, workloads
from nnpops_amd.pme.pme import bspline_moduli

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ALPHA, COULOMB = 0.6, 138.935


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


def splines_torch(pos, box, K, order):
    """base index and weights of every atom, computed with torch (cubic box): the input of the atomic-scatter comparison."""
    frac = torch.remainder(pos / box.diagonal(), 1.0) * K
    base = frac.floor().long() % K
    dr = frac - frac.floor()
    w = [1 - dr, dr] + [torch.zeros_like(dr) for _ in range(order - 2)]
    for n in range(3, order + 1):
        div = 1.0 / (n - 1)
        nw = [None] * order
        nw[n - 1] = div * dr * w[n - 2]
        for k in range(1, n - 1):
            nw[n - k - 1] = div * ((dr + k) * w[n - k - 2] + (n - k - dr) * w[n - k - 1])
        nw[0] = div * (1 - dr) * w[0]
        w = [x if x is not None else torch.zeros_like(dr) for x in nw]
    return base, torch.stack(w, 1)                   # [N, 3], [N, order, 3]


def main():
    pos, _, box = workloads.random_box(100000, density=0.1, seed=6)
    n = len(pos)
    rng = np.random.default_rng(6)
    tp = torch.tensor(pos, device=dev)
    tq = torch.tensor(rng.normal(0, 0.4, n).astype(np.float32), device=dev)
    tb = torch.tensor(box, device=dev)
    L = capi.lib()
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = capi._ptr
    print(f"# {n} atoms, box {box[0, 0]:.2f} A, alpha {ALPHA}; times in us (event-timed means over {reps} calls)")
    print("grid order | spread  rfftn  convolve | irfftn  interp | fwd    bwd    | atomic-scatter spread | min MB: spread fft conv interp")
    for K in (96, 128, 192):
        for order in (4, 5):
            mods = [bspline_moduli(K, order).to(dev)] * 3
            ws = torch.empty((int(L.nnpops_pme_reciprocal_workspace_bytes(n, K, K, K, order)),), dtype=torch.uint8, device=dev)
            real = torch.empty((K, K, K), dtype=torch.float32, device=dev)
            energy = torch.empty((1,), dtype=torch.float32, device=dev)
            pd = torch.empty((n, 3), dtype=torch.float32, device=dev)
            cd = torch.empty((n,), dtype=torch.float32, device=dev)
            state = {}

            def spread():
                capi._check(L.nnpops_pme_reciprocal_spread(n, K, K, K, order, ptr(tp), ptr(tq), ptr(tb), COULOMB, ptr(real), ptr(ws), s))

            def rfft():
                state["recip"] = torch.fft.rfftn(real)

            def convolve():
                r = state["recip"]
                capi._check(L.nnpops_pme_reciprocal_convolve(n, K, K, K, order, ptr(tb), ALPHA, ptr(mods[0]), ptr(mods[1]), ptr(mods[2]),
                                                             ptr(r), ptr(energy), ptr(ws), s))

            def irfft():
                state["grid"] = torch.fft.irfftn(state["recip"], s=(K, K, K), norm="forward")

            def interp():
                capi._check(L.nnpops_pme_reciprocal_interpolate(n, K, K, K, order, ptr(tq), ptr(tb), COULOMB, ptr(state["grid"]), ptr(pd),
                                                                ptr(cd), ptr(ws), s))

            spread(); rfft(); convolve(); irfft(); interp()
            t = {name: timed(fn) for name, fn in (("spread", spread), ("rfftn", rfft), ("convolve", convolve), ("irfftn", irfft),
                                                   ("interp", interp))}
            # float-atomic scatter of the same contributions (index_add_ issues one float atomic per (atom, stencil point))
            base, w = splines_torch(tp, tb, K, order)
            o = torch.arange(order, device=dev)
            ix = (base[:, 0, None] + o) % K
            iy = (base[:, 1, None] + o) % K
            iz = (base[:, 2, None] + o) % K
            idx = ((ix[:, :, None, None] * K + iy[:, None, :, None]) * K + iz[:, None, None, :]).reshape(-1)
            val = (tq[:, None, None, None] * COULOMB ** 0.5 * w[:, :, None, None, 0] * w[:, None, :, None, 1]
                   * w[:, None, None, :, 2]).reshape(-1)
            flat = torch.empty(K * K * K, dtype=torch.float32, device=dev)

            def atomic():
                flat.zero_()
                flat.index_add_(0, idx, val)

            t_atomic = timed(atomic)
            err = float((flat.view(K, K, K) - real).abs().max() / real.abs().max())
            cplx = K * K * (K // 2 + 1) * 8
            mb = (4 * K ** 3 + n * (12 + 4 + 16 + 2 * 12 * order + 16)) / 1e6, (4 * K ** 3 + cplx) / 1e6, 2 * cplx / 1e6, \
                (4 * K ** 3 + n * (4 + 16 + 2 * 12 * order + 16)) / 1e6
            fwd = t["spread"] + t["rfftn"] + t["convolve"]
            bwd = t["irfftn"] + t["interp"]
            print(f"{K:4d} {order:5d} | {t['spread']:6.1f} {t['rfftn']:6.1f} {t['convolve']:8.1f} | {t['irfftn']:6.1f} {t['interp']:7.1f} | "
                  f"{fwd:6.1f} {bwd:6.1f} | {t_atomic:8.1f} (grid diff {err:.1e}) | "
                  + " ".join(f"{m:.1f}" for m in mb)
                  + f"  -> GB/s spread {mb[0] * 1e3 / t['spread']:.0f} conv {mb[2] * 1e3 / t['convolve']:.0f} "
                    f"interp {mb[3] * 1e3 / t['interp']:.0f}")
            if K == 192 and order == 5:
                try:
                    from torch.profiler import ProfilerActivity, profile
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        for _ in range(5):
                            spread()
                        torch.cuda.synchronize()
                    print("# kernels of the spread at 192^3, order 5 (mean us per call):")
                    for ev in prof.key_averages():
                        if "pme_recip" in ev.key:
                            dt = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                            print(f"#   {ev.key[:60]:60s} {dt / max(ev.count, 1):8.1f}")
                except Exception as exc:                     # (the profiler is a convenience: the phase times above stand alone)
                    print(f"# profiler unavailable: {exc}")


if __name__ == "__main__":
    main()
