"""Host time of a CFConv module call: wall clock per forward + backward (and per force-loss step of the recorded flavours) at a shape
where the host dominates (90 atoms, W = 16, G = 8), the device drained at the end of each bracket of 300 calls; rows interleaved,
medians of 15 rounds.  What a change of the torch binding's autograd nodes can move, and what the stream-time rows of the other
cfconv_*_time.py tools cannot see.

    python tools/cfconv_binding_host_time.py [ROOT]        ROOT: another checkout, built, to time instead of this one"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nnpops_amd  # noqa: E402
from nnpops_amd import workloads  # noqa: E402
from NNPOps.CFConv import CFConv  # noqa: E402
from NNPOps.CFConvNeighbors import CFConvNeighbors  # noqa: E402

assert os.path.abspath(nnpops_amd.__file__).startswith(ROOT), nnpops_amd.__file__
dev = "cuda:0"
W, G, n = 16, 8, 90


def walled(fn, reps=300, warm=30):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def main():
    pos = torch.tensor(workloads.conformer(n, seed=7)[0], device=dev)
    rng = np.random.default_rng(1)
    t = lambda *s: torch.tensor(0.2 * rng.standard_normal(s).astype(np.float32))
    w = (t(G, W), t(W), t(W, W), t(W))
    x, g = t(n, W).to(dev), t(n, W).to(dev)
    nb = CFConvNeighbors(5.0)
    nb.build(pos)
    rows = []
    for name, kw in (("default", {}), ("twice_differentiable", dict(twice_differentiable=True)), ("trainable", dict(trainable=True)),
                     ("force_trainable", dict(force_trainable=True))):
        conv = CFConv(0.4, "ssp", *w, **kw).to(dev)
        p, xx = pos.clone().requires_grad_(True), x.clone().requires_grad_(True)
        leaves = [p, xx, *conv.parameters()]

        def step(conv=conv, p=p, xx=xx, leaves=leaves):
            torch.autograd.grad((conv(nb, p, xx) * g).sum(), leaves)

        def force_step(conv=conv, p=p, xx=xx, leaves=leaves):
            E = (conv(nb, p, xx) * g).sum()
            F, = torch.autograd.grad(E, p, create_graph=True)
            torch.autograd.grad((F ** 2).sum(), leaves)

        rows.append((f"{name}: forward + backward", step))
        if "twice_differentiable" in kw or "force_trainable" in kw:
            rows.append((f"{name}: force-loss step", force_step))
    rounds = [[walled(fn) for _, fn in rows] for _ in range(15)]
    print(f"host time, {n} atoms W={W} G={G}, wall clock us per call, medians of 15 interleaved rounds (spread = max - min), root {ROOT}:")
    for k, (name, _) in enumerate(rows):
        q = [r[k] for r in rounds]
        print(f"  {name:45s} {np.median(q):9.1f} us  (min {min(q):.1f}, spread {max(q) - min(q):.1f})")


if __name__ == "__main__":
    main()
