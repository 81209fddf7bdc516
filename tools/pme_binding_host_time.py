"""Host time of a PME op call: wall clock per forward + backward (and per force-loss step of a _twice op) at shapes where the host
dominates (3 frames of 5, 9 and 7 atoms, 24 atoms for the single system, grid 6 x 8 x 10, order 5: those of
tests/test_pme_binding_nodes_gpu.py), the device drained at the end of each bracket of 200 calls; rows interleaved, medians of 15
rounds.  What a change of the torch binding's autograd nodes can move, and what the stream-time rows of the other pme_*_time.py tools
cannot see.

    python tools/pme_binding_host_time.py [ROOT]        ROOT: another checkout, built, to time instead of this one"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nnpops_amd  # noqa: E402
import NNPOps  # noqa: E402,F401
from NNPOps.pme import PME  # noqa: E402

assert os.path.abspath(nnpops_amd.__file__).startswith(ROOT), nnpops_amd.__file__
dev = "cuda:0"
GRID, ORDER, ALPHA, COULOMB, CUTOFF, L = (6, 8, 10), 5, 3.5, 138.935, 1.0, 2.4
SIZES, ATOMS = (5, 9, 7), 24


def walled(fn, reps=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def system(n, rng):
    box = np.array([[L, 0, 0], [0.3 * L, 1.05 * L, 0], [-0.25 * L, 0.2 * L, 0.95 * L]], np.float32)
    q = rng.normal(0, 0.5, n)
    return (rng.random((n, 3)) @ box).astype(np.float32), (q - q.mean()).astype(np.float32), box


def main():
    rng = np.random.default_rng(3)
    parts = [system(n, rng) for n in SIZES]
    offsets = [0, *np.cumsum(SIZES).tolist()]
    excl = -np.ones((offsets[-1], 1), np.int32)
    for a in offsets[:-1]:                                   # one excluded pair per frame
        excl[a, 0], excl[a + 1, 0] = a + 1, a
    fpos, fq, fbox = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.stack([p[2] for p in parts]))
    spos, sq, sbox = system(ATOMS, rng)
    sexcl = -np.ones((ATOMS, 1), np.int32)
    sexcl[0, 0], sexcl[1, 0] = 1, 0
    frames = PME(*GRID, ORDER, ALPHA, COULOMB, torch.tensor(excl), reciprocal=True)
    single = PME(*GRID, ORDER, ALPHA, COULOMB, torch.tensor(sexcl), reciprocal=True)
    single_twice = PME(*GRID, ORDER, ALPHA, COULOMB, torch.tensor(sexcl), reciprocal=True, twice_differentiable=True)
    w = torch.tensor([1.0, -0.5, 2.0], device=dev)

    def leaves(pos, q, box, box_grad):
        return (torch.tensor(pos, device=dev, requires_grad=True), torch.tensor(q, device=dev, requires_grad=True),
                torch.tensor(box, device=dev, requires_grad=box_grad))

    def step(energy, x, c, b):
        lv = (x, c, b) if b.requires_grad else (x, c)
        return lambda: torch.autograd.grad(energy(x, c, b), lv)

    def force_step(energy, x, c, b):
        def fn():
            fx, fq_ = torch.autograd.grad(energy(x, c, b), (x, c), create_graph=True)
            torch.autograd.grad((fx ** 2).sum() + (fq_ ** 2).sum(), (x, c))
        return fn

    def recip_frames(**kw):
        return lambda x, c, b: (frames.compute_reciprocal_frames(x, c, b, offsets, **kw) * w).sum()

    def direct_frames(**kw):
        return lambda x, c, b: (frames.compute_direct_frames(x, c, CUTOFF, b, offsets, **kw) * w).sum()

    F, S = (fpos, fq, fbox), (spos, sq, sbox)
    rows = [
        ("pme_reciprocal_frames: forward + backward", step(recip_frames(), *leaves(*F, False))),
        ("pme_reciprocal_frames_box: forward + backward", step(recip_frames(box_gradient=True), *leaves(*F, True))),
        ("pme_reciprocal_frames_lds: forward + backward", step(recip_frames(transform="lds"), *leaves(*F, False))),
        ("pme_reciprocal_frames_twice: forward + backward", step(recip_frames(twice_differentiable=True), *leaves(*F, False))),
        ("pme_reciprocal_frames_twice: force-loss step", force_step(recip_frames(twice_differentiable=True), *leaves(*F, False))),
        ("pme_direct_frames: forward + backward", step(direct_frames(), *leaves(*F, False))),
        ("pme_direct_frames_twice: force-loss step", force_step(direct_frames(twice_differentiable=True), *leaves(*F, False))),
        ("pme_direct: forward + backward", step(lambda x, c, b: single.compute_direct(x, c, CUTOFF, b), *leaves(*S, False))),
        ("pme_direct_box: forward + backward", step(lambda x, c, b: single.compute_direct(x, c, CUTOFF, b), *leaves(*S, True))),
        ("pme_reciprocal: forward + backward", step(lambda x, c, b: single.compute_reciprocal(x, c, b), *leaves(*S, True))),
        ("pme_direct_twice: force-loss step", force_step(lambda x, c, b: single_twice.compute_direct(x, c, CUTOFF, b), *leaves(*S, False))),
        ("pme_reciprocal_twice: force-loss step", force_step(lambda x, c, b: single_twice.compute_reciprocal(x, c, b), *leaves(*S, False))),
    ]
    rounds = [[walled(fn) for _, fn in rows] for _ in range(15)]
    print(f"host time, frames {SIZES} / {ATOMS} atoms, grid {GRID}, wall clock us per call, medians of 15 interleaved rounds "
          f"(spread = max - min), root {ROOT}:")
    for k, (name, _) in enumerate(rows):
        q = [r[k] for r in rounds]
        print(f"  {name:50s} {np.median(q):9.1f} us  (min {min(q):.1f}, spread {max(q) - min(q):.1f})")


if __name__ == "__main__":
    main()
