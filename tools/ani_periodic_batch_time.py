"""Periodic batches -- B frames of a 64-water box (192 atoms), each in its own box -- against what they replace, a loop of B
single-frame periodic calls on the same build: stream time per batch, interleaved rounds (batch, loop, batch, loop, ...), medians.

    AEV fwd+bwd         capi.AniSymmetryFunctions: compute() + backprop() of one handle with B molecules and box [B,3,3]
                        against B x (compute() + backprop()) of ONE single-frame handle
    ... with box grad   the same with backprop_box() (the per-molecule pass / the single frame's two launches)
    fused step          OptimizedTorchANI.forward_batch(..., cell [B,3,3], pbc) + backward against B x (forward(..., cell) + backward)

The frames are one water box, jittered by up to 0.05 A and scaled by 0.97 .. 1.04 (an NPT-like spread of cells); capacities are
fitted and every shape is warmed before the timed windows.

    python tools/ani_periodic_batch_time.py [B ...]        (default: 8 64 256)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import workloads  # noqa: E402
from nnpops_amd.capi import AniSymmetryFunctions  # noqa: E402

dev = torch.device("cuda:0")
S, RCR, RCA = 7, 5.1, 3.5
WATERS = 64


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


def interleaved(calls, reps, rounds=5):
    """-> {name: median over the rounds of the stream time per call, us}; every round times every call once, in turn"""
    seen = [{name: timed(fn, reps) for name, fn in calls.items()} for _ in range(rounds)]
    return {name: float(np.median([r[name] for r in seen])) for name in calls}


def frames(batch):
    pos, species, box = workloads.water_box(WATERS, seed=11)
    rng = np.random.default_rng(batch)
    scales = np.linspace(0.97, 1.04, batch) if batch > 1 else np.ones(1)
    coords = np.stack([((pos + rng.uniform(-0.05, 0.05, pos.shape)) * s).astype(np.float32) for s in scales])
    cells = np.stack([(box * np.float32(s)).astype(np.float32) for s in scales])
    assert float(cells[:, [0, 1, 2], [0, 1, 2]].min()) >= 2 * RCR
    return species, coords, cells


def c_abi(batch, species, coords, cells):
    rf, af = workloads.ani2x_functions()
    n = len(species)
    many = AniSymmetryFunctions(S, RCR, RCA, np.tile(species, batch), rf, af, periodic=True)
    many.set_molecules(np.arange(batch + 1, dtype=np.int32) * n)
    one = AniSymmetryFunctions(S, RCR, RCA, species, rf, af, periodic=True)
    x, boxes = torch.tensor(coords.reshape(batch * n, 3), device=dev), torch.tensor(cells, device=dev)
    xs, bs = [x[b * n:(b + 1) * n].contiguous() for b in range(batch)], [boxes[b].contiguous() for b in range(batch)]
    radial, angular = many.compute(x, boxes)                    # (fits the capacities)
    r1, a1 = one.compute(xs[0], bs[0])
    gen = torch.Generator(device=dev).manual_seed(0)
    wr, wa = torch.randn(radial.shape, device=dev, generator=gen), torch.randn(angular.shape, device=dev, generator=gen)
    wr1, wa1 = wr[:n].contiguous(), wa[:n].contiguous()
    g, gb = torch.empty_like(x), torch.empty_like(boxes)
    g1, gb1 = torch.empty_like(xs[0]), torch.empty_like(bs[0])

    def batch_plain():
        many.compute(x, boxes, radial, angular, check=False)
        many.backprop(wr, wa, g)

    def batch_box():
        many.compute(x, boxes, radial, angular, check=False)
        many.backprop_box(x, boxes, wr, wa, g, gb)

    def loop_plain():
        for b in range(batch):
            one.compute(xs[b], bs[b], r1, a1, check=False)
            one.backprop(wr1, wa1, g1)

    def loop_box():
        for b in range(batch):
            one.compute(xs[b], bs[b], r1, a1, check=False)
            one.backprop_box(xs[b], bs[b], wr1, wa1, g1, gb1)

    reps = max(2, 256 // batch)
    t = interleaved(dict(batch=batch_plain, loop=loop_plain, batch_box=batch_box, loop_box=loop_box), reps)
    return t, many.describe(), one.describe()


def fused_step(batch, species, coords, cells):
    from NNPOps import OptimizedTorchANI
    model = workloads.torchani_like_model(n_models=8, seed=2)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=dev)
    module = OptimizedTorchANI(model, numbers.cpu()).to(dev)
    pbc = torch.tensor([True, True, True])
    x = torch.tensor(coords, device=dev).requires_grad_(True)
    cell = torch.tensor(cells, device=dev)
    xs, cs = [x[b:b + 1].detach().clone().requires_grad_(True) for b in range(batch)], [cell[b].contiguous() for b in range(batch)]
    many = numbers.expand(batch, -1)

    def step_batch():
        x.grad = None
        module.forward_batch((many, x), cell, pbc).energies.sum().backward()

    def step_loop():
        for b in range(batch):
            xs[b].grad = None
            module((numbers, xs[b]), cs[b], pbc).energies.sum().backward()

    reps = max(2, 128 // batch)
    return interleaved(dict(batch=step_batch, loop=step_loop), reps)


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [8, 64, 256]
    for batch in sizes:
        species, coords, cells = frames(batch)
        t, what, what1 = c_abi(batch, species, coords, cells)
        f = fused_step(batch, species, coords, cells)
        print(f"B={batch} x {len(species)} atoms: AEV fwd+bwd batch {t['batch']:.1f} us, loop {t['loop']:.1f} us ({t['loop'] / t['batch']:.2f} x); "
              f"with box gradient batch {t['batch_box']:.1f} us, loop {t['loop_box']:.1f} us ({t['loop_box'] / t['batch_box']:.2f} x); "
              f"fused step batch {f['batch']:.1f} us, loop {f['loop']:.1f} us ({f['loop'] / f['batch']:.2f} x)  "
              f"(batch: batch_boxes={what.get('batch_boxes', '0')} fused_build={what['fused_build']} cap={what['cap']} cap_angular={what['cap_angular']}; "
              f"single: fused_build={what1['fused_build']} cells={what1['cells']})", flush=True)
