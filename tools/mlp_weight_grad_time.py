"""A training step of an ANI ensemble on the fused networks (OptimizedTorchANI(..., trainable=True): csrc/mlp_weight_grad.h behind
torch.ops.NNPOpsBatchedNN.FusedMLPMembersTrainable) against the same step on the plain-torch layout, at two shapes: stream time per
call, cases interleaved, medians of several rounds.

    conformers   64 conformers x 60 atoms (README's conformer batch), 8 members, ANI-2x widths, forward_batch
    water        2 001-atom periodic water (BASELINE config 2), 8 members, forward

    (a) default module: energy + coordinate gradient         what a step with fixed networks costs
    (b) trainable module: the same + the eight weight gradients
    (c) one rebuild of the packed planes: what an optimizer step adds before the next forward.  On the host route
        (_FusedSpeciesNN._refresh_planes: a few hundred small torch calls, wall clock) and on the device route
        (torch.ops.NNPOpsBatchedNN.PackNetworks + one small copy to the host: stream time and wall clock)
    (g) nn_layout='grouped', trainable=True: the step of (b) in plain torch, on the same device in the same run
    (l) a full loop step -- zero_grad, forward, backward, opt.step() (SGD), the next forward finding new weights -- of the fused and of
        the grouped trainable module: wall clock per step with the device drained at the end, and stream time
Prints the largest difference between the fused and the grouped parameter gradients as a fraction of each array's largest entry, as a
sanity figure (both float32).

    python tools/mlp_weight_grad_time.py [--rounds R] [--shape conformers|water|both]
    python tools/mlp_weight_grad_time.py --profile          (a few calls only, for rocprofv3 --kernel-trace --stats)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import workloads  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=10, warm=3):
    """stream time per call, us"""
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


def walled(fn, reps=5, warm=1):
    """wall clock per call with the device drained, us"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def shape(name):
    """-> (numbers [1, N] on the device, call(module, coordinates) -> energies, coordinates)"""
    if name == "conformers":
        base, species = workloads.conformer(60, seed=100)
        rng = np.random.default_rng(160)
        confs = np.stack([base + rng.uniform(-0.1, 0.1, base.shape).astype(np.float32) for _ in range(64)]).astype(np.float32)
        numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=dev)
        coords = torch.tensor(confs, device=dev)
        return numbers, (lambda module, p: module.forward_batch((numbers.expand(64, -1), p)).energies), coords
    pos, species, box = workloads.water_box(667, seed=1)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=dev)
    cell, pbc = torch.tensor(box, device=dev), torch.tensor([True, True, True])
    return numbers, (lambda module, p: module((numbers, p), cell, pbc).energies), torch.tensor(pos, device=dev).unsqueeze(0)


def measure(name, rounds, profile):
    from NNPOps import OptimizedTorchANI
    numbers, call, coords = shape(name)
    model = workloads.torchani_like_model(n_models=8, seed=2)
    default = OptimizedTorchANI(model, numbers.cpu()).to(dev)
    fused = OptimizedTorchANI(model, numbers.cpu(), trainable=True).to(dev)
    grouped = OptimizedTorchANI(model, numbers.cpu(), nn_layout="grouped", trainable=True).to(dev)
    p = coords.clone().requires_grad_(True)

    def step_default():
        return torch.autograd.grad(call(default, p).sum(), [p])

    def step_of(module):
        leaves = [p, *module.neural_networks.parameters()]
        return lambda: torch.autograd.grad(call(module, p).sum(), leaves)

    step_fused, step_grouped = step_of(fused), step_of(grouped)
    nets = fused.neural_networks[0]
    call(fused, p)                                                     # (the planes of the module on the device)
    assert nets._packs_on_device(), "the fused trainable module does not pack on the device here"
    from NNPOps.BatchedNN import _FusedSpeciesNN

    def loop_of(module):
        opt = torch.optim.SGD(module.neural_networks.parameters(), lr=1e-9)

        def step():
            opt.zero_grad(set_to_none=True)
            p.grad = None
            call(module, p).sum().backward()
            opt.step()
        return step

    loop_fused, loop_grouped = loop_of(fused), loop_of(grouped)
    parameters = [q.detach() for q in nets.parameters()]

    def pack_alone():                                                  # (the op without the copy of its status block: nothing waits)
        return torch.ops.NNPOpsBatchedNN.PackNetworks(parameters, nets.widths, nets.x_blocks if nets.live_blocks else None)

    def host_route():
        with torch.no_grad():
            _FusedSpeciesNN._refresh_planes(nets)
    stream = [("(a) default: energy + coordinate gradient", step_default),
              ("(b) trainable, fused: + the eight weight gradients", step_fused),
              ("(g) trainable, grouped (plain torch): the same step", step_grouped),
              ("(c) PackNetworks alone: the two launches (stream)", pack_alone),
              ("(c) rebuild of the planes, device route (stream)", nets._refresh_planes),
              ("(l) loop step, fused (stream)", loop_fused),
              ("(l) loop step, grouped (stream)", loop_grouped)]
    wall = [("(c) rebuild of the planes, host route (wall clock)", host_route),
            ("(c) rebuild of the planes, device route (wall clock)", nets._refresh_planes),
            ("(l) loop step, fused (wall clock)", loop_fused),
            ("(l) loop step, grouped (wall clock)", loop_grouped)]
    if profile:
        for _ in range(3):
            for _, fn in stream[:5]:
                fn()
        torch.cuda.synchronize()
        return
    table = [[timed(fn) for _, fn in stream] + [walled(fn) for _, fn in wall] for _ in range(rounds)]            # interleaved
    names = [n for n, _ in stream + wall]
    med = [float(np.median([q[k] for q in table])) for k in range(len(names))]
    spread = [float(np.max([q[k] for q in table]) - np.min([q[k] for q in table])) for k in range(len(names))]
    print(f"{name}: {coords.shape[0]} x {coords.shape[1]} atoms, 8 members, medians of {rounds} interleaved rounds (spread = max - min):")
    for n, m, s in zip(names, med, spread):
        print(f"  {n:58s} {m:10.1f} us  (spread {s:.1f})")
    print(f"  (b) / (a) {med[1] / med[0]:.2f}    (g) / (b) {med[2] / med[1]:.2f}    (c) host / device, wall clock {med[7] / med[8]:.1f}"
          f"    (l) grouped / fused, wall clock {med[10] / med[9]:.2f}")
    read = sum(q.numel() * 4 for q in parameters)
    written = 2 * (nets.mlp_planes.numel() + nets.live_planes.numel()) + 4 * nets.mlp_floats.numel()
    print(f"  the device rebuild reads {read / 1e6:.1f} MB of parameters once (the first layer three to five times: its planes, their transposes,"
          f" the live sets) and writes {written / 1e6:.1f} MB: {(read + written) / med[3] / 1e6:.2f} TB/s of stream time counting every array once")
    worst = 0.0
    for a, b in zip(step_fused()[1:], step_grouped()[1:]):
        for k in range(a.shape[0]):
            worst = max(worst, float((a[k] - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-30)))
    print(f"  fused against grouped parameter gradients: {worst:.2e} of each array's largest entry per kind")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default="both", choices=("conformers", "water", "both"))
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    for name in (("conformers", "water") if args.shape == "both" else (args.shape,)):
        measure(name, args.rounds, args.profile)


if __name__ == "__main__":
    main()
