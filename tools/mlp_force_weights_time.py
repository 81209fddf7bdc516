"""A training step on a loss with FORCES in it, on the fused networks (OptimizedTorchANI(..., force_trainable=True):
csrc/mlp_weight_grad_tangent.h behind torch.ops.NNPOpsBatchedNN.FusedMLPMeanForceTrainable) against the same step on the plain-torch
layout (nn_layout='grouped', trainable=True), and the new call next to nnpops_mlp_weight_grad, at two shapes: stream time per call,
cases interleaved, medians of several rounds (the method of tools/mlp_weight_grad_time.py).

    conformers   64 conformers x 60 atoms, 8 members, ANI-2x widths, forward_batch
    water        2 001-atom periodic water, 8 members, forward

    (w) nnpops_mlp_weight_grad                 the first-order weight gradient of the frame's networks (capi.FusedMLP, the module's
    (t) nnpops_mlp_weight_grad_tangent         packed widths and live blocks, a random AEV-sized x and tangent), with and without E'
    (e) energy-only step, fused / grouped      E, backward in the coordinates and the parameters
    (f) force-loss step, fused / grouped       E, F = -dE/dx with create_graph, (E - E0)^2 + sum (F - F0)^2, grad in the parameters
Prints the largest difference between the fused and the grouped parameter gradients of (f) as a fraction of each array's largest entry.

    python tools/mlp_force_weights_time.py [--rounds R] [--shape conformers|water|both]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mlp_weight_grad_time import shape, timed, walled  # noqa: E402
from nnpops_amd import workloads  # noqa: E402

dev = torch.device("cuda:0")


def fused_mlp_of(nets, batch):
    """capi.FusedMLP over the module's networks at their packed widths, every species' atoms `batch` times, live blocks as in the module"""
    from nnpops_amd.capi import FusedMLP
    kinds, first = [], 0
    for k, n in enumerate(nets.group_sizes):
        h1, h2, h3 = nets.widths[3 * k:3 * k + 3]
        get = lambda name: getattr(nets, name).detach()[k]
        kinds.append(dict(w0=get("layer0_weights")[:, :h1].contiguous(), b0=get("layer0_biases")[:, :h1, 0].contiguous(),
                          w2=get("layer2_weights")[:, :h2, :h1].contiguous(), b2=get("layer2_biases")[:, :h2, 0].contiguous(),
                          w4=get("layer4_weights")[:, :h3, :h2].contiguous(), b4=get("layer4_biases")[:, :h3, 0].contiguous(),
                          w6=get("layer6_weights")[:, 0, :h3].contiguous(), b6=get("layer6_biases")[:, 0, 0].contiguous(),
                          atoms=torch.arange(first * batch, (first + n) * batch, dtype=torch.int32, device=dev)))
        first += n
    width = int(nets.layer0_weights.shape[3])
    return FusedMLP(kinds, width, alpha=0.1, live_groups=list(nets.live_blocks) if nets.live_blocks else None), first * batch, width


def measure(name, rounds):
    from NNPOps import OptimizedTorchANI
    numbers, call, coords = shape(name)
    model = workloads.torchani_like_model(n_models=8, seed=2)
    fused = OptimizedTorchANI(model, numbers.cpu(), force_trainable=True).to(dev)
    grouped = OptimizedTorchANI(model, numbers.cpu(), nn_layout="grouped", trainable=True).to(dev)
    p = coords.clone().requires_grad_(True)
    with torch.no_grad():
        e0 = call(grouped, coords).detach() + 0.3
    f0 = 0.05 * torch.randn(coords.shape, generator=torch.Generator().manual_seed(7)).to(dev)

    def energy_step(module):
        leaves = [p, *module.neural_networks.parameters()]
        return lambda: torch.autograd.grad(call(module, p).sum(), leaves)

    def force_step(module):
        params = list(module.neural_networks.parameters())

        def step():
            energies = call(module, p)
            force = -torch.autograd.grad(energies.sum(), p, create_graph=True)[0]
            loss = ((energies - e0) ** 2).sum() + ((force - f0) ** 2).sum()
            return torch.autograd.grad(loss, params)
        return step

    mlp, atoms, width = fused_mlp_of(fused.neural_networks[0], int(coords.shape[0]))
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand((atoms, width), generator=gen) * 0.5).to(dev)
    t = torch.randn((atoms, width), generator=gen).to(dev)
    mlp.forward(x, with_gradient=True)
    cases = [("(w) nnpops_mlp_weight_grad", lambda: mlp.weight_grad()),
             ("(t) nnpops_mlp_weight_grad_tangent", lambda: mlp.weight_grad_tangent(t)),
             ("(t) nnpops_mlp_weight_grad_tangent with E'", lambda: mlp.weight_grad_tangent(t, tangent_energies=True)),
             ("(e) energy-only step, fused", energy_step(fused)), ("(e) energy-only step, grouped", energy_step(grouped)),
             ("(f) force-loss step, fused", force_step(fused)), ("(f) force-loss step, grouped", force_step(grouped))]
    wall = cases[5:]
    table = [[timed(fn) for _, fn in cases] + [walled(fn) for _, fn in wall] for _ in range(rounds)]                # interleaved
    names = [n + " (stream)" for n, _ in cases] + [n + " (wall clock)" for n, _ in wall]
    med = [float(np.median([q[k] for q in table])) for k in range(len(names))]
    spread = [float(np.max([q[k] for q in table]) - np.min([q[k] for q in table])) for k in range(len(names))]
    print(f"{name}: {coords.shape[0]} x {coords.shape[1]} atoms, 8 members, medians of {rounds} interleaved rounds (spread = max - min):")
    for n, m, s in zip(names, med, spread):
        print(f"  {n:58s} {m:10.1f} us  (spread {s:.1f})")
    print(f"  (t) / (w) {med[1] / med[0]:.2f}    (e) grouped / fused {med[4] / med[3]:.2f}    (f) grouped / fused, stream {med[6] / med[5]:.2f}, "
          f"wall clock {med[8] / med[7]:.2f}    (f) / (e), fused {med[5] / med[3]:.2f}")
    worst = 0.0
    for a, b in zip(force_step(fused)(), force_step(grouped)()):
        for k in range(a.shape[0]):
            worst = max(worst, float((a[k] - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-30)))
    print(f"  fused against grouped parameter gradients of the force loss: {worst:.2e} of each array's largest entry per kind", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default="both", choices=("conformers", "water", "both"))
    args = ap.parse_args()
    for name in (("conformers", "water") if args.shape == "both" else (args.shape,)):
        measure(name, args.rounds)


if __name__ == "__main__":
    main()
