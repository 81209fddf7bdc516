"""Energies + forces of B conformers of workloads.conformer(60) with workloads.torchani_like_model(): stream time per evaluation of
    (a) the batched one-node step, FusedOptimizedTorchANI.energy_and_forces_batch;
    (b) a Python loop of B single-molecule energy_and_forces calls;
    (c) the composition: forward_batch of OptimizedTorchANI(nn_layout='grouped', fused_step=False) and a backward pass,
at B = 8, 64 and 1 024.  Device events around a window of repetitions sized to about a third of a second, every variant warmed up at
the shape it is timed at, five interleaved rounds (a, b, c, a, b, c, ...) so that all three see the same clocks; the median and the
spread of the rounds are printed.  The capacity check of the AEV holders stays at its default (every call) in all three.

    python tools/ani_batch_energy_time.py [B ...]
    python tools/ani_batch_energy_time.py --profile batch|single [B]   (eleven calls of one variant only, for rocprofv3 --kernel-trace --stats:
                                                                       the calls of a kernel divided by eleven are its launches per step)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import workloads  # noqa: E402
from NNPOps import OptimizedTorchANI  # noqa: E402

dev = torch.device("cuda:0")


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps          # microseconds per evaluation


def reps_for(fn, target_ms=300.0):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    once = window(fn, 2)
    return max(3, min(2000, int(target_ms * 1e3 / max(once, 1.0))))


def setup(batch):
    model = workloads.torchani_like_model()
    base, species = workloads.conformer(60)
    rng = np.random.default_rng(batch)
    confs = np.stack([base + rng.uniform(-0.1, 0.1, base.shape).astype(np.float32) for _ in range(batch)]).astype(np.float32)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=dev)
    fused = OptimizedTorchANI(model, numbers.cpu()).to(dev)
    plain = OptimizedTorchANI(model, numbers.cpu(), nn_layout="grouped", fused_step=False).to(dev)
    assert type(fused).__name__ == "FusedOptimizedTorchANI"
    coords = torch.tensor(confs, device=dev)
    many = numbers.expand(batch, -1)
    singles = [coords[b:b + 1].contiguous() for b in range(batch)]

    def batched():
        return fused.energy_and_forces_batch((many, coords))

    def loop():
        return [fused.energy_and_forces((numbers, p)) for p in singles]

    def composition():
        p = coords.detach().requires_grad_(True)
        e = plain.forward_batch((many, p)).energies
        return e.detach(), -torch.autograd.grad(e.sum(), p)[0]

    return batched, loop, composition


def measure(batch):
    batched, loop, composition = setup(batch)
    print(f"B = {batch} conformers of 60 atoms, 8 members")
    # how far the three are from each other, before they are timed (the same float32 steps in another order)
    e_a, f_a = batched()
    out_b = loop()
    e_c, f_c = composition()
    e_b, f_b = torch.cat([o[0] for o in out_b]), torch.cat([o[1] for o in out_b])
    top = float(f_a.abs().max())
    for name, e, f in (("loop of single steps", e_b, f_b), ("composition", e_c, f_c)):
        print(f"    batched step vs {name}: energies differ by up to {float((e - e_a).abs().max()):.2e}, forces by up to "
              f"{float((f - f_a).abs().max()) / top:.2e} of the largest")
    variants = (("batched step", batched), ("loop of single steps", loop), ("composition", composition))
    reps = [reps_for(fn) for _, fn in variants]
    rounds = [[window(fn, r) for (_, fn), r in zip(variants, reps)] for _ in range(5)]
    print("    energies + forces, microseconds per evaluation (median of 5 interleaved rounds, min .. max):")
    for k, (name, _) in enumerate(variants):
        t = sorted(r[k] for r in rounds)
        print(f"    {name:22s} {t[2]:11.1f}   ({t[0]:.1f} .. {t[4]:.1f}; {reps[k]} evaluations per window; {t[2] / batch:.2f} per conformer)")
    sys.stdout.flush()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--profile" in sys.argv:
        which = args[0] if args else "batch"
        batch = int(args[1]) if len(args) > 1 else 64
        batched, loop, _ = setup(1 if which == "single" else batch)
        for _ in range(11):
            (loop if which == "single" else batched)()
        torch.cuda.synchronize()
    else:
        for batch in ([int(a) for a in args] or [8, 64, 1024]):
            measure(batch)
