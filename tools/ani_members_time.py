"""What the two-node form of the member energies costs next to the one-node step, on the config-2 frame (667 waters, 2 001 atoms,
periodic, workloads.torchani_like_model() with 8 members), same module, same frame:
    (a) forward + backward of the energy (FusedOptimizedTorchANI.forward: one autograd node);
    (b) energies_qbcs + backward of the QBC factor (the AEV op, FusedMLPMembers, a handful of small torch kernels for mean and std).
Device events around a window of repetitions sized to about a third of a second, both warmed up, five interleaved rounds; median and
spread are printed.  The capacity check of the AEV holder stays at its default (every call) in both.

    python tools/ani_members_time.py [n_waters]"""
import os
import sys

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
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    once = window(fn, 3)
    return max(3, min(2000, int(target_ms * 1e3 / max(once, 1.0))))


if __name__ == "__main__":
    waters = int(sys.argv[1]) if len(sys.argv) > 1 else 667
    pos, species, box = workloads.water_box(waters)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]], device=dev)
    module = OptimizedTorchANI(workloads.torchani_like_model(), numbers.cpu()).to(dev)
    assert type(module).__name__ == "FusedOptimizedTorchANI"
    coords = torch.tensor(pos[None], device=dev)
    cell, pbc = torch.tensor(box, device=dev), torch.tensor([True, True, True], device=dev)

    def energy():
        p = coords.detach().requires_grad_(True)
        e = module((numbers, p), cell, pbc).energies
        return e.detach(), torch.autograd.grad(e.sum(), p)[0]

    def qbc():
        p = coords.detach().requires_grad_(True)
        _, e, q = module.energies_qbcs((numbers, p), cell, pbc)
        return e.detach(), torch.autograd.grad(q.sum(), p)[0]

    variants = (("forward + backward", energy), ("energies_qbcs + backward of qbcs", qbc))
    reps = [reps_for(fn) for _, fn in variants]
    rounds = [[window(fn, r) for (_, fn), r in zip(variants, reps)] for _ in range(5)]
    print(f"{3 * waters} atoms, 8 members, {16 * module.neural_networks[0].x_blocks.numel()} live columns; microseconds per evaluation "
          "(median of 5 interleaved rounds, min .. max):")
    for k, (name, _) in enumerate(variants):
        t = sorted(r[k] for r in rounds)
        print(f"    {name:34s} {t[2]:9.1f}   ({t[0]:.1f} .. {t[4]:.1f}; {reps[k]} evaluations per window)")
