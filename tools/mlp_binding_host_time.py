"""Host time of the fused atomic networks' autograd nodes and of a rebuild of their planes: wall clock per call at a shape where the
host dominates (73 atoms in two kinds, 3 members, F = 1008 over 3 live column blocks: the shape of tests/test_mlp_binding_nodes_gpu.py),
the device drained at the end of each bracket; rows interleaved, medians and smallest rounds of 15.  What a change of
torch_binding.cpp's FusedMLP* nodes or of BatchedNN.py's dispatch can move, and what the stream-time rows of mlp_weight_grad_time.py
cannot see.

    python tools/mlp_binding_host_time.py [ROOT]        ROOT: another checkout, built, to time instead of this one"""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import nnpops_amd  # noqa: E402
from NNPOps.BatchedNN import TorchANIBatchedNN, _FusedSpeciesNN  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(nnpops_amd.__file__))) == ROOT, nnpops_amd.__file__
dev = "cuda:0"
ATOMS, M, F, LIVE, WIDTHS = 73, 3, 1008, [2, 17, 40], [(96, 64, 32), (40, 32, 17)]


def walled(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def ensemble(seed=7):
    """M models of one Sequential(Linear CELU Linear CELU Linear CELU Linear) per kind, weights uniform in +-1 / sqrt(fan in)"""
    gen = torch.Generator().manual_seed(seed)
    models = []
    for _ in range(M):
        nets = []
        for widths in WIDTHS:
            layers = []
            for n_in, n_out in zip((F,) + widths, widths + (1,)):
                linear = nn.Linear(n_in, n_out)
                with torch.no_grad():
                    linear.weight.copy_((2 * torch.rand((n_out, n_in), generator=gen) - 1) / n_in ** 0.5)
                    linear.bias.copy_((2 * torch.rand(n_out, generator=gen) - 1) / n_in ** 0.5)
                layers += [linear, nn.CELU(0.1)]
            nets.append(nn.Sequential(*layers[:-1]))
        models.append(nn.ModuleList(nets))
    return nn.ModuleList(models)


def main():
    numbers = torch.tensor([[1 if a in (5, 30, 72) else 0 for a in range(ATOMS)]])
    converter = lambda pair: SimpleNamespace(species=pair[0])
    default, trainable = (TorchANIBatchedNN(converter, ensemble(), numbers, trainable=flag)[0].to(dev) for flag in (False, True))
    for nets in (default, trainable):
        nets.set_live_blocks(LIVE)
    x = (torch.rand((ATOMS, F), generator=torch.Generator().manual_seed(1)) * 0.5).to(dev).requires_grad_(True)
    g = torch.tensor([[0.7, -0.2, 0.4]], device=dev)
    leaves = [x, *trainable.parameters()]

    def host_route():
        with torch.no_grad():
            _FusedSpeciesNN._refresh_planes(trainable)

    rows = [("FusedMLPMembers: forward + backward", lambda: torch.autograd.grad((default.fused_members(x) * g).sum(), [x]), 300),
            ("FusedMLPMembersTrainable: forward + backward", lambda: torch.autograd.grad((trainable.fused_members(x) * g).sum(), leaves), 300),
            ("FusedMLPMeanTrainable: forward + backward", lambda: torch.autograd.grad(trainable.fused_mean(x).sum(), leaves), 300),
            ("rebuild of the planes, device route", trainable._refresh_planes, 100),
            ("rebuild of the planes, host route", host_route, 3)]
    trainable.fused_members(x)
    assert trainable._packs_on_device(), "the trainable module does not pack on the device here"
    rounds = [[walled(fn, reps, max(reps // 10, 1)) for _, fn, reps in rows] for _ in range(15)]
    print(f"host time, {ATOMS} atoms M={M} F={F} over {len(LIVE)} live blocks, wall clock us per call, medians of 15 interleaved rounds, root {ROOT}:")
    for k, (name, _, _) in enumerate(rows):
        q = [r[k] for r in rounds]
        print(f"  {name:48s} {np.median(q):10.1f} us  (min {min(q):.1f}, spread {max(q) - min(q):.1f})")


if __name__ == "__main__":
    main()
