"""Synthetic atomic networks for the tests of the whole-ensemble pack (no GPU code, no tests; importable anywhere): modules of the library
built from made-up networks of any input width, layer widths, number of kinds and members, and the host formulas the pack's status block
is judged by.  The judge of the planes themselves is the library's host route, ``_FusedSpeciesNN._refresh_planes``.
"""
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

THRESHOLD = 62500.0            # BatchedNN.py: the activation bound of scale 2^-k is 62 500 * 2^k

# name -> (input width, true layer widths (h1, h2, h3) per kind, members, live 16-column blocks or None).  The packed widths are the
# true ones rounded up to 32; the module's arrays are padded to the widest kind.
#   F = 8: a lone partial K step, and a partial row block in the transposed first layer;  40: a K tail;  1008: ANI-2x;  1024: the maximum
#   widths from {32, 96, 160, 256}; "two-kinds": the padding to the widest is stripped, and 90 / 150 / 20 end inside a block of 32
#   "eight-kinds": the most kinds, one whose third layer is a single row block (16)
#   live blocks: 3 of F = 1008 (adds w0t per member), 17 (272 columns: none)
CASES = {
    "F8": (8, [(32, 32, 32)], 1, None),
    "two-kinds": (40, [(90, 150, 20), (256, 96, 96)], 3, None),
    "ani2x-live3": (1008, [(160, 96, 32), (96, 96, 96)], 3, [2, 17, 40]),
    "ani2x-live17": (1008, [(96, 32, 32)], 1, [0, 1, 2, 5, 8, 9, 13, 20, 21, 22, 30, 31, 40, 47, 55, 61, 62]),
    "F1024-members8": (1024, [(256, 160, 96)], 8, None),
    "eight-kinds": (40, [(32, 32, 32), (96, 32, 16), (32, 96, 32), (160, 32, 32), (32, 160, 96), (96, 96, 96), (256, 32, 32), (32, 256, 160)], 1, None),
}


class _Converter:
    """atomic numbers that are the species themselves"""

    def __call__(self, pair):
        return SimpleNamespace(species=pair[0])


def ensemble(F, kinds, members, seed, wide=True):
    """A ModuleList of `members` models, each a list of Sequential(Linear CELU Linear CELU Linear CELU Linear) per kind.  wide: magnitudes
    10^-8 .. 10^3 with random signs (both fp16 planes carry bits); else ordinary weights, uniform in +-1 / sqrt(fan in)."""
    rng = np.random.default_rng(seed)

    def values(*shape):
        if wide:
            return torch.tensor((rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-8, 3, shape)).astype(np.float32))
        return torch.tensor((rng.uniform(-1, 1, shape) / np.sqrt(shape[-1])).astype(np.float32))
    models = []
    for _ in range(members):
        nets = []
        for h1, h2, h3 in kinds:
            layers = []
            for n_in, n_out in ((F, h1), (h1, h2), (h2, h3), (h3, 1)):
                linear = nn.Linear(n_in, n_out)
                with torch.no_grad():
                    linear.weight.copy_(values(n_out, n_in))
                    linear.bias.copy_(values(n_out))
                layers += [linear, nn.CELU(0.1)]
            nets.append(nn.Sequential(*layers[:-1]))
        models.append(nn.ModuleList(nets))
    return nn.ModuleList(models)


def module(name, trainable, seed=0, wide=True):
    """the fused networks of a case on the CPU, packed there by the host route: one atom per kind; the live blocks set"""
    from NNPOps.BatchedNN import TorchANIBatchedNN
    F, kinds, members, live = CASES[name]
    numbers = torch.arange(len(kinds)).unsqueeze(0)
    nets = TorchANIBatchedNN(_Converter(), ensemble(F, kinds, members, seed, wide), numbers, trainable=trainable)[0]
    if live is not None:
        nets.set_live_blocks(live)
    return nets


def host_bounds(nets):
    """(bound, back) of _FusedSpeciesNN._refresh_planes from the module's arrays, in float64 on the CPU"""
    w = [getattr(nets, f"layer{l}_weights").detach().double().cpu() for l in (0, 2, 4, 6)]
    b = [getattr(nets, f"layer{l}_biases").detach().double().cpu() for l in (0, 2, 4)]
    bound = 64.0
    for wl, bl in zip(w[:3], b):
        bound = float(wl.abs().sum(-1).amax()) * bound + float(bl.abs().amax())
    back = float(w[3].abs().amax())
    for wl in (w[2], w[1]):
        back = float(wl.abs().sum(-2).amax()) * back
    return bound, back


def scale_of(worst):
    """-> (act_scale_log2, fused_ok, the factor between `worst` and the nearest threshold 62 500 * 2^k, k = 4 .. 12)"""
    k = 4
    while k < 12 and worst >= THRESHOLD * 2.0 ** k:
        k += 1
    margin = min(max(worst / (THRESHOLD * 2.0 ** j), (THRESHOLD * 2.0 ** j) / worst) for j in range(4, 13))
    return k, worst < THRESHOLD * 2.0 ** k, margin


def bits(t):
    """a tensor of fp16 planes, floats or status words as integers: NaNs compare"""
    if t.numel() == 0:
        return torch.empty(0, dtype=torch.int16)
    return t.detach().cpu().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])
