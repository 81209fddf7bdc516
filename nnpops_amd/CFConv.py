"""CFConv -- SchNet continuous-filter convolution layer (reference src/pytorch/CFConv.py:29-83).

    neighbors = CFConvNeighbors(cutoff)
    conv = CFConv(gaussianWidth, 'ssp', weights1[G, W], biases1[W], weights2[W, W], biases2[W])
    neighbors.build(positions)
    output = conv(neighbors, positions, input)        # differentiable in positions and input

Periodic (an extension, as CFConvNeighbors.build's ``box``): pass the box vectors of the build to the convolution as well and the
output is differentiable in them too -- ``box.grad`` is dL/dbox with the minimum-image shifts of the build held fixed, from which
the stress is (sum_i x_i (x) dL/dx_i + box^T dL/dbox) / V:

    neighbors.build(positions, box)
    output = conv(neighbors, positions, input, box)

Training on forces (an extension): ``CFConv(..., twice_differentiable=True)`` records the backward pass so that it can be
differentiated once more with respect to positions and input -- ``torch.autograd.grad(E, positions, create_graph=True)`` followed by
``loss.backward()``, or a Hessian-vector product.  Forward and first backward are those of the default layer, bit for bit; the box
gets no gradient from it, and the list must not be rebuilt between the forward pass and the last derivative.  The default layer's
backward is not differentiable: under ``create_graph=True`` its share of the second derivative is missing.
"""
from typing import Optional

import torch
from torch import Tensor

from . import torch_binding
from .CFConvNeighbors import CFConvNeighbors

torch_binding.load()


class CFConv(torch.nn.Module):

    def __init__(self, gaussianWidth: float, activation: str, weights1: Tensor, biases1: Tensor, weights2: Tensor,
                 biases2: Tensor, twice_differentiable: bool = False) -> None:
        super().__init__()
        self.twice_differentiable = twice_differentiable
        self.holder = torch.classes.NNPOpsCFConv.Holder(gaussianWidth, activation, weights1, biases1, weights2, biases2)

    def forward(self, neighbors: CFConvNeighbors, positions: Tensor, input: Tensor, box: Optional[Tensor] = None) -> Tensor:
        if self.twice_differentiable:
            if box is None:
                return torch.ops.NNPOpsCFConv.operation_twice(self.holder, neighbors.holder, positions, input)
            return torch.ops.NNPOpsCFConv.operation_periodic_twice(self.holder, neighbors.holder, positions, box, input)
        if box is None:
            return torch.ops.NNPOpsCFConv.operation(self.holder, neighbors.holder, positions, input)
        return torch.ops.NNPOpsCFConv.operation_periodic(self.holder, neighbors.holder, positions, box, input)
