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

Trainable filters (an extension): ``CFConv(..., trainable=True)`` turns the four arrays into ``torch.nn.Parameter``s (``weights1``,
``biases1``, ``weights2``, ``biases2``, with the shapes the constructor takes) that receive gradients from ``backward()``; the
convolution's own handle is given the new values on the first forward pass after an optimizer step, ``load_state_dict`` or
``.to(device)``, and nothing is copied while they stand.  Forward and the gradients in positions, input and box are those of the
default layer, bit for bit.  First derivatives only: ``create_graph=True`` raises, and so does ``trainable=True`` together with
``twice_differentiable=True`` (mixed second derivatives with respect to the weights are not implemented by those two ops).

Trainable filters under a force loss (an extension): ``CFConv(..., force_trainable=True)`` has the four parameters of
``trainable=True`` (same names and shapes: state dicts interchange, ``.to(device)``, optimizers and the lazy upload work as there) and
records its backward pass as ``twice_differentiable=True`` does, so that ``F = -torch.autograd.grad(E, positions, create_graph=True)``
followed by ``loss(E, F).backward()`` reaches the weights: the mixed second derivatives come from one more kernel over the pair list.
Forward, first gradients and first-order weight gradients are those of ``trainable=True``, the second derivatives in positions and
input those of ``twice_differentiable=True``, bit for bit.  The flag stands alone (with either of the other two it raises).  Refused:
third derivatives, second derivatives of the weight gradients themselves, a box that requires a gradient, a list rebuilt or weights
changed between the forward pass and the last derivative.
"""
from typing import Optional

import torch
from torch import Tensor

from . import torch_binding
from .CFConvNeighbors import CFConvNeighbors

torch_binding.load()


class CFConv(torch.nn.Module):

    def __init__(self, gaussianWidth: float, activation: str, weights1: Tensor, biases1: Tensor, weights2: Tensor,
                 biases2: Tensor, twice_differentiable: bool = False, trainable: bool = False, force_trainable: bool = False) -> None:
        super().__init__()
        if force_trainable and (trainable or twice_differentiable):
            raise ValueError("CFConv: force_trainable=True stands alone: it already has the parameters of trainable=True and the second "
                             "derivatives of twice_differentiable=True, and cannot be combined with either flag")
        if trainable and twice_differentiable:
            raise ValueError("CFConv: trainable=True cannot be combined with twice_differentiable=True: mixed second derivatives with "
                             "respect to the filter network's weights (a force loss differentiated with respect to them) are not "
                             "implemented by these two flags; CFConv(..., force_trainable=True) has them")
        self.twice_differentiable = twice_differentiable
        self.trainable = trainable
        self.force_trainable = force_trainable
        if trainable or force_trainable:
            new = lambda t: torch.nn.Parameter(t.detach().to(torch.float32).clone().contiguous())
            self.weights1, self.biases1 = new(weights1), new(biases1)
            self.weights2, self.biases2 = new(weights2), new(biases2)
        else:       # (attributes of the same names and types, for scripting; not parameters, not in the state_dict, never read)
            self.weights1, self.biases1 = torch.empty(0), torch.empty(0)
            self.weights2, self.biases2 = torch.empty(0), torch.empty(0)
        self.holder = torch.classes.NNPOpsCFConv.Holder(gaussianWidth, activation, weights1, biases1, weights2, biases2)

    def forward(self, neighbors: CFConvNeighbors, positions: Tensor, input: Tensor, box: Optional[Tensor] = None) -> Tensor:
        if self.force_trainable:
            if box is None:
                return torch.ops.NNPOpsCFConv.operation_weights_twice(self.holder, neighbors.holder, positions, input, self.weights1,
                                                                      self.biases1, self.weights2, self.biases2)
            return torch.ops.NNPOpsCFConv.operation_periodic_weights_twice(self.holder, neighbors.holder, positions, box, input,
                                                                           self.weights1, self.biases1, self.weights2, self.biases2)
        if self.trainable:
            if box is None:
                return torch.ops.NNPOpsCFConv.operation_weights(self.holder, neighbors.holder, positions, input, self.weights1,
                                                                self.biases1, self.weights2, self.biases2)
            return torch.ops.NNPOpsCFConv.operation_periodic_weights(self.holder, neighbors.holder, positions, box, input, self.weights1,
                                                                     self.biases1, self.weights2, self.biases2)
        if self.twice_differentiable:
            if box is None:
                return torch.ops.NNPOpsCFConv.operation_twice(self.holder, neighbors.holder, positions, input)
            return torch.ops.NNPOpsCFConv.operation_periodic_twice(self.holder, neighbors.holder, positions, box, input)
        if box is None:
            return torch.ops.NNPOpsCFConv.operation(self.holder, neighbors.holder, positions, input)
        return torch.ops.NNPOpsCFConv.operation_periodic(self.holder, neighbors.holder, positions, box, input)
