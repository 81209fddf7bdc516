"""PME -- the direct-space (short-range) term of Particle Mesh Ewald on the HIP neighbour-pair list.

Mirrors the reference class (src/pytorch/pme/pme.py:5-165): same constructor arguments and checks, same
``compute_direct(positions, charges, cutoff, box_vectors, max_num_pairs)`` contract, same unit convention (the value of
Coulomb's constant sets the units), same exclusion semantics (only the un-wrapped copy of an excluded pair is left out, and
the erf() part that reciprocal space cannot leave out is subtracted here).  ``compute_direct`` = getNeighborPairs +
``torch.ops.pme.pme_direct``, differentiable w.r.t. positions and charges (first derivatives only).  When ``box_vectors``
requires a gradient (and grad mode is on) it calls ``torch.ops.pme.pme_direct_box`` instead: the same forward pass, bit for
bit, and dE/dbox as well.  Second derivatives with respect to positions and charges are an opt-in,
``PME(..., twice_differentiable=True)``.

The reciprocal-space term (charge spreading onto a grid + 3-D FFTs, src/pytorch/pme/pmeCUDA.cu:102-430) is
``torch.ops.pme.pme_reciprocal``: deterministic HIP passes around torch's FFTs (nnpops_amd/csrc/pme_recip.hip) and a CPU key.
The class reaches it through a keyword-only opt-in, ``PME(..., reciprocal=True)``: the constructor then computes the B-spline
moduli and ``compute_reciprocal`` returns the self energy plus the op, as the reference does.  With the default
``reciprocal=False`` the class behaves exactly as before and ``compute_reciprocal`` raises; making ``True`` the default is left
to a later change.
"""
import math

import numpy as np
import torch

from ..neighbors import getNeighborPairs


def bspline_moduli(size: int, order: int) -> torch.Tensor:
    """|sum_j M_n(j + 1) exp(2 pi i j k / K)|^2 for k = 0 .. K-1, K = `size`, n = `order` (the cardinal B-spline at the integers;
    the sum runs over the K terms j = 0 .. K-1, as the reference's class does, src/pytorch/pme/pme.py:95-130).  Entries below 1e-7
    are replaced by the mean of their two neighbours.  Computed in float64, returned as float32."""
    # M_n at the integer knots 1 .. n-1 by the recursion M_n(x) = (x M_{n-1}(x) + (n - x) M_{n-1}(x - 1)) / (n - 1)
    m = np.zeros(order + 1)
    m[1] = 1.0                                           # M_2: 1 at x = 1
    for n in range(3, order + 1):
        prev = m.copy()
        for x in range(1, n):
            m[x] = (x * prev[x] + (n - x) * prev[x - 1]) / (n - 1)
    values = np.zeros(size)
    count = min(size, order + 1)
    values[:count] = m[:count]                           # values[j] = M_n(j), j = 0 .. K-1
    j = np.arange(size)
    arg = 2.0 * np.pi * np.outer(j, j) / size
    mod = (values @ np.cos(arg)) ** 2 + (values @ np.sin(arg)) ** 2
    for k in range(size):
        if mod[k] < 1e-7:
            mod[k] = (mod[(k - 1 + size) % size] + mod[(k + 1) % size]) * 0.5
    return torch.tensor(mod, dtype=torch.float32)


_TWICE_BOX_MESSAGE = ("PME(..., twice_differentiable=True): box gradients need the default ops (PME without twice_differentiable); the "
                      "twice-differentiable ops return no box gradient")


class PME:
    """Particle Mesh Ewald (the reference's class, src/pytorch/pme/pme.py).  The direct- and reciprocal-space terms are not
    physically meaningful on their own, only their sum.

    Both terms are differentiable with respect to positions, charges and box vectors (first derivatives only; the reference
    offers no box derivative).  The box gradient is that of the physical energy with the positions held fixed as passed: all
    nine entries, in the box's dtype, so stress and virial losses see both PME terms.

    ``reciprocal`` (keyword only, default False): with True the constructor computes the B-spline moduli and
    ``compute_reciprocal`` works as the reference's; with False ``compute_reciprocal`` raises, as this class always did.  The
    default will become True in a later change.

    ``twice_differentiable`` (keyword only, default False): with True ``compute_direct`` and ``compute_reciprocal`` call
    ``torch.ops.pme.pme_direct_twice`` / ``pme_reciprocal_twice``: the same forward and first-order passes, bit for bit, whose
    backward can itself be differentiated with respect to positions and charges (``create_graph=True``: force matching, Hessian-
    vector products).  These ops return no box gradient -- a box that requires a gradient raises -- and the
    reciprocal term then needs ``order >= 4``.  With the default False second derivatives are refused, as before."""

    def __init__(self, gridx: int, gridy: int, gridz: int, order: int, alpha: float, coulomb: float, exclusions: torch.Tensor, *,
                 reciprocal: bool = False, twice_differentiable: bool = False):
        # the reference's argument checks (pme.py:75-85)
        if gridx < 1 or gridy < 1 or gridz < 1:
            raise ValueError('The grid dimensions must be positive')
        if order < 1:
            raise ValueError('order must be positive')
        if alpha <= 0:
            raise ValueError('alpha must be positive')
        if coulomb <= 0:
            raise ValueError('coulomb must be positive')
        if exclusions.dim() != 2:
            raise ValueError('exclusions must be 2D')
        self.gridx, self.gridy, self.gridz, self.order = gridx, gridy, gridz, order
        self.alpha, self.coulomb = alpha, coulomb
        # The table must be symmetric -- j in row i exactly when i is in row j (the reference documents it, pme.py:66-73, and its
        # kernel visits an excluded pair from the row of the higher index only).  The owner-computes HIP kernel has every atom take
        # the terms of its excluded pairs from ITS OWN row (nnpops_hip.h: nnpops_pme_direct): a one-sided table would give
        # derivatives that differ between the device and the host path without any error.  Checked here, once.
        ex = exclusions.to(torch.int64).cpu()
        n, width = ex.shape
        if width > 0 and n > 0:
            if bool(((ex >= n) | (ex < -1)).any()):
                raise ValueError('exclusions must hold atom indices or -1')
            rows = torch.arange(n).unsqueeze(1).expand(n, width)
            valid = ex >= 0
            pairs = torch.stack([rows[valid], ex[valid]], dim=1)
            keys = set((pairs[:, 0] * n + pairs[:, 1]).tolist())
            if any((j * n + i) not in keys for i, j in pairs.tolist()):
                raise ValueError('exclusions must be symmetric: if atom j is excluded from atom i, atom i must be excluded from atom j')
        # rows sorted in descending order: the kernels stop scanning a row at the first entry below the partner (pme.py:93)
        self.exclusions, _ = torch.sort(exclusions.to(torch.int32), descending=True)
        self.reciprocal = bool(reciprocal)
        self.twice_differentiable = bool(twice_differentiable)
        if self.reciprocal:
            self.moduli = [bspline_moduli(k, order) for k in (gridx, gridy, gridz)]

    def compute_direct(self, positions: torch.Tensor, charges: torch.Tensor, cutoff: float, box_vectors: torch.Tensor,
                       max_num_pairs: int = -1):
        """Energy of the direct-space term (a 0-dim tensor).  Differentiable with respect to positions, charges and, when it
        requires a gradient, box_vectors (``pme_direct_box``; the pair list's deltas pass no gradient, so the box is not counted
        twice)."""
        if positions.dim() != 2 or positions.shape[1] != 3:
            raise ValueError('positions must have shape (atoms, 3)')
        if charges.dim() != 1:
            raise ValueError('charges must be 1D')
        if positions.shape[0] != self.exclusions.shape[0] or charges.shape[0] != self.exclusions.shape[0]:
            raise ValueError('positions, charges, and exclusions must all have the same length')
        if box_vectors.dim() != 2 or box_vectors.shape[0] != 3 or box_vectors.shape[1] != 3:
            raise ValueError('box_vectors must have shape (3, 3)')
        if cutoff <= 0:
            raise ValueError('cutoff must be positive')
        neighbors, deltas, distances, _ = getNeighborPairs(positions, cutoff, max_num_pairs, box_vectors)
        self.exclusions = self.exclusions.to(positions.device)
        if self.twice_differentiable:
            if box_vectors.requires_grad and torch.is_grad_enabled():
                raise RuntimeError(_TWICE_BOX_MESSAGE)
            return torch.ops.pme.pme_direct_twice(positions, charges, neighbors, deltas, distances, self.exclusions, self.alpha,
                                                  self.coulomb)
        if box_vectors.requires_grad and torch.is_grad_enabled():
            return torch.ops.pme.pme_direct_box(positions, charges, neighbors, deltas, distances, self.exclusions, box_vectors,
                                                self.alpha, self.coulomb)
        return torch.ops.pme.pme_direct(positions, charges, neighbors, deltas, distances, self.exclusions, self.alpha, self.coulomb)

    def compute_reciprocal(self, positions: torch.Tensor, charges: torch.Tensor, box_vectors: torch.Tensor):
        """Energy of the reciprocal-space term including the self energy (a 0-dim tensor); needs ``PME(..., reciprocal=True)``.
        Differentiable with respect to positions, charges and box_vectors (the self energy does not depend on the box)."""
        if not self.reciprocal:
            raise RuntimeError("the reciprocal-space term of PME is not enabled on this object: construct it with "
                               "PME(..., reciprocal=True) (the default stays False for now, see DESIGN.md, scope)")
        if positions.dim() != 2 or positions.shape[1] != 3:
            raise ValueError('positions must have shape (atoms, 3)')
        if charges.dim() != 1:
            raise ValueError('charges must be 1D')
        if positions.shape[0] != self.exclusions.shape[0] or charges.shape[0] != self.exclusions.shape[0]:
            raise ValueError('positions, charges, and exclusions must all have the same length')
        if box_vectors.dim() != 2 or box_vectors.shape[0] != 3 or box_vectors.shape[1] != 3:
            raise ValueError('box_vectors must have shape (3, 3)')
        for i in range(3):
            self.moduli[i] = self.moduli[i].to(positions.device)
        self_energy = -torch.sum(charges ** 2) * (self.coulomb * self.alpha / math.sqrt(math.pi))
        if self.twice_differentiable:
            if box_vectors.requires_grad and torch.is_grad_enabled():
                raise RuntimeError(_TWICE_BOX_MESSAGE)
            return self_energy + torch.ops.pme.pme_reciprocal_twice(positions, charges, box_vectors, self.gridx, self.gridy, self.gridz,
                                                                    self.order, self.alpha, self.coulomb, self.moduli[0],
                                                                    self.moduli[1], self.moduli[2])
        return self_energy + torch.ops.pme.pme_reciprocal(positions, charges, box_vectors, self.gridx, self.gridy, self.gridz,
                                                          self.order, self.alpha, self.coulomb, self.moduli[0], self.moduli[1],
                                                          self.moduli[2])
