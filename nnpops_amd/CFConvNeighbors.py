"""CFConvNeighbors -- neighbour list of the continuous-filter convolution
(reference src/pytorch/CFConvNeighbors.py:27-45)."""
from typing import List, Optional

import torch
from torch import Tensor

from . import torch_binding

torch_binding.load()


class CFConvNeighbors(torch.nn.Module):

    molecule_offsets: List[int]

    def __init__(self, cutoff: float) -> None:
        super().__init__()
        self.holder = torch.classes.NNPOpsCFConvNeighbors.Holder(cutoff)
        self.molecule_offsets = []

    @torch.jit.export
    def set_molecules(self, molecule_offsets: List[int]) -> None:
        """An extension: the atoms are a batch of independent non-periodic molecules, atoms ``[offsets[m], offsets[m + 1])`` being
        molecule m (B + 1 entries, first 0, last the number of atoms; an empty list restores one system).  Atoms of different
        molecules never become neighbours, so one ``build`` and one ``CFConv`` call evaluate the whole batch, each molecule as if
        it were alone.  The offsets are kept with the module (the holder's pickle is its cutoff alone) and are handed to a holder
        that does not have them yet: a scripted, saved and reloaded module still batches.  The number of atoms of a holder is
        fixed by its first build, as ever: keep one module per batch shape."""
        self.holder.set_molecules(molecule_offsets)
        self.molecule_offsets = molecule_offsets

    @torch.jit.export
    def build(self, positions: Tensor, box: Optional[Tensor] = None) -> None:
        """``box`` (3, 3, rows = lattice vectors in reduced form) is an extension: the reference's Python surface
        is non-periodic although its core supports a box (src/schnet/CFConv.h:57).  A holder is periodic or not
        for life, decided by its first build."""
        if len(self.molecule_offsets) > 0:
            if box is not None:
                raise RuntimeError("CFConvNeighbors.build: batched molecules (set_molecules) are non-periodic and take no box")
            if self.holder.molecules() != self.molecule_offsets:
                self.holder.set_molecules(self.molecule_offsets)
        if box is None:
            self.holder.build(positions)
        else:
            self.holder.build_periodic(positions, box)
