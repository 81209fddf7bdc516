"""CFConvNeighbors -- neighbour list of the continuous-filter convolution
(reference src/pytorch/CFConvNeighbors.py:27-45)."""
from typing import List, Optional

import torch
from torch import Tensor

from . import torch_binding

torch_binding.load()


class CFConvNeighbors(torch.nn.Module):

    molecule_offsets: List[int]
    frame_offsets: List[int]

    def __init__(self, cutoff: float) -> None:
        super().__init__()
        self.holder = torch.classes.NNPOpsCFConvNeighbors.Holder(cutoff)
        self.molecule_offsets = []
        self.frame_offsets = []

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
    def set_frames(self, frame_offsets: List[int]) -> None:
        """An extension: the atoms are a batch of PERIODIC frames, atoms ``[offsets[m], offsets[m + 1])`` being frame m (B + 1 entries,
        first 0, last the number of atoms; an empty list restores one system), every frame in its own box -- a minibatch of an NPT
        trajectory.  ``build(positions, box[B, 3, 3])`` pairs an atom only with atoms of its own frame, through the minimum image of
        the frame's box, and ``CFConv(neighbors, positions, input, box[B, 3, 3])`` evaluates the whole batch in one launch sequence;
        a box that requires a gradient gets ``box.grad[B, 3, 3]``.  The offsets are kept with the module, as ``molecule_offsets`` are,
        so a scripted, saved and reloaded module still batches.  Not together with ``set_molecules``."""
        self.holder.set_frames(frame_offsets)
        self.frame_offsets = frame_offsets

    @torch.jit.export
    def build(self, positions: Tensor, box: Optional[Tensor] = None) -> None:
        """``box`` (3, 3, rows = lattice vectors in reduced form) is an extension: the reference's Python surface
        is non-periodic although its core supports a box (src/schnet/CFConv.h:57).  A holder is periodic or not
        for life, decided by its first build.  With frames set (``set_frames``) ``box`` is [B, 3, 3], a box for every frame."""
        if len(self.frame_offsets) > 0:
            if box is None:
                raise RuntimeError("CFConvNeighbors.build: periodic frames (set_frames) need the box of every frame, box[B, 3, 3]")
            if self.holder.frames() != self.frame_offsets:
                self.holder.set_frames(self.frame_offsets)
        if len(self.molecule_offsets) > 0:
            if box is not None:
                raise RuntimeError("CFConvNeighbors.build: batched molecules (set_molecules) are non-periodic and take no box")
            if self.holder.molecules() != self.molecule_offsets:
                self.holder.set_molecules(self.molecule_offsets)
        if box is None:
            self.holder.build(positions)
        else:
            self.holder.build_periodic(positions, box)
