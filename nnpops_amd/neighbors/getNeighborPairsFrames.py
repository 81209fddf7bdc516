"""getNeighborPairsFrames -- the pair lists of a batch of frames, every frame in its own box, in one launch sequence."""
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, empty

from .. import torch_binding

torch_binding.load()


def frame_table(offsets: Union[Sequence[int], Tensor], device) -> Tensor:
    """Host-side preparation of a batch shape, done once: frame ``m`` holds the atoms ``[offsets[m], offsets[m + 1])``.

    ``offsets``: B + 1 ascending ints, the first 0; empty frames are allowed.  Every frame's lower triangle, n(n-1)/2 pairs in
    row-major order, is cut into consecutive segments of at most ``NNPOPS_PAIRS_FRAMES_PART_PAIRS`` pairs -- one workgroup each.
    Returns an int32 tensor on ``device`` with one row per segment, ``{frame, first atom, atom count, first flat pair, pair count}``,
    ordered by frame, then by first pair.  ``getNeighborPairsFrames`` takes this very tensor (not a copy or an edited one).
    """
    offsets = torch.as_tensor(offsets, dtype=torch.int64, device="cpu").reshape(-1)
    return torch.ops.neighbors.frameTable(offsets, torch.device(device))


def getNeighborPairsFrames(positions: Tensor, cutoff: float, table: Tensor, max_num_pairs: int = -1,
                           box_vectors: Optional[Tensor] = None, check_errors: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Returns ``(neighbors, deltas, distances, number_found_pairs)`` with the meanings of ``getNeighborPairs`` for a batch of frames.

    positions [N, 3] float32/float64 on the GPU, the frames one after the other as ``table = frame_table(offsets, device)`` describes
    them; atom indices in ``neighbors`` are global.  An atom is paired only with atoms of its own frame -- through the minimum image of
    ``box_vectors[m]`` when ``box_vectors`` [B, 3, 3] is given -- however the coordinates of different frames overlap, and a frame's
    slots hold the bits ``getNeighborPairs`` gives for that frame alone.  ``max_num_pairs = -1`` returns one slot per pair of each
    frame's triangle, frames concatenated; ``max_num_pairs > 0`` the compacted list, deterministic: grouped by ``neighbors[0]``
    ascending with ascending ``neighbors[1]`` inside a row; surplus pairs are dropped and ``number_found_pairs`` reports the true count
    (``check_errors=True`` raises instead, synchronises, and cannot be captured in a graph).

    Differentiable with respect to ``positions`` (twice, as ``getNeighborPairs``) and ``box_vectors`` (once: ``box_vectors.grad`` is
    [B, 3, 3] in the box's dtype, shifts held fixed; a backward pass under ``create_graph=True`` raises while the box requires a
    gradient).  GPU only.
    """
    if box_vectors is None:
        box_vectors = empty((0, 3, 3), device=positions.device, dtype=positions.dtype)
    return torch.ops.neighbors.getNeighborPairsFrames(positions, cutoff, max_num_pairs, table, box_vectors, check_errors)
