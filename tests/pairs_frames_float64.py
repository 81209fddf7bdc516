"""What the getNeighborPairsFrames tests share: the seeded batch and a plain float64 restatement in torch -- a loop over frames, all
pairs of the lower triangle in row-major order, the z -> y -> x round-based minimum image."""
import torch

CUTOFF = 2.0
LDS_ATOMS = 512          # neighbor_pairs_frames.h: kFrameLdsAtoms
PART_PAIRS = 2079        # include/nnpops_hip.h: NNPOPS_PAIRS_FRAMES_PART_PAIRS; the 65-atom frame's triangle is one pair more
# sizes 0, 1, 2, 3, 63, 64, 65 (a row straddles two segments), one atom beyond the LDS cap, and frame 8 a copy of frame 5
SIZES = [0, 1, 2, 3, 63, 64, 65, LDS_ATOMS + 1, 64]
SEED = {True: 10, False: 7}         # periodic / molecules: seeds at which no distance lies within 1e-4 cutoff of the cutoff


def batch(periodic, seed=None):
    """-> positions [N, 3] float64 holding float32-representable numbers, offsets, boxes [B, 3, 3] float64 or None.  Triclinic boxes of a
    different size per frame, each at least two cutoffs wide; a third of the atoms lie outside their box."""
    g = torch.Generator().manual_seed(SEED[periodic] if seed is None else seed)
    offsets, pos, boxes = [0], [], []
    for m, n in enumerate(SIZES):
        edge = (2.2 + 0.13 * m) * CUTOFF * (2.4 if n > 100 else 1.0)
        box = torch.tensor([[edge, 0, 0], [0.11 * edge, 1.1 * edge, 0], [-0.07 * edge, 0.13 * edge, 0.95 * edge]])
        frac = torch.rand(n, 3, generator=g) * (1.6 if periodic else 1.0) - (0.3 if periodic else 0.0)
        pos.append(frac @ box)
        boxes.append(box)
        offsets.append(offsets[-1] + n)
    pos[8] = pos[5].clone()
    boxes[8] = boxes[5].clone()
    pos = torch.cat(pos).float().double()
    return pos, offsets, (torch.stack(boxes).float().double() if periodic else None)


def frame_pairs(pos, box):
    """Every pair of one frame's lower triangle: rows, cols (local), deltas, distances."""
    n = pos.shape[0]
    row, col = torch.tril_indices(n, n, -1)
    d = pos[row] - pos[col]
    if box is not None:
        for a in (2, 1, 0):
            d = d - torch.outer(torch.round(d[:, a] / box[a, a]), box[a])
    return row, col, d, d.norm(dim=1)


def reference(pos, offsets, boxes, cutoff=CUTOFF):
    """The compacted list of the batch in float64 (differentiable): rows, cols (global), deltas, distances, and the smallest
    |distance - cutoff| / cutoff over all candidate pairs."""
    rows, cols, dl, ds, margin = [], [], [], [], float("inf")
    for m, (a, b) in enumerate(zip(offsets, offsets[1:])):
        row, col, d, r = frame_pairs(pos[a:b], None if boxes is None else boxes[m])
        if r.numel():
            margin = min(margin, float(((r.detach() - cutoff).abs() / cutoff).min()))
        keep = r <= cutoff
        rows.append(row[keep] + a); cols.append(col[keep] + a); dl.append(d[keep]); ds.append(r[keep])
    return torch.cat(rows), torch.cat(cols), torch.cat(dl), torch.cat(ds), margin


def energy(dl, ds):
    """A smooth scalar of deltas and distances (no tensor is made here: a step that calls it can be captured in a graph)."""
    return (1.3 * torch.exp(-0.4 * ds ** 2)).sum() + 0.2 * ((0.3 * dl[:, 0] - 0.2 * dl[:, 1] + 0.9 * dl[:, 2]) ** 2).sum()
