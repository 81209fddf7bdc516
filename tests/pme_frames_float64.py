"""The float64 judge of the PME frames ops, per frame, made from what tests/pme_float64.py has (no GPU code, no tests), and the seeded
case table of tests/test_pme_frames_gpu.py.

Direct term: every frame's minimum-image pair set in float64 (the single-round rule of getNeighborPairs: z, then y, then x; pairs with
r <= cutoff), minus the excluded pairs, with erfc terms, minus the un-wrapped erf terms of the excluded pairs (direct_energy_frozen).
Reciprocal term: spme_energy with the frame's box.  Derivatives by autograd.

Condition on the inputs: no pair's float64 distance lies within 1e-4 cutoff of the cutoff -- float32 and float64 could disagree on
membership there, and one pair's erfc(alpha r_c) / r_c would masquerade as an error.  Asserted when a case is built."""
import numpy as np
import torch

import pme_float64 as f64

ALPHA, COULOMB, CUTOFF = 3.5, 138.935, 1.0
LDS_ATOMS = 1024                     # pme_frames.hip: kFrameLdsAtoms


def frame_pairs(pos, box, excl, first, cutoff):
    """listed_pairs_frozen's tuple for one frame (indices inside the frame): included pairs i > j with their frozen shifts, excluded
    pairs a < b.  pos, box float64 tensors; excl: the global table's rows of this frame."""
    d = pos[:, None, :] - pos[None, :, :]
    for a in (2, 1, 0):
        d = d - torch.round(d[..., a] / box[a, a])[..., None] * box[a]
    r = torch.linalg.norm(d, dim=-1)
    lower = torch.tril(torch.ones_like(r, dtype=torch.bool), -1)
    assert not bool((lower & ((r - cutoff).abs() < 1e-4 * cutoff)).any()), "a pair sits on the cutoff: choose another seed"
    excluded = {(a, int(b) - first) for a in range(len(pos)) for b in excl[a] if b >= 0}
    i, j = torch.nonzero(lower & (r <= cutoff), as_tuple=True)
    keep = torch.tensor([(int(a), int(b)) not in excluded for a, b in zip(i, j)], dtype=torch.bool)
    i, j = i[keep], j[keep]
    shift = pos[i] - pos[j] - d[i, j]
    once = sorted((a, b) for a, b in excluded if a < b)
    return i, j, shift, torch.tensor([a for a, _ in once], dtype=torch.long), torch.tensor([b for _, b in once], dtype=torch.long)


def judge(energy_of_frame, pos, q, offsets, weights=None):
    """per-frame energies [B] and the gradients of sum_m weights[m] E_m (weights default to ones), float64"""
    x = torch.tensor(np.asarray(pos), dtype=torch.float64, requires_grad=True)
    c = torch.tensor(np.asarray(q), dtype=torch.float64, requires_grad=True)
    zero = (x.sum() + c.sum()) * 0
    e = torch.stack([energy_of_frame(m, x[a:b], c[a:b]) + zero if b > a else zero for m, (a, b) in enumerate(zip(offsets, offsets[1:]))])
    w = torch.ones(len(e), dtype=torch.float64) if weights is None else torch.as_tensor(weights, dtype=torch.float64)
    gx, gq = torch.autograd.grad((w * e).sum(), (x, c))
    return e.detach(), gx, gq


def direct_judge(pos, q, boxes, offsets, excl, cutoff=CUTOFF, alpha=ALPHA, coulomb=COULOMB, weights=None):
    """-> energies [B], the frames' sums of |terms| [B], dE/dx, dE/dq"""
    p64, b64 = torch.tensor(np.asarray(pos), dtype=torch.float64), torch.tensor(np.asarray(boxes), dtype=torch.float64)
    ex = np.asarray(excl)
    pairs = [frame_pairs(p64[a:b], b64[m], ex[a:b], a, cutoff) for m, (a, b) in enumerate(zip(offsets, offsets[1:]))]
    e, gx, gq = judge(lambda m, x, c: f64.direct_energy_frozen(x, c, pairs[m], alpha, coulomb), pos, q, offsets, weights)
    q64 = torch.tensor(np.asarray(q), dtype=torch.float64)
    terms = torch.stack([f64.direct_energy_frozen(p64[a:b], q64[a:b], pairs[m], alpha, coulomb, magnitude=True) + 0.0
                         for m, (a, b) in enumerate(zip(offsets, offsets[1:]))])
    return e, terms, gx, gq


def recip_judge(pos, q, boxes, offsets, grid, order, moduli, alpha=ALPHA, coulomb=COULOMB, weights=None):
    b64 = torch.tensor(np.asarray(boxes), dtype=torch.float64)
    return judge(lambda m, x, c: f64.spme_energy(x, c, b64[m], grid, order, alpha, coulomb, moduli), pos, q, offsets, weights)


def batch(sizes, seed, scales=(1.0,), triclinic=True, excl="few"):
    """Frames of `sizes` atoms from pme_float64.system (a third of the atoms one or two box lengths outside), frame m's box and positions
    scaled by scales[m % len(scales)] (boxes of 2.4 x scale: at least two cutoffs wide).  excl: "none", "few" (bonded-like pairs inside
    every frame), "wide" (atom 0 of every frame excludes up to 20 partners: a row wider than 16) or "all" (every pair of every frame).
    -> positions, charges, boxes [B, 3, 3] (float32 arrays), offsets, exclusions int32 [N, width] (global indices, -1 padded)"""
    pos, q, boxes, offsets, rows = [], [], [], [0], []
    for m, n in enumerate(sizes):
        s = scales[m % len(scales)]
        p, c, b = f64.system(triclinic, n=max(n, 1), seed=seed + m, outside=True)
        pos.append(p[:n] * np.float32(s)); q.append(c[:n]); boxes.append(b * np.float32(s))
        first = offsets[-1]
        if excl == "few" and n > 1:
            local = f64.exclusion_table(n, seed=seed + m).numpy()
        elif excl == "wide":
            local = -np.ones((n, max(min(n - 1, 20), 1)), np.int32)
            local[0, : min(n - 1, 20)] = np.arange(1, min(n - 1, 20) + 1)
            local[1 : min(n - 1, 20) + 1, 0] = 0
        elif excl == "all":
            local = np.array([[b for b in range(n) if b != a] for a in range(n)], np.int32).reshape(n, max(n - 1, 0))
        else:
            local = -np.ones((n, 0), np.int32)
        rows.append(np.where(local >= 0, local + first, -1))
        offsets.append(first + n)
    width = max(r.shape[1] for r in rows)
    table = -np.ones((offsets[-1], width), np.int32)
    for first, r in zip(offsets, rows):
        table[first : first + r.shape[0], : r.shape[1]] = r
    return np.concatenate(pos).astype(np.float32), np.concatenate(q).astype(np.float32), np.stack(boxes).astype(np.float32), offsets, table


# name -> batch(...) arguments.  Tile edges (15, 16, 17, 33), lanes without a partner and an atom without a neighbour (0, 1, 2); many
# small frames; one frame one atom over the LDS limit, and one exactly at it, next to a small one; neighbouring boxes a factor of two apart; a wide exclusion
# row; a frame in which every pair is excluded.
DIRECT_CASES = {
    "tile_edges": dict(sizes=(0, 1, 2, 15, 16, 17, 33), seed=11, scales=(1.0, 2.0)),
    "seventy_small": dict(sizes=tuple(1 + m % 9 for m in range(70)), seed=200, scales=(1.0, 2.0, 1.5)),
    "over_lds": dict(sizes=(LDS_ATOMS + 1, 5), seed=31, scales=(8.0, 1.0)),
    "at_lds": dict(sizes=(LDS_ATOMS, 3), seed=33, scales=(8.0, 1.0)),       # the last staged size (a box of 2.4 holds no 1 024 atoms clear of the cutoff)
    "orthorhombic": dict(sizes=(20, 33), seed=41, triclinic=False, excl="none"),
    "wide_row": dict(sizes=(33, 40), seed=51, excl="wide"),
    "all_excluded": dict(sizes=(6, 17, 9), seed=61, excl="all"),
}

# name -> (grid, order, sizes, seed, scales)
RECIP_CASES = {
    "ragged_grid_4": ((5, 7, 18), 4, (9, 0, 17, 40), 71, (1.0, 2.0)),
    "ragged_grid_5": ((5, 7, 18), 5, (9, 0, 17, 40), 72, (1.0, 2.0)),
    "folded_stencil": ((3, 3, 3), 4, (12, 5), 73, (1.0, 1.5)),
    "cube_16": ((16, 16, 16), 5, (33, 1, 64), 74, (1.0, 2.0)),
    "second_round": ((8, 8, 16), 5, (300, 0, 7), 75, (1.0, 1.0, 2.0)),
    "second_round_4": ((8, 8, 16), 4, (300, 20), 76, (1.0, 2.0)),
}


def reorder(case, order):
    """the batch `case` = (positions, charges, boxes, offsets, exclusions) with its frames in the given order (a subset is fine)"""
    pos, q, boxes, offsets, excl = case
    P, Q, E, off = [], [], [], [0]
    for m in order:
        a, b = offsets[m], offsets[m + 1]
        P.append(pos[a:b]); Q.append(q[a:b]); E.append(np.where(excl[a:b] >= 0, excl[a:b] - a + off[-1], -1))
        off.append(off[-1] + b - a)
    return np.concatenate(P), np.concatenate(Q), boxes[list(order)], off, np.concatenate(E).astype(np.int32)
