"""The float64 judge of every reciprocal pass of PME over frames (pme_frames.hip), and the cases at which those passes' loops reach their
edges (no GPU code, no tests; importable anywhere).

The passes themselves are those of tests/pme_recip_passes_reference.py -- spread64, convolve64, interpolate64 take a box and serve a
frame as they stand.  What is new here is the frames spread's own walk: pme_recip_spread_frames has no sort; a workgroup per (frame,
brick of 4 x 4 x 16 points) walks the frame's atoms 256 at a time, keeps those whose cyclic stencil meets the brick (stencil_meets),
ranks them by ballot and the four waves' counts into 256 LDS slots and adds the slots up ("flushes") whenever filled + round > 256 and
at the end.  This module holds

  * meets and slot_walk: stencil_meets and the walk restated on the host -- for every (frame, brick) the kept atoms per round and per
    wave, and `filled` at every flush;
  * spread64_by_walk: the spread as the walk does it, in float64, and the options that build one of the walk's possible defects in;
  * the cases (CASES, sweep_case): batches of frames, frame m in BOX x (1 + m / 2), so that neighbouring frames never share a box; every
    named case reaches one event of the walk for brick TARGET_BRICK of its last frame, `stride` the second trip of the convolution.

tests/test_pme_frames_passes_reference_cpu.py checks this module on the host; tests/test_pme_frames_passes_gpu.py compares
capi.pme_reciprocal_frames_passes with it."""
import functools
import math

import numpy as np
import torch

import pme_recip_passes_reference as ref
from pme_recip_passes_reference import ALPHA, BOX, BRICK, COULOMB, MARGIN, SWEEP, charges, place, spme_energy  # noqa: F401

ROUND, WAVE = 256, 64                       # pme_recip_spread_frames: atoms per round = LDS slots, lanes per wave
WAVES = ROUND // WAVE

# The bars of tests/test_pme_frames_passes_gpu.py (per frame: max error / max reference of one pass fed with the device's own input;
# that file lists the measurements and checks that these are the same numbers).  The sensitivity tests are stated in them.
BAR_SPREAD = 1e-4
BAR_SCALED = 2e-6
BAR_CONVOLVE_ENERGY = 2e-6
BAR_INTERPOLATE = (7e-5, 1e-5)              # dE/dpositions, dE/dcharges


# ---- the walk -----------------------------------------------------------------------------------------------------------------------
def meets(g0, lo, hi, K, order, wrap_ahead=True, behind_inclusive=True):
    """stencil_meets of pme_frames.hip on an array of base indices: does the cyclic stencil [g0, g0 + order - 1] mod K meet the points
    [lo, hi]?  Either the brick's first point lies in the stencil (`ahead` < order) or the stencil's first point lies in the brick
    (`behind` <= hi - lo); a stencil as long as the axis meets everything.  The two options build a slip in:
      wrap_ahead=False        `ahead` = lo - g0 is not wrapped: a stencil that runs over the end of the axis does not come back
      behind_inclusive=False  `behind` < hi - lo: a stencil that starts on the brick's last point is left out"""
    g0 = np.asarray(g0)
    if order >= K:
        return np.ones(g0.shape, dtype=bool)
    ahead, behind = lo - g0, g0 - lo
    behind = np.where(behind < 0, behind + K, behind)
    if wrap_ahead:
        near = np.where(ahead < 0, ahead + K, ahead) < order
    else:
        near = (ahead >= 0) & (ahead < order)
    return near | ((behind <= hi - lo) if behind_inclusive else (behind < hi - lo))


def bricks_of(grid):
    """bricks per axis, and per axis the (lo, hi) points of every brick (the last one may be short)"""
    nb = [-(-grid[a] // BRICK[a]) for a in range(3)]
    return nb, [[(b * BRICK[a], min(b * BRICK[a] + BRICK[a], grid[a]) - 1) for b in range(nb[a])] for a in range(3)]


def kept_masks(base, grid, order, **how):
    """(brick, mask [n] of the atoms brick's workgroup keeps) for every brick of one frame, bricks in the kernel's order (z innermost)"""
    nb, bounds = bricks_of(grid)
    per_axis = [[meets(base[:, a], lo, hi, grid[a], order, **how) for lo, hi in bounds[a]] for a in range(3)]
    for bx in range(nb[0]):
        for by in range(nb[1]):
            both = per_axis[0][bx] & per_axis[1][by]
            for bz in range(nb[2]):
                yield (bx * nb[1] + by) * nb[2] + bz, both & per_axis[2][bz]


class Walk:
    """one workgroup's walk: waves[r][w] atoms kept by wave w in round r, flushes: `filled` at every flush inside the loop, final:
    `filled` when the frame is exhausted, last_slot: the highest slot written"""

    def __init__(self, keep):
        self.waves, self.flushes, filled, self.last_slot = [], [], 0, -1
        for c0 in range(0, len(keep), ROUND):
            chunk = keep[c0:c0 + ROUND]
            counts = [int(chunk[w * WAVE:(w + 1) * WAVE].sum()) for w in range(WAVES)]
            self.waves.append(counts)
            if filled + sum(counts) > ROUND:
                self.flushes.append(filled)
                filled = 0
            filled += sum(counts)
            if sum(counts):
                self.last_slot = max(self.last_slot, filled - 1)
        self.final = filled
        self.rounds = [sum(c) for c in self.waves]


def slot_walk(base, offsets, grid, order, **how):
    """{(frame, brick): Walk} for a batch: base [N, 3] integer base indices, offsets [B + 1]"""
    base = np.asarray(base)
    return {(m, brick): Walk(keep) for m, (a, b) in enumerate(zip(offsets, offsets[1:]))
            for brick, keep in kept_masks(base[a:b], grid, order, **how)}


def spread64_by_walk(pos, q, box, grid, order, coulomb, forget_on_flush=False, flush_drops_round=False, ranks_ignore_waves=False, **how):
    """The spread of one frame as pme_recip_spread_frames does it, in float64: every brick adds up, for its own points, the atoms its
    slots held at every flush and at the end.  Without options it equals spread64; the options build the defects in:
      forget_on_flush     a flush inside the loop resets `filled` without adding the slots
      flush_drops_round   the flush happens at filled + round >= 256 and the round that triggered it is not stored
      ranks_ignore_waves  slot = filled + rank inside the wave, without the earlier waves' counts: the waves write over each other (the
                          later wave stays) and the slots behind them keep what they held before (nothing, at first)
      **how               the options of meets"""
    K = list(grid)
    base, _, th, _ = ref.stencil(pos, box, grid, order)
    th = [torch.stack(t, 1) for t in th]                                # [N, order] per axis
    qs = q * math.sqrt(coulomb)
    slot_i = torch.arange(order)
    _, bounds = bricks_of(grid)
    nb = [len(b) for b in bounds]

    def axis_weight(points, atoms, a):
        dd = (points[None, :] - base[atoms, a][:, None]) % K[a]         # [atoms, points]
        return ((slot_i[None, None, :] % K[a] == dd[:, :, None]) * th[a][atoms][:, None, :]).sum(-1)

    Q = torch.zeros(K[0], K[1], K[2], dtype=torch.float64)
    for brick, keep in kept_masks(base.numpy(), grid, order, **how):
        slots, filled, added = np.full(ROUND, -1), 0, []
        for c0 in range(0, len(keep), ROUND):
            lanes = np.nonzero(keep[c0:c0 + ROUND])[0]
            if filled + len(lanes) >= ROUND if flush_drops_round else filled + len(lanes) > ROUND:
                if not forget_on_flush:
                    added.append(slots[:filled].copy())
                filled = 0
                if flush_drops_round:
                    continue
            if ranks_ignore_waves:
                for w in range(WAVES):
                    mine = lanes[lanes // WAVE == w]
                    slots[filled:filled + len(mine)] = c0 + mine
            else:
                slots[filled:filled + len(lanes)] = c0 + lanes
            filled += len(lanes)
        added.append(slots[:filled].copy())
        atoms = np.concatenate(added)
        atoms = torch.as_tensor(atoms[atoms >= 0], dtype=torch.long)
        if len(atoms) == 0:
            continue
        bz, by, bx = brick % nb[2], (brick // nb[2]) % nb[1], brick // (nb[2] * nb[1])
        px, py, pz = (torch.arange(lo, hi + 1) for lo, hi in (bounds[0][bx], bounds[1][by], bounds[2][bz]))
        wx = axis_weight(px, atoms, 0) * qs[atoms][:, None]
        Q[px[0]:px[-1] + 1, py[0]:py[-1] + 1, pz[0]:pz[-1] + 1] = torch.einsum("mx,my,mz->xyz", wx, axis_weight(py, atoms, 1),
                                                                               axis_weight(pz, atoms, 2))
    return Q


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
EVENT_GRID = (16, 16, 32)
TARGET_BRICK = (1 * 4 + 1) * 2 + 0          # brick (1, 1, 0) of EVENT_GRID: the points x, y in [4, 8), z in [0, 16)
WHERE = {
    "any": {},
    "in": {"lo": (4 / 16, 4 / 16, 0.0), "hi": (8 / 16, 8 / 16, 16 / 32)},       # base index inside the target brick: always kept
    "far": {"lo": (8 / 16, 0.0, 0.0), "hi": (1.0, 1.0, 1.0)},                   # x base in [8, 16): orders 4 and 5 never reach x in [4, 8)
}


def scale_of(m):
    return 1.0 + 0.5 * m


def _frame(rng, grid, rounds, scale):
    """positions (in BOX x scale) and charges of one frame.  rounds: an atom count (anywhere in the box) or a list of (segments,
    shuffle): segments = [(count, where), ...] in atom order, shuffled inside the round when `shuffle` (uneven counts per wave)"""
    if isinstance(rounds, int):
        rounds = [([(rounds, "any")], False)] if rounds else []
    parts = []
    for segments, shuffle in rounds:
        p = np.concatenate([place(rng, n, grid, **WHERE[w]) for n, w in segments])
        parts.append(p[rng.permutation(len(p))] if shuffle else p)
    pos = np.concatenate(parts) * scale if parts else np.zeros((0, 3))
    return pos, charges(rng, len(pos)) if len(pos) else np.zeros(0)


def _batch(name, grid, order, seed, frames):
    rng = np.random.default_rng(seed)
    made = [_frame(rng, grid, rounds, scale_of(m)) for m, rounds in enumerate(frames)]
    offsets = [0]
    for p, _ in made:
        offsets.append(offsets[-1] + len(p))
    return {"name": name, "grid": tuple(grid), "order": order, "offsets": offsets,
            "pos": np.concatenate([p for p, _ in made]).astype(np.float32), "q": np.concatenate([c for _, c in made]).astype(np.float32),
            "boxes": np.stack([BOX * scale_of(m) for m in range(len(made))]).astype(np.float32)}


# the last frame of every event case, round by round (what TARGET_BRICK keeps: the "in" atoms)
PARTIAL_FLUSH = [([(250, "in"), (6, "far")], True), ([(44, "in")], False)]                       # 300 atoms: a flush at filled = 250
EXACT_FILL = [([(200, "in"), (56, "far")], True), ([(56, "in"), (200, "far")], True)]            # 512 atoms: 200 + 56, no flush
THREE_FLUSHES = [([(230, "in"), (26, "far")], True)] * 3 + [([(32, "in")], False)]               # 800 atoms: flushes at 230, 230, 230
EMPTY_ROUND = [([(100, "in"), (156, "far")], True), ([(256, "far")], False), ([(50, "in")], False)]
IDLE_WAVE = [([(64, "in"), (64, "far"), (30, "in"), (54, "far"), (44, "in")], False)]            # waves keep 64, 0, 30, 44

CASES = {
    # (a 7-atom frame and an empty one first: the big frame's atoms do not start at a multiple of 256 for the per-atom kernels)
    "partial-flush": lambda: _batch("partial-flush", EVENT_GRID, 5, 301, [7, 0, PARTIAL_FLUSH]),
    "partial-flush-4": lambda: _batch("partial-flush-4", EVENT_GRID, 4, 302, [7, 0, PARTIAL_FLUSH]),
    "exact-fill": lambda: _batch("exact-fill", EVENT_GRID, 5, 303, [5, EXACT_FILL]),
    "three-flushes": lambda: _batch("three-flushes", EVENT_GRID, 5, 304, [9, THREE_FLUSHES]),
    "empty-round": lambda: _batch("empty-round", EVENT_GRID, 5, 305, [3, EMPTY_ROUND]),
    "idle-wave": lambda: _batch("idle-wave", EVENT_GRID, 5, 306, [11, IDLE_WAVE]),
    "stride-4": lambda: _batch("stride-4", (72, 68, 120), 4, 307, [300, 40]),
    "stride-5": lambda: _batch("stride-5", (72, 68, 120), 5, 308, [300, 40]),
}
CASE_NAMES = list(CASES)
LOOP_CASES = ["partial-flush", "partial-flush-4", "three-flushes", "stride-4", "stride-5"]      # judged end to end as well
CONVOLVE_PASS = ref.CONVOLVE_PASS           # complex points per trip of the convolution's capped stride (1024 workgroups x 256 lanes)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def sweep_case(grid, order):
    return _batch(f"sweep-{order}-{grid}", grid, order, 400 + 7 * sum(grid) + order, [20, 0, 60])


def frames_of(c):
    """[(m, first atom, end atom)] of a batch"""
    return [(m, a, b) for m, (a, b) in enumerate(zip(c["offsets"], c["offsets"][1:]))]


def frame_case(c, m):
    """frame m of a batch as a single-system case of pme_recip_passes_reference (case64, moduli, smallest_atom_at_a_point take it)"""
    a, b = c["offsets"][m], c["offsets"][m + 1]
    return {"name": f"{c['name']}[{m}]", "pos": c["pos"][a:b], "q": c["q"][a:b], "box": c["boxes"][m], "grid": c["grid"], "order": c["order"]}


def moduli(c):
    return ref.moduli(c)


def has_a_float64_energy(c):
    """False for a grid with a one-point axis: the B-spline modulus of a single point is exactly 0 (bspline_moduli has no neighbour to
    mend it from), so smooth PME's energy is infinite in float64 as well and only the spread can be judged"""
    return all(float(m.min()) > 0 for m in moduli(c))


def base_of(c):
    """the float64 base indices [N, 3] (numpy) of a batch, and the smallest distance of a grid coordinate from a cell edge, in cells"""
    base, margin = np.zeros((len(c["q"]), 3), dtype=np.int64), 0.5
    for m, a, b in frames_of(c):
        if b > a:
            pos, _, box = ref.case64(frame_case(c, m))
            g0, dr, _, _ = ref.stencil(pos, box, c["grid"], c["order"])
            base[a:b] = g0.numpy()
            margin = min(margin, float(torch.minimum(dr, 1 - dr).min()))
    return base, margin


@functools.lru_cache(maxsize=None)
def walk_of(name):
    c = case(name)
    return slot_walk(base_of(c)[0], c["offsets"], c["grid"], c["order"])


def spread_frames64(c):
    """spread64 of every frame: [B, Kx, Ky, Kz] float64 (an empty frame: zeros)"""
    out = torch.zeros(len(c["offsets"]) - 1, *c["grid"], dtype=torch.float64)
    for m, a, b in frames_of(c):
        if b > a:
            out[m] = ref.spread64(*ref.case64(frame_case(c, m)), c["grid"], c["order"], COULOMB)
    return out


@functools.lru_cache(maxsize=None)
def spread_of(name):
    return spread_frames64(case(name))


def autograd_frames64(c):
    """(energies [B], dE/dpositions [N, 3], dE/dcharges [N], dE/dboxes [B, 3, 3]) by autograd of spme_energy with every frame's own
    box as a leaf; zeros for an empty frame"""
    B, n = len(c["offsets"]) - 1, len(c["q"])
    e, gp, gq, gb = (torch.zeros(s, dtype=torch.float64) for s in ((B,), (n, 3), (n,), (B, 3, 3)))
    for m, a, b in frames_of(c):
        if b > a:
            f = frame_case(c, m)
            pos, q, box = (t.requires_grad_() for t in ref.case64(f))
            em = spme_energy(pos, q, box, c["grid"], c["order"], ALPHA, COULOMB, moduli(c))
            gp[a:b], gq[a:b], gb[m] = torch.autograd.grad(em, (pos, q, box))
            e[m] = em.detach()
    return e, gp, gq, gb


@functools.lru_cache(maxsize=None)
def autograd_of(name):
    return autograd_frames64(case(name))
