"""The float64 judge of CFConv periodic batches (no GPU code, no tests; importable anywhere) and the batches it is asked about.

A periodic batch is B frames behind one neighbour list (nnpops_cfconv_neighbors_set_frames): positions [sum n_m][3], B + 1 offsets
and boxes [B][3][3], frame m = atoms [offsets[m], offsets[m + 1]) in the box boxes[m] of its own.  The judge knows nothing about
batches: it asks `Restatement.evaluate(pos[lo:hi], boxes[m], ...)` of tests/cfconv_float64.py -- and `SecondOrder.periodic` for the
second-order cases -- about ONE frame at a time and concatenates what they return, the box gradient `gbox` [B][3][3] included.  A
frame of one atom has no pair and gets exact zeros.

Batches (cutoff 3 A; every frame's first seed, counted up from the one written here, at which its conditions hold):
    ragged    frames of 1, 2, 21, 64, 65 and 7 atoms, every one brought to the origin (its box centre subtracted) so that the frames
              lie on top of each other: an empty row, an exactly full wave of candidates, one candidate more than a wave.  Boxes of
              their own, perpendicular widths 2.12 to 3.9 cutoffs (6.35 A to 12 A: nearly a factor of two); the 65-atom box is
              triclinic; the 64-atom frame is moved 0.37 box lengths along x and wrapped back (box_gradient_judge.moved_frames), the
              65-atom frame moved and NOT wrapped (a third of its atoms a box vector outside); the two atoms of the pair stand on
              either side of a box face
    many      70 frames of 1 ... 9 atoms, clusters astride a corner of boxes of their own, every third box triclinic
    crowded   190 atoms at 0.7 atoms / A^3 beside frames of 5 and 12 atoms: rows of more than 64 entries, beyond the first capacity
    long      257 atoms beside 3: the per-frame stride of the box pass (64 workgroups x 4 waves = 256 atoms) goes round a second time.
              The one atom of that round is the frame's last and owns no pair (a pair belongs to its lower index), so a frame of 300
              atoms follows: its atoms 256 ... 299 own shifted pairs among themselves, summed in the second round
Conditions on every frame (tests/test_cfconv_frames_reference_cpu.py pins them): every box at least 2.1 cutoffs wide between
opposite faces; no intra-frame minimum-image distance within 1e-4 of the cutoff; at least one pair in every frame of two atoms or
more; shifted pairs on every axis in every frame of 21 atoms or more.
"""
import functools

import numpy as np

from ani_periodic_batch_float64 import _corner_cluster, _wrapped
from box_gradient_judge import moved_frames
from cfconv_float64 import Restatement, SecondOrder, cotangents, sigma_of, weights
from nnpops_amd import workloads

CUTOFF = 3.0
NEAR = 1e-4                                 # no intra-frame minimum-image distance is this close to the cutoff
MIN_WIDTH = 2.1                             # cutoffs between opposite faces of every box
RAGGED = (1, 2, 21, 64, 65, 7)
MANY = 70
CROWDED = (5, 190, 12)
CROWDED_DENSITY = 0.7
LONG = (257, 3, 300)
BOX_STRIDE = 256                            # atoms per round of a frame's box pass: kConvBoxFrameBlocks x kConvBoxWaves (cfconv_box_grad.h)
SEEDS = {"ragged": 2100, "many": 2300, "crowded": 2500, "long": 2700}     # frame k of a batch starts counting at SEEDS[tag] + 10 k
TAGS = tuple(SEEDS)

_LISTER = Restatement(1, 2, CUTOFF, 0.4, "ssp", np.zeros((1, 2)), np.zeros(1), np.zeros((1, 1)), np.zeros(1))


# ---------------------------------------------------------------------------------------------- geometry
def widths(box):
    """perpendicular widths of a box (rows = vectors): the distances between its three pairs of opposite faces"""
    B = np.asarray(box, np.float64).reshape(3, 3)
    V = abs(np.linalg.det(B))
    return np.array([V / np.linalg.norm(np.cross(B[(k + 1) % 3], B[(k + 2) % 3])) for k in range(3)])


def frame_pairs(pos, box, cutoff=CUTOFF):
    """-> (i, j, n) of one frame's half list by the restatement's rule (float64 on the float32 inputs); a lone atom has none"""
    if len(pos) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3))
    lister = _LISTER if cutoff == CUTOFF else Restatement(1, 2, cutoff, 0.4, "ssp", np.zeros((1, 2)), np.zeros(1), np.zeros((1, 1)), np.zeros(1))
    return lister.pairs(np.asarray(pos, np.float32).astype(np.float64), np.asarray(box, np.float32).astype(np.float64).reshape(3, 3))


def frame_margin(pos, box, cutoff=CUTOFF):
    """the smallest |r - cutoff| over every pair of the frame under the restatement's minimum image, listed or not"""
    p, B = np.asarray(pos, np.float32).astype(np.float64), np.asarray(box, np.float32).astype(np.float64).reshape(3, 3)
    best = np.inf
    for i in range(len(p) - 1):
        d = p[i + 1:] - p[i]
        for k in (2, 1, 0):
            d = d - np.round(d[:, k] / B[k, k])[:, None] * B[k]
        best = min(best, float(np.abs(np.sqrt((d * d).sum(1)) - float(np.float32(cutoff))).min()))
    return best


def census(pos, box, cutoff=CUTOFF):
    """-> dict(pairs, per_axis [3] shifted pairs, longest row, margin, widths in cutoffs) of one frame"""
    i, j, n = frame_pairs(pos, box, cutoff)
    rows = np.bincount(np.concatenate([i, j]).astype(np.int64), minlength=len(pos))
    return dict(pairs=len(i), per_axis=[int((n[:, a] != 0).sum()) for a in range(3)], row=int(rows.max()), margin=frame_margin(pos, box, cutoff),
                widths=widths(box) / float(np.float32(cutoff)))


def _acceptable(pos, box):
    c = census(pos, box)
    return (c["widths"].min() >= MIN_WIDTH and c["margin"] > NEAR and (len(pos) < 2 or c["pairs"] > 0)
            and (len(pos) < 21 or min(c["per_axis"]) > 0))


def _tilted(L):
    return np.array([[L, 0, 0], [0.15 * L, L, 0], [-0.05 * L, -0.1 * L, L]], dtype=np.float32)


def _liquid(n, L, seed, triclinic=False, moved=None, density=None):
    """n atoms of workloads' lattice gas in a cube of side L (or at `density`); moved "wrapped" / "shifted": box_gradient_judge.moved_frames"""
    pos, _, box = workloads.random_box(n, density=n / L ** 3 if density is None else density, seed=seed)
    if triclinic:
        box = _tilted(float(box[0, 0]))
    if moved is not None:
        pos = moved_frames(pos, box)[1 if moved == "wrapped" else 0]
    return pos.astype(np.float32), np.asarray(box, np.float32)


def _cluster(n, seed, triclinic):
    """a cluster of n atoms astride a corner of a box of its own (diagonal entries 6.4 .. 8.5 A, one axis in three 1.4 times that)"""
    rng = np.random.default_rng(seed)
    lx, ly, lz = rng.uniform(6.4, 8.5, 3) * rng.choice([1.0, 1.0, 1.4], 3)
    box = (np.array([[lx, 0, 0], [0.15 * lx, ly, 0], [-0.05 * lx, -0.1 * ly, lz]]) if triclinic else np.diag([lx, ly, lz])).astype(np.float32)
    return _wrapped(_corner_cluster(n, rng), box), box


def _across_a_face(seed):
    """two atoms on either side of the x face of a cubic 7 A box, about 1 A apart through it"""
    rng = np.random.default_rng(seed)
    L = 7.0
    pos = np.array([[0.4, 3.0, 3.0], [L - 0.5, 3.3, 2.8]]) + rng.uniform(-0.1, 0.1, (2, 3))
    return pos.astype(np.float32), (np.eye(3) * L).astype(np.float32)


def _first(make, seed):
    """the first seed, counted up from `seed`, at which the frame meets the conditions -> (pos, box, seed)"""
    for s in range(seed, seed + 10):
        try:
            pos, box = make(s)
        except AssertionError:                              # (moved_frames: too few or too many atoms beyond the face)
            continue
        if _acceptable(pos, box):
            return pos, box, s
    raise RuntimeError(f"no acceptable frame within ten seeds of {seed}")


def _centred(pos, box):
    """the frame brought to the origin: half of every box vector subtracted (float32 positions of their own; the frame then lies
    outside its box on the negative side, unwrapped, and on top of the other frames of its batch)"""
    return (pos.astype(np.float64) - 0.5 * box.astype(np.float64).sum(axis=0)).astype(np.float32)


def _makers(tag):
    if tag == "ragged":
        return [lambda s: _liquid(1, 6.4, s), _across_a_face, lambda s: _liquid(21, 6.35, s),
                lambda s: _liquid(64, 8.0, s, moved="wrapped"), lambda s: _liquid(65, 12.0, s, triclinic=True, moved="shifted"),
                lambda s: _liquid(7, 9.0, s)]
    if tag == "many":
        return [functools.partial(lambda s, m: _cluster(1 + m % 9, s, m % 3 == 1), m=m) for m in range(MANY)]
    if tag == "crowded":
        return [lambda s: _cluster(CROWDED[0], s, False), lambda s: _liquid(CROWDED[1], 0.0, s, density=CROWDED_DENSITY),
                lambda s: _cluster(CROWDED[2], s, True)]
    if tag == "long":
        return [lambda s: _liquid(LONG[0], 12.0, s), lambda s: _cluster(LONG[1], s, True), lambda s: _liquid(LONG[2], 12.6, s, triclinic=True)]
    raise KeyError(tag)


@functools.lru_cache(maxsize=None)
def batch(tag):
    """-> (positions [N][3] float32, boxes [B][3][3] float32, offsets [B + 1] int32, seeds): built once and read-only"""
    parts, seeds = [], []
    for k, make in enumerate(_makers(tag)):
        pos, box, seed = _first(make, SEEDS[tag] + 10 * k)
        if tag == "ragged":
            pos = _centred(pos, box)
            assert _acceptable(pos, box), (tag, k)
        parts.append((pos, box)); seeds.append(seed)
    pos = np.concatenate([p for p, _ in parts]).astype(np.float32)
    boxes = np.stack([b for _, b in parts]).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p, _ in parts])]).astype(np.int32)
    for a in (pos, boxes, offsets):
        a.setflags(write=False)
    return pos, boxes, offsets, tuple(seeds)


def segments(offsets):
    return [(int(lo), int(hi)) for lo, hi in zip(offsets[:-1], offsets[1:])]


def reorder(pos, boxes, offsets, order, *per_atom):
    """the frames in another order -> (pos, boxes, offsets, rows, per-atom arrays...): rows[k] = the old index of new atom k"""
    segs = segments(offsets)
    rows = np.concatenate([np.arange(*segs[m]) for m in order])
    new_offsets = np.concatenate([[0], np.cumsum([segs[m][1] - segs[m][0] for m in order])]).astype(np.int32)
    return (np.ascontiguousarray(pos[rows]), np.ascontiguousarray(boxes[list(order)]), new_offsets, rows) + tuple(np.ascontiguousarray(a[rows]) for a in per_atom)


# ---------------------------------------------------------------------------------------------- lists
def half_pairs(pos, boxes, offsets, cutoff=CUTOFF):
    """-> (i, j, d [P][3] float64, n [P][3]) of the batch's half list: every frame's own list under its own box, one behind the other"""
    out = [[], [], [], []]
    for m, (lo, hi) in enumerate(segments(offsets)):
        i, j, n = frame_pairs(pos[lo:hi], boxes[m], cutoff)
        p, B = pos[lo:hi].astype(np.float64), boxes[m].astype(np.float64)
        for k, v in enumerate((i + lo, j + lo, (p[j] - p[i] + n @ B).reshape(-1, 3), n.reshape(-1, 3))):
            out[k].append(v)
    return tuple(np.concatenate(v) for v in out)


def pair_set(i, j):
    return set(zip((int(v) for v in i), (int(v) for v in j)))


# ---------------------------------------------------------------------------------------------- layers and the judge
def batch_layer(tag, W, G):
    """-> (w1, b1, w2, b2, x, gout, V, Q) of a layer on a batch, seeded by the shape"""
    n = len(batch(tag)[0])
    return weights(W, G, n, 5000 * W + G) + cotangents(n, W, 6000 * W + G)


def judge_of(tag, W, G, act, cutoff=CUTOFF):
    w1, b1, w2, b2 = batch_layer(tag, W, G)[:4]
    return Restatement(W, G, cutoff, sigma_of(G), act, w1, b1, w2, b2)


def evaluate(judge, pos, boxes, offsets, x, gout):
    """Restatement.evaluate frame by frame, each in its own box -> dict(out, gx, g, gbox [B][3][3], i, j, n), concatenated"""
    W = judge.W
    out, gx, g = (np.zeros((len(pos), k)) for k in (W, W, 3))
    gbox = np.zeros((len(offsets) - 1, 3, 3))
    pi, pj, pn = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, 3))]
    for m, (lo, hi) in enumerate(segments(offsets)):
        if hi - lo < 2:
            continue
        r = judge.evaluate(pos[lo:hi], boxes[m], x[lo:hi], gout[lo:hi])
        out[lo:hi], gx[lo:hi], g[lo:hi], gbox[m] = r["out"], r["gx"], r["g"], r["gbox"]
        pi.append(r["i"] + lo); pj.append(r["j"] + lo); pn.append(r["n"].reshape(-1, 3))
    return dict(out=out, gx=gx, g=g, gbox=gbox, i=np.concatenate(pi), j=np.concatenate(pj), n=np.concatenate(pn))


def second(judge, pos, boxes, offsets, x, gout, V, Q):
    """SecondOrder.periodic(...).second frame by frame -> dict(dg, dx, dp), concatenated"""
    W = judge.W
    res = dict(dg=np.zeros((len(pos), W)), dx=np.zeros((len(pos), W)), dp=np.zeros((len(pos), 3)))
    for m, (lo, hi) in enumerate(segments(offsets)):
        if hi - lo < 2:
            continue
        so = SecondOrder.periodic(judge, pos[lo:hi], boxes[m])
        if len(so.i) == 0:
            continue
        r = so.second(pos[lo:hi], x[lo:hi], gout[lo:hi], V[lo:hi], Q[lo:hi])
        for k in res:
            res[k][lo:hi] = r[k]
    return res


_REFERENCES = {}


def reference(tag, W, G, act):
    """float64 once per (batch, layer): dict(out, gx, g, gbox, i, j, n) for the layer's x and gout"""
    key = (tag, W, G, act)
    if key not in _REFERENCES:
        pos, boxes, offsets, _ = batch(tag)
        x, gout = batch_layer(tag, W, G)[4:6]
        _REFERENCES[key] = evaluate(judge_of(tag, W, G, act), pos, boxes, offsets, x, gout)
    return _REFERENCES[key]


def stress_antisymmetry(pos, boxes, offsets, g, gbox):
    """per frame: (largest entry of the antisymmetric part of W_m = x_m^T g_m + B_m^T dB_m, largest entry of W_m)"""
    out = []
    for m, (lo, hi) in enumerate(segments(offsets)):
        x, B = pos[lo:hi].astype(np.float64), boxes[m].astype(np.float64)
        Wm = x.T @ np.asarray(g[lo:hi], np.float64) + B.T @ np.asarray(gbox[m], np.float64)
        out.append((float(np.abs(Wm - Wm.T).max()) / 2, float(np.abs(Wm).max())))
    return out
