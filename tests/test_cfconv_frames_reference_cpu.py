"""CFConv periodic batches without a GPU: the batches of tests/cfconv_frames_float64.py are pinned to the edges they are named for, the
judge to the single-frame Restatement, to central differences of itself and to the float32 oracle, and the library, the torch holder
and the module are shown to have the new entry points (the last three tests fail before nnpops_cfconv_neighbors_set_frames)."""
import ctypes
import itertools

import numpy as np
import pytest

import cfconv_frames_float64 as frames
from cfconv_float64 import FORCE_RTOL, OUT_ATOL_FRAC, OUT_RTOL, Restatement, sigma_of

FD_RTOL = 1e-6                                   # tests/test_cfconv_box_gradient_reference_cpu.py


# ---------------------------------------------------------------------------------------------- the batches
def test_shapes_of_the_batches():
    assert tuple(np.diff(frames.batch("ragged")[2])) == frames.RAGGED == (1, 2, 21, 64, 65, 7)
    sizes = np.diff(frames.batch("many")[2])
    assert len(sizes) == 70 and sizes.min() == 1 and sizes.max() == 9
    assert tuple(np.diff(frames.batch("crowded")[2])) == frames.CROWDED
    assert tuple(np.diff(frames.batch("long")[2])) == frames.LONG and frames.LONG[0] == frames.BOX_STRIDE + 1 and frames.LONG[2] > frames.BOX_STRIDE + 1
    for tag in frames.TAGS:
        pos, boxes, offsets, seeds = frames.batch(tag)
        assert boxes.shape == (len(offsets) - 1, 3, 3) and offsets[-1] == len(pos) and pos.dtype == boxes.dtype == np.float32
        assert all(0 <= s - (frames.SEEDS[tag] + 10 * k) < 10 for k, s in enumerate(seeds))
        assert np.array_equal(np.triu(boxes, 1), np.zeros_like(boxes))                  # reduced form: lower triangular


@pytest.mark.parametrize("tag", frames.TAGS)
def test_conditions_on_every_frame(tag):
    pos, boxes, offsets, _ = frames.batch(tag)
    worst_margin, narrowest = np.inf, np.inf
    for m, (lo, hi) in enumerate(frames.segments(offsets)):
        c = frames.census(pos[lo:hi], boxes[m])
        assert c["widths"].min() >= frames.MIN_WIDTH, (tag, m, c["widths"])
        assert c["margin"] > frames.NEAR, (tag, m, c["margin"])
        assert hi - lo < 2 or c["pairs"] > 0, (tag, m)
        assert hi - lo < 21 or min(c["per_axis"]) > 0, (tag, m, c["per_axis"])
        worst_margin, narrowest = min(worst_margin, c["margin"]), min(narrowest, c["widths"].min())
    print(f"\n[cfconv-frames] {tag}: {len(offsets) - 1} frames, {len(pos)} atoms, smallest |r - cutoff| {worst_margin:.2e} A, narrowest box "
          f"{narrowest:.3f} cutoffs")


def test_ragged_boxes_and_placements():
    pos, boxes, offsets, _ = frames.batch("ragged")
    segs = frames.segments(offsets)
    w = np.array([frames.widths(b) / frames.CUTOFF for b in boxes])
    assert 2.1 <= w.min() < 2.2 and 3.8 < w.max() <= 4.05 and w.max() / w.min() > 1.8      # nearly a factor of two
    assert np.abs(np.tril(boxes[4], -1)).max() > 0 and not np.abs(np.tril(boxes[[0, 1, 2, 3, 5]], -1)).any()      # one triclinic box
    # every frame reaches across the origin, so the frames lie on top of each other
    for lo, hi in segs[2:5]:
        assert (pos[lo:hi].min(axis=0) < -1.0).all() and (pos[lo:hi].max(axis=0) > 1.0).all()
    for (lo, hi), b in zip(segs, boxes):
        assert np.abs(pos[lo:hi]).max() < 1.5 * np.abs(b).max()
    # the 64-atom frame is wrapped: with the box centre added back every atom lies inside [0, L); the 65-atom frame is not: a quarter
    # to half of its atoms lie beyond the x face
    lo, hi = segs[3]
    back = pos[lo:hi].astype(np.float64) + 0.5 * boxes[3].astype(np.float64).sum(axis=0)
    assert (back > -1e-5).all() and (back < float(boxes[3][0, 0]) + 1e-5).all()
    lo, hi = segs[4]
    back = pos[lo:hi].astype(np.float64) + 0.5 * boxes[4].astype(np.float64).sum(axis=0)
    assert 0.25 < float((back[:, 0] > float(boxes[4][0, 0])).mean()) < 0.45
    # the pair of the two-atom frame goes through a face
    i, j, n = frames.frame_pairs(pos[segs[1][0]:segs[1][1]], boxes[1])
    assert len(i) == 1 and np.abs(n).sum() == 1


def test_rows_and_rounds():
    pos, boxes, offsets, _ = frames.batch("crowded")
    lo, hi = frames.segments(offsets)[1]
    row = frames.census(pos[lo:hi], boxes[1])["row"]
    assert 64 < row <= 128, row                                             # one doubling of the row capacity
    # long: atoms beyond the first round of the box pass own shifted pairs in the 300-atom frame
    pos, boxes, offsets, _ = frames.batch("long")
    lo, hi = frames.segments(offsets)[2]
    i, j, n = frames.frame_pairs(pos[lo:hi], boxes[2])
    late = (i >= frames.BOX_STRIDE) & (np.abs(n).sum(axis=1) > 0)
    assert late.sum() > 10, int(late.sum())


@pytest.mark.parametrize("tag", ["ragged", "many"])
def test_single_round_rule_finds_the_nearest_image(tag):
    """every box is wide enough for the single-round rule: the pairs it lists are those of a search over 27 images"""
    pos, boxes, offsets, _ = frames.batch(tag)
    images = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.float64)
    for m, (lo, hi) in enumerate(frames.segments(offsets)):
        p, B = pos[lo:hi].astype(np.float64), boxes[m].astype(np.float64)
        d = p[None, :, None, :] - p[:, None, None, :] + (images @ B)[None, None]
        r = np.sqrt((d * d).sum(-1)).min(axis=-1)
        bi, bj = np.nonzero(np.triu(r < frames.CUTOFF, 1))
        i, j, _ = frames.frame_pairs(pos[lo:hi], boxes[m])
        assert frames.pair_set(i, j) == frames.pair_set(bi, bj), (tag, m)


# ---------------------------------------------------------------------------------------------- what a wrong builder would give
def test_ignoring_the_offsets_gives_another_list():
    """the list of ONE system under frame 0's box over all the atoms: pairs between frames (they lie on top of each other)"""
    pos, boxes, offsets, _ = frames.batch("ragged")
    i, j, _, _ = frames.half_pairs(pos, boxes, offsets)
    wi, wj, _ = frames.frame_pairs(pos, boxes[0])
    frame_of = np.searchsorted(offsets, np.arange(len(pos)), side="right") - 1
    assert (frame_of[i] == frame_of[j]).all()
    cross = frame_of[wi] != frame_of[wj]
    assert cross.sum() > 500 and frames.pair_set(i, j) != frames.pair_set(wi, wj)


def test_one_box_for_every_frame_gives_another_list():
    """the frames kept apart but every one of them under frame 0's box (6.4 A): other pairs and other shifts"""
    pos, boxes, offsets, _ = frames.batch("ragged")
    i, j, _, n = frames.half_pairs(pos, boxes, offsets)
    same = np.broadcast_to(boxes[0], boxes.shape)
    wi, wj, _, wn = frames.half_pairs(pos, same, offsets)
    assert frames.pair_set(i, j) != frames.pair_set(wi, wj)
    assert len(wi) > len(i) + 100                                          # the larger frames folded into the small box
    # ... and under the LAST frame's box (9 A) the 21-atom frame loses its pairs through the faces
    lo, hi = frames.segments(offsets)[2]
    a = frames.frame_pairs(pos[lo:hi], boxes[2])
    b = frames.frame_pairs(pos[lo:hi], boxes[5])
    assert len(b[0]) < len(a[0]) and not np.array_equal(a[2][:len(b[2])], b[2])


# ---------------------------------------------------------------------------------------------- the judge
def test_a_batch_of_one_frame_is_the_restatement():
    pos, boxes, offsets, _ = frames.batch("ragged")
    W, G = 16, 8
    w1, b1, w2, b2, x, gout, V, Q = frames.batch_layer("ragged", W, G)
    judge = frames.judge_of("ragged", W, G, "ssp")
    lo, hi = frames.segments(offsets)[3]
    one = np.array([0, hi - lo], np.int32)
    got = frames.evaluate(judge, pos[lo:hi], boxes[3:4], one, x[lo:hi], gout[lo:hi])
    ref = judge.evaluate(pos[lo:hi], boxes[3], x[lo:hi], gout[lo:hi])
    for k in ("out", "gx", "g", "i", "j", "n"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["gbox"][0], ref["gbox"]) and np.abs(ref["gbox"]).min() > 0
    whole = frames.reference("ragged", W, G, "ssp")
    assert np.array_equal(whole["out"][lo:hi], ref["out"]) and np.array_equal(whole["gbox"][3], ref["gbox"])
    assert not whole["out"][0].any() and not whole["gbox"][0].any()        # the lone atom: exact zeros
    # the two-atom frame: its one pair goes through the x face, so only the first row of its box gradient is set
    assert np.abs(whole["gbox"][1][0]).max() > 0 and not whole["gbox"][1][1:].any()


def test_box_gradient_of_a_frame_against_central_differences():
    """all nine entries of the judge's per-frame gbox, on the 21-atom frame of `ragged` (a box 2.12 cutoffs wide)"""
    pos, boxes, offsets, _ = frames.batch("ragged")
    W, G = 8, 6
    w1, b1, w2, b2, x, gout, _, _ = frames.batch_layer("ragged", W, G)
    judge = Restatement(W, G, frames.CUTOFF, 0.5, "ssp", w1, b1, w2, b2)
    lo, hi = frames.segments(offsets)[2]
    base = frames.evaluate(judge, pos, boxes, offsets, x, gout)
    mine = (base["i"] >= lo) & (base["i"] < hi)
    pos64, box64 = pos[lo:hi].astype(np.float64), boxes[2].astype(np.float64)

    def energy(b):
        L, (pi, pj, pn) = judge.energy(pos64, b, x[lo:hi], gout[lo:hi])
        assert np.array_equal(pi + lo, base["i"][mine]) and np.array_equal(pj + lo, base["j"][mine]) and np.array_equal(pn, base["n"][mine])
        return L

    worst, top = 0.0, np.abs(base["gbox"][2]).max()
    for k in range(3):
        for c in range(3):
            def central(h):
                plus, minus = box64.copy(), box64.copy()
                plus[k, c] += h; minus[k, c] -= h
                return (energy(plus) - energy(minus)) / (2 * h)
            fd = (4.0 * central(2.0 ** -15) - central(2.0 ** -14)) / 3.0
            worst = max(worst, abs(fd - base["gbox"][2][k, c]))
    print(f"\n[cfconv-frames] 21-atom frame: box gradient vs central differences {worst / top:.2e} of max {top:.3e}")
    assert top > 0 and worst <= FD_RTOL * top


def test_float32_oracle_within_half_the_bar():
    """the float32 CPU oracle, frame by frame in the frame's own box, against the judge: half the bars of the GPU tests"""
    from oracle import CFConvNeighborsOracle, CFConvOracle
    pos, boxes, offsets, _ = frames.batch("ragged")
    W, G, act = 12, 9, "tanh"
    w1, b1, w2, b2, x, gout, _, _ = frames.batch_layer("ragged", W, G)
    ref = frames.reference("ragged", W, G, act)
    got_out, got_gx, got_g = np.zeros_like(ref["out"]), np.zeros_like(ref["gx"]), np.zeros_like(ref["g"])
    for m, (lo, hi) in enumerate(frames.segments(offsets)):
        n = hi - lo
        onb = CFConvNeighborsOracle(n, frames.CUTOFF, True)
        onb.build(np.ascontiguousarray(pos[lo:hi]), np.ascontiguousarray(boxes[m]))
        ocf = CFConvOracle(n, W, G, frames.CUTOFF, sigma_of(G), act, w1, b1, w2, b2, periodic=True)
        got_out[lo:hi] = ocf.forward(onb, np.ascontiguousarray(pos[lo:hi]), np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(boxes[m]))
        xg, pg = ocf.backward(onb, np.ascontiguousarray(pos[lo:hi]), np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(gout[lo:hi]),
                              np.ascontiguousarray(boxes[m]))
        got_gx[lo:hi], got_g[lo:hi] = xg, pg
    np.testing.assert_allclose(got_out, ref["out"], rtol=OUT_RTOL / 2, atol=OUT_ATOL_FRAC / 2 * np.abs(ref["out"]).max())
    np.testing.assert_allclose(got_gx, ref["gx"], rtol=OUT_RTOL / 2, atol=OUT_ATOL_FRAC / 2 * np.abs(ref["gx"]).max())
    err = np.abs(got_g - ref["g"]).max() / np.abs(ref["g"]).max()
    print(f"\n[cfconv-frames] float32 oracle, frame by frame: position gradient {err:.2e} of max")
    assert err <= FORCE_RTOL / 2


# ---------------------------------------------------------------------------------------------- the new entry points exist
def test_library_exports_set_frames():
    from nnpops_amd import build, capi
    handle = ctypes.CDLL(build.build())
    assert hasattr(handle, "nnpops_cfconv_neighbors_set_frames") and "nnpops_cfconv_neighbors_set_frames" in capi.SIGNATURES
    assert hasattr(capi.CFConvNeighbors, "set_frames")
    L = capi.lib()
    assert L.nnpops_cfconv_neighbors_set_frames(None, 1, None) < 0 and b"NULL" in L.nnpops_last_error()


def test_holder_has_set_frames_and_frames():
    import torch
    from nnpops_amd import torch_binding
    torch_binding.load()
    holder = torch.classes.NNPOpsCFConvNeighbors.Holder(3.0)
    assert holder.frames() == []
    holder.set_frames([0, 3, 7])                                           # kept until the first build creates the handle
    assert holder.frames() == [0, 3, 7]
    with pytest.raises(RuntimeError, match="B \\+ 1"):
        holder.set_frames([0])
    with pytest.raises(RuntimeError, match="set_frames"):
        holder.set_molecules([0, 3, 7])                                    # frames and molecules exclude each other, both ways
    holder.set_frames([])
    assert holder.frames() == []
    holder.set_molecules([0, 3, 7])
    with pytest.raises(RuntimeError, match="set_molecules"):
        holder.set_frames([0, 3, 7])


def test_module_has_set_frames_and_keeps_the_offsets(tmp_path):
    import torch
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    nb = CFConvNeighbors(3.0)
    assert nb.frame_offsets == []
    nb.set_frames([0, 3, 7])
    assert nb.frame_offsets == [0, 3, 7] and nb.holder.frames() == [0, 3, 7]
    scripted = torch.jit.script(nb)
    assert scripted.frame_offsets == [0, 3, 7]
    path = str(tmp_path / "neighbors.pt")
    scripted.save(path)
    loaded = torch.jit.load(path)
    assert loaded.frame_offsets == [0, 3, 7] and loaded.holder.frames() == []          # the pickle is the cutoff alone: build() re-applies
    with pytest.raises(Exception, match="set_frames"):
        loaded.build(torch.zeros(7, 3), None)
