"""Batched CFConv without a GPU: the judge of tests/cfconv_batch_float64.py is pinned to the single-molecule Restatement, the batch
frames are shown to be what the GPU tests need (overlapping molecules, no distance at the cutoff, rows longer than the first
capacity), and the library and the torch holder export the new entry points."""
import ctypes

import numpy as np
import pytest

import cfconv_batch_float64 as batch
from cfconv_float64 import OUT_ATOL_FRAC, OUT_RTOL, Restatement, SecondOrder, sigma_of


def test_a_batch_of_one_molecule_is_the_restatement():
    """one segment over the whole array: the judge returns Restatement.evaluate / SecondOrder.second of that molecule, to the bit"""
    pos, offsets, cutoff = batch.batch_frame("ragged")
    lo, hi = batch.segments(offsets)[3]                                    # the 64-atom molecule
    W, G = 32, 16
    w1, b1, w2, b2, x, gout, V, Q = batch.batch_layer("ragged", W, G)
    judge = Restatement(W, G, cutoff, sigma_of(G), "ssp", w1, b1, w2, b2)
    mol, one = pos[lo:hi], np.array([0, hi - lo], np.int32)
    got = batch.evaluate(judge, mol, one, x[lo:hi], gout[lo:hi])
    ref = judge.evaluate(mol, batch.FAR_BOX, x[lo:hi], gout[lo:hi])
    for k in ("out", "gx", "g", "i", "j"):
        assert np.array_equal(got[k], ref[k]), k
    assert len(ref["i"]) > 500 and not ref["n"].any()
    sec = batch.second(judge, mol, one, x[lo:hi], gout[lo:hi], V[lo:hi], Q[lo:hi])
    ref2 = SecondOrder.open(judge, mol).second(mol, x[lo:hi], gout[lo:hi], V[lo:hi], Q[lo:hi])
    for k in ("dg", "dx", "dp"):
        assert np.array_equal(sec[k], ref2[k]) and np.abs(ref2[k]).max() > 0, k
    # ... and inside a batch the molecule gets the same numbers, whatever lies around it
    whole = batch.evaluate(judge, pos, offsets, x, gout)
    assert np.array_equal(whole["out"][lo:hi], ref["out"]) and np.array_equal(whole["g"][lo:hi], ref["g"])
    assert not whole["out"][0].any()                                       # the single atom: an empty row, exact zeros


@pytest.mark.parametrize("tag", batch.TAGS)
def test_molecules_overlap_so_that_ignoring_the_segments_shows(tag):
    pos, offsets, cutoff = batch.batch_frame(tag)
    i, j = batch.half_pairs(pos, offsets, cutoff)
    ai, aj = batch.all_pairs(pos, cutoff)
    mol = np.searchsorted(offsets, np.arange(len(pos)), side="right") - 1
    cross = mol[ai] != mol[aj]
    assert cross.sum() > 1000 and len(ai) == len(i) + cross.sum(), (len(i), len(ai), int(cross.sum()))
    assert (mol[i] == mol[j]).all()
    # every molecule of more than one atom has a partner in another molecule inside the cutoff
    touched = np.zeros(len(offsets) - 1, bool)
    touched[mol[ai[cross]]] = True; touched[mol[aj[cross]]] = True
    assert touched.all()


def test_ignoring_the_segments_changes_the_output():
    """the Restatement over the concatenated atoms (what a list without segments would convolve) against the judge: another output,
    thousands of times the parity bar away"""
    tag, W, G = "ragged", 20, 10
    pos, offsets, cutoff = batch.batch_frame(tag)
    w1, b1, w2, b2, x, gout, _, _ = batch.batch_layer(tag, W, G)
    judge = Restatement(W, G, cutoff, sigma_of(G), "ssp", w1, b1, w2, b2)
    right = batch.evaluate(judge, pos, offsets, x, gout)
    wrong = judge.evaluate(pos, batch.FAR_BOX, x, gout)
    assert len(wrong["i"]) > len(right["i"])
    top = np.abs(right["out"]).max()
    err = np.abs(wrong["out"] - right["out"])
    assert err.max() > 1000 * (OUT_RTOL + OUT_ATOL_FRAC) * top, (err.max(), top)
    assert (err.max(axis=1) > OUT_ATOL_FRAC * top).all()                    # every atom, the lone one included, feels the others


@pytest.mark.parametrize("tag", batch.TAGS)
def test_no_intramolecular_distance_sits_at_the_cutoff(tag):
    """float64 distances of the float32 coordinates: none within NEAR = 1e-4 A of the cutoff, no molecule excluded -- float32
    arithmetic on the device (relative error ~1e-7 of r^2 = 25 .. 81) then decides every pair as float64 does"""
    pos, offsets, cutoff = batch.batch_frame(tag)
    m = batch.margin(pos, offsets, cutoff)
    print(f"\n[cfconv-batch] {tag}: {len(offsets) - 1} molecules, {len(pos)} atoms, smallest |r - cutoff| {m:.2e} A")
    assert m > batch.NEAR


def test_frames_have_the_shapes_the_builder_is_probed_with():
    pos, offsets, cutoff = batch.batch_frame("ragged")
    assert np.diff(offsets).tolist() == [1, 2, 21, 64, 65, 7] and len(pos) == 160
    pos, offsets, cutoff = batch.batch_frame("frames64")
    assert len(pos) == 1344 >= 1024 and (np.diff(offsets) == 21).all()
    pos, offsets, cutoff = batch.batch_frame("crowded")
    i, j = batch.half_pairs(pos, offsets, cutoff)
    rows = np.bincount(np.concatenate([i, j]), minlength=len(pos))
    assert rows.max() > 64 and rows.max() <= 128, rows.max()                # one doubling of the row capacity
    for tag in batch.TAGS:                                                  # every molecule is centred on the origin
        pos, offsets, _ = batch.batch_frame(tag)
        for lo, hi in batch.segments(offsets):
            assert np.abs(pos[lo:hi].astype(np.float64).mean(axis=0)).max() < 1e-5


def test_library_and_holder_export_set_molecules():
    import torch
    from nnpops_amd import build, capi, torch_binding
    handle = ctypes.CDLL(build.build())
    assert hasattr(handle, "nnpops_cfconv_neighbors_set_molecules") and "nnpops_cfconv_neighbors_set_molecules" in capi.SIGNATURES
    assert hasattr(capi.CFConvNeighbors, "set_molecules")
    L = capi.lib()
    assert L.nnpops_cfconv_neighbors_set_molecules(None, 1, None) < 0 and b"NULL" in L.nnpops_last_error()
    torch_binding.load()
    holder = torch.classes.NNPOpsCFConvNeighbors.Holder(5.0)
    assert holder.molecules() == []
    holder.set_molecules([0, 3, 7])                                         # kept until the first build creates the handle
    assert holder.molecules() == [0, 3, 7]
    with pytest.raises(RuntimeError, match="B \\+ 1"):
        holder.set_molecules([0])
    holder.set_molecules([])
    assert holder.molecules() == []


def test_module_keeps_the_offsets_through_script_and_save(tmp_path):
    import torch
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    nb = CFConvNeighbors(5.0)
    nb.set_molecules([0, 3, 7])
    scripted = torch.jit.script(nb)
    assert scripted.molecule_offsets == [0, 3, 7]
    path = str(tmp_path / "neighbors.pt")
    scripted.save(path)
    loaded = torch.jit.load(path)
    assert loaded.molecule_offsets == [0, 3, 7] and loaded.holder.molecules() == []      # the pickle is the cutoff alone: build() re-applies
    with pytest.raises(Exception, match="batched molecules"):
        loaded.build(torch.zeros(7, 3), torch.eye(3))
