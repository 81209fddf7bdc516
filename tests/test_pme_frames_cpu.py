"""PME over frames, what can be checked without a GPU: the exported symbols, the op schemas, the host table, the Python refusals, and
the per-frame float64 judge against the single-system restatement."""
import ctypes
import os
import sys

import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
from NNPOps.pme import PME
from nnpops_amd.pme.pme import bspline_moduli
from nnpops_amd import capi

sys.path.insert(0, os.path.dirname(__file__))
import pme_float64 as f64  # noqa: E402
import pme_frames_float64 as judge  # noqa: E402


def test_library_exports_the_frames_entries():
    lib = ctypes.CDLL(capi.lib()._name)
    for name in ("nnpops_pme_frames_table", "nnpops_pme_frames_table_ints", "nnpops_pme_direct_frames",
                 "nnpops_pme_direct_frames_workspace_bytes", "nnpops_pme_reciprocal_frames_spread", "nnpops_pme_reciprocal_frames_convolve",
                 "nnpops_pme_reciprocal_frames_interpolate", "nnpops_pme_reciprocal_frames_workspace_bytes"):
        assert hasattr(lib, name), name


def test_op_schemas():
    assert str(torch.ops.pme.pmeFramesTable.default._schema) == "pme::pmeFramesTable(Tensor offsets, Device device) -> Tensor"
    assert str(torch.ops.pme.pme_direct_frames.default._schema) == (
        "pme::pme_direct_frames(Tensor positions, Tensor charges, Tensor exclusions, Tensor box_vectors, Tensor table, Scalar cutoff, "
        "Scalar alpha, Scalar coulomb) -> Tensor")
    assert str(torch.ops.pme.pme_reciprocal_frames.default._schema) == (
        "pme::pme_reciprocal_frames(Tensor positions, Tensor charges, Tensor box_vectors, Tensor table, Scalar gridx, Scalar gridy, "
        "Scalar gridz, Scalar order, Scalar alpha, Scalar coulomb, Tensor xmoduli, Tensor ymoduli, Tensor zmoduli) -> Tensor")


def test_table_records():
    offsets = [0, 3, 3, 20, 36]                          # 3 atoms, an empty frame, 17 atoms (two tiles), 16 atoms (one tile)
    t = torch.ops.pme.pmeFramesTable(torch.tensor(offsets), torch.device("cpu")).tolist()
    assert t == capi.pme_frames_table(offsets).tolist()
    B, N, T = 4, 36, 4
    assert t[:4] == [B, N, T, 0]
    assert t[4:9] == offsets
    assert t[9:14] == [0, 1, 1, 3, 4]                    # tile_start: the empty frame owns no tile
    assert t[14:30] == [0, 0, 3, 0,   2, 3, 17, 3,   2, 3, 17, 19,   3, 20, 16, 20]
    assert t[30:] == [0] * 3 + [2] * 17 + [3] * 16 and len(t) == 4 + 2 * (B + 1) + 4 * T + N
    for bad in ([1, 3], [0, 3, 2]):
        with pytest.raises(Exception):
            torch.ops.pme.pmeFramesTable(torch.tensor(bad), torch.device("cpu"))


def test_python_refusals():
    pos, q, boxes = torch.zeros(6, 3), torch.zeros(6), torch.eye(3).repeat(2, 1, 1)
    across = torch.tensor([[3], [-1], [-1], [0], [-1], [-1]], dtype=torch.int32)      # atom 0 (frame 0) excludes atom 3 (frame 1)
    pme = PME(8, 8, 8, 5, 3.0, 138.935, across, reciprocal=True)
    with pytest.raises(ValueError, match="inside a frame"):
        pme.compute_direct_frames(pos, q, 0.4, boxes, [0, 3, 6])
    none = torch.zeros(6, 0, dtype=torch.int32)
    pme = PME(8, 8, 8, 5, 3.0, 138.935, none, reciprocal=True)
    for offsets in ([0, 3, 5], [1, 3, 6], [0, 4, 3, 6], [0]):
        with pytest.raises(ValueError, match="offsets"):
            pme.compute_direct_frames(pos, q, 0.4, boxes, offsets)
    with pytest.raises(ValueError, match="on the GPU"):
        pme.compute_direct_frames(pos, q, 0.4, boxes, [0, 3, 6])
    with pytest.raises(ValueError, match="on the GPU"):
        pme.compute_reciprocal_frames(pos, q, boxes, [0, 3, 6])
    with pytest.raises(ValueError, match="one box per frame"):
        pme.compute_reciprocal_frames(pos, q, boxes[0], [0, 3, 6])
    twice = PME(8, 8, 8, 5, 3.0, 138.935, none, reciprocal=True, twice_differentiable=True)
    for call in (lambda: twice.compute_direct_frames(pos, q, 0.4, boxes, [0, 3, 6]), lambda: twice.compute_reciprocal_frames(pos, q, boxes, [0, 3, 6])):
        with pytest.raises(RuntimeError, match="twice_differentiable"):
            call()
    with pytest.raises(ValueError, match="order 4 or 5"):
        PME(8, 8, 8, 6, 3.0, 138.935, none, reciprocal=True).compute_reciprocal_frames(pos, q, boxes, [0, 3, 6])


def test_reciprocal_workspace_refuses_more_workgroups_than_one_launch_takes():
    """check_recip: frames x max(bricks, convolution workgroups) must fit blockIdx.x, 2^31 - 1; a refused shape reports 0 bytes"""
    size = capi.lib().nnpops_pme_reciprocal_frames_workspace_bytes
    box_size = capi.lib().nnpops_pme_reciprocal_frames_box_workspace_bytes
    limit = 2 ** 31 - 1
    for grid, per_frame in (((64, 64, 64), 1024),          # 16 x 16 x 4 bricks = the convolution's cap of 1 024 workgroups
                            ((8, 8, 16), 4),               # 2 x 2 x 1 bricks, 3 convolution workgroups
                            ((256, 256, 64), 16384)):      # 64 x 64 x 4 bricks, above the convolution's cap
        most = limit // per_frame
        for order in (4, 5):
            assert size(0, most, *grid, order) > 0 and size(0, most + 1, *grid, order) == 0, (grid, order)
        assert box_size(most, *grid) > 0 and box_size(most + 1, *grid) == 0, grid
    assert size(0, 1, 8, 8, 8, 6) == 0 and size(0, 0, 8, 8, 8, 5) == 0 and size(-1, 1, 8, 8, 8, 5) == 0


@pytest.mark.parametrize("triclinic", [False, True])
def test_judge_equals_the_single_system_restatement(triclinic):
    pos, q, box = f64.system(triclinic, n=30, seed=5, outside=True)
    excl = f64.exclusion_table(30, seed=5)
    nb, deltas, _, _ = torch.ops.neighbors.getNeighborPairs(torch.tensor(pos, dtype=torch.float64), judge.CUTOFF, -1,
                                                             torch.tensor(box, dtype=torch.float64), False)
    x, c = torch.tensor(pos, dtype=torch.float64), torch.tensor(q, dtype=torch.float64)
    pairs = f64.listed_pairs_frozen(nb, deltas, x, excl)
    ref = f64.direct_energy_frozen(x, c, pairs, judge.ALPHA, judge.COULOMB)
    e, terms, _, _ = judge.direct_judge(pos, q, box[None], [0, 30], excl.numpy())
    assert abs(float(e[0]) - float(ref)) <= 1e-12 * float(terms[0])
    moduli = [bspline_moduli(k, 5) for k in (6, 7, 9)]
    e, _, _ = judge.recip_judge(pos, q, box[None], [0, 30], (6, 7, 9), 5, moduli)
    ref = f64.spme_energy(x, c, torch.tensor(box, dtype=torch.float64), (6, 7, 9), 5, judge.ALPHA, judge.COULOMB, moduli)
    assert abs(float(e[0]) - float(ref)) <= 1e-13 * abs(float(ref))
