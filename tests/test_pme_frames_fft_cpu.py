"""The LDS-resident transform of PME over frames, what can be checked without a GPU: the exported symbols, the op schemas, the shape rule
through the LDS query, and the refusals of compute_reciprocal_frames(transform=...), which come before any device work."""
import ctypes
import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
from NNPOps.pme import PME
from nnpops_amd import capi

SERVED = [(8, 8, 16), (6, 10, 12), (5, 7, 18), (16, 16, 16), (24, 24, 24), (32, 32, 32), (32, 32, 36)]
REFUSED = [((32, 32, 40), "LDS"), ((11, 8, 8), "prime factors"), ((8, 8, 9), "even")]


def test_library_exports_the_transform_entries():
    lib = ctypes.CDLL(capi.lib()._name)
    for name in ("nnpops_pme_reciprocal_frames_transform", "nnpops_pme_reciprocal_frames_transform_lds_bytes"):
        assert hasattr(lib, name) and name in capi.SIGNATURES, name


@pytest.mark.parametrize("op", ["pme_reciprocal_frames_lds", "pme_reciprocal_frames_lds_box"])
def test_op_schemas(op):
    assert str(getattr(torch.ops.pme, op).default._schema) == (
        f"pme::{op}(Tensor positions, Tensor charges, Tensor box_vectors, Tensor table, Scalar gridx, Scalar gridy, "
        "Scalar gridz, Scalar order, Scalar alpha, Scalar coulomb, Tensor xmoduli, Tensor ymoduli, Tensor zmoduli) -> Tensor")


def test_the_shape_rule():
    for grid in SERVED:
        nbytes, rule = capi.pme_reciprocal_frames_transform_lds_bytes(*grid)
        assert grid[0] * grid[1] * (grid[2] // 2 + 1) * 8 < nbytes <= 160 * 1024 and rule == "", grid
    for grid, word in REFUSED:
        nbytes, rule = capi.pme_reciprocal_frames_transform_lds_bytes(*grid)
        assert nbytes == 0 and word in rule, (grid, rule)


def test_python_refusals_come_before_any_device_work():
    pos, q, boxes = torch.zeros(4, 3), torch.zeros(4), torch.eye(3).repeat(2, 1, 1)        # host tensors: nothing below may reach a launch
    excl = -torch.ones(4, 1, dtype=torch.int32)
    for grid, word in REFUSED:
        with pytest.raises(ValueError, match=word):
            PME(*grid, 4, 3.5, 138.935, excl, reciprocal=True).compute_reciprocal_frames(pos, q, boxes, [0, 2, 4], transform="lds")
    pme = PME(8, 8, 16, 4, 3.5, 138.935, excl, reciprocal=True)
    with pytest.raises(RuntimeError, match="twice_differentiable"):
        pme.compute_reciprocal_frames(pos, q, boxes, [0, 2, 4], twice_differentiable=True, transform="lds")
    with pytest.raises(ValueError, match='"torch" or "lds"'):
        pme.compute_reciprocal_frames(pos, q, boxes, [0, 2, 4], transform="fast")
