"""Second derivatives of PME over frames, what can be checked without a GPU: the exported symbols, the op schemas, and that the keyword
on host tensors meets the frames methods' own refusal."""
import ctypes

import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
from NNPOps.pme import PME
from nnpops_amd import capi


def test_library_exports_the_second_order_frames_entries():
    lib = ctypes.CDLL(capi.lib()._name)
    for name in ("nnpops_pme_direct_frames_double_backward", "nnpops_pme_direct_frames_double_backward_workspace_bytes",
                 "nnpops_pme_reciprocal_frames_spread_directional", "nnpops_pme_reciprocal_frames_interpolate_second",
                 "nnpops_pme_reciprocal_frames_second_workspace_bytes", "nnpops_pme_frames_upstream_grad"):
        assert hasattr(lib, name), name


def test_op_schemas():
    for name in ("pme_direct_frames", "pme_reciprocal_frames"):
        plain, twice = (str(getattr(torch.ops.pme, n).default._schema) for n in (name, name + "_twice"))
        assert twice == plain.replace(f"pme::{name}(", f"pme::{name}_twice(") and twice != plain


def test_the_keyword_on_host_tensors_is_refused_as_the_frames_methods_refuse_them():
    pos, q, boxes = torch.zeros(6, 3), torch.zeros(6), torch.eye(3).repeat(2, 1, 1)
    pme = PME(8, 8, 8, 5, 3.0, 138.935, torch.zeros(6, 0, dtype=torch.int32), reciprocal=True)
    with pytest.raises(ValueError, match="on the GPU"):
        pme.compute_direct_frames(pos, q, 0.4, boxes, [0, 3, 6], twice_differentiable=True)
    with pytest.raises(ValueError, match="on the GPU"):
        pme.compute_reciprocal_frames(pos, q, boxes, [0, 3, 6], twice_differentiable=True)
