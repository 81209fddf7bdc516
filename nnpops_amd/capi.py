"""ctypes view of ``libnnpops_hip.so`` -- the C ABI declared in ``include/nnpops_hip.h``.

This is the thinnest possible host layer: it loads the in-tree library, declares every exported
symbol's signature, and offers small classes that hand PyTorch device tensors (used purely as
device-memory owners) to the C ABI by raw pointer.  There is no CPU fallback: if the library is
missing or there is no HIP device the calls raise.

Reference interfaces mirrored (file:line relative to /root/reference/src):
    AniSymmetryFunctions   -> ani/ANISymmetryFunctions.h:41-154   (computeSymmetryFunctions / backprop)
    CFConvNeighbors, CFConv -> schnet/CFConv.h:37-217             (build / compute / backprop)
    neighbor_pairs          -> pytorch/neighbors/getNeighborPairsCUDA.cu:103-196
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnnpops_hip.so")

OK = 0
ERR_CAPACITY = -4

# name -> (restype, argtypes); the single source the symbol-export test checks against the header
SIGNATURES = {
    "nnpops_last_error": (C.c_char_p, []),
    "nnpops_version": (C.c_char_p, []),
    "nnpops_device_count": (C.c_int, []),
    "nnpops_ani_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "nnpops_ani_destroy": (C.c_int, [C.c_void_p]),
    "nnpops_ani_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nnpops_ani_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_ani_backprop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_ani_compute_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "nnpops_ani_backprop_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "nnpops_ani_backprop_box_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                  C.c_void_p]),
    "nnpops_ani_tangent_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "nnpops_ani_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nnpops_ani_check_begin": (C.c_int, [C.c_void_p]),
    "nnpops_ani_check_end": (C.c_int, [C.c_void_p]),
    "nnpops_ani_set_neighbor_algorithm": (C.c_int, [C.c_void_p, C.c_int]),
    "nnpops_ani_set_grid_build": (C.c_int, [C.c_void_p, C.c_int]),
    "nnpops_ani_set_molecules": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "nnpops_ani_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "nnpops_ani_set_timing_stride": (C.c_int, [C.c_void_p, C.c_int]),
    "nnpops_ani_get_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "nnpops_ani_timing_overhead": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "nnpops_ani_overflow_word": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "nnpops_ani_read_overflow": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "nnpops_ani_read_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "nnpops_ani_describe": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "nnpops_ani_check_begin_with": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    "nnpops_ani_set_timing_merge": (C.c_int, [C.c_void_p, C.c_int]),
    "nnpops_cfconv_neighbors_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_float, C.c_int, C.c_int]),
    "nnpops_cfconv_neighbors_destroy": (C.c_int, [C.c_void_p]),
    "nnpops_cfconv_neighbors_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_neighbors_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_neighbors_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "nnpops_cfconv_neighbors_export": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_neighbors_read_grid": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "nnpops_cfconv_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "nnpops_cfconv_destroy": (C.c_int, [C.c_void_p]),
    "nnpops_cfconv_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_backprop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_backprop_box": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_double_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_neighbors_build_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "nnpops_cfconv_neighbors_set_molecules": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "nnpops_cfconv_neighbors_set_frames": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "nnpops_cfconv_plan": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "nnpops_cfconv_describe": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "nnpops_cfconv_backprop_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "nnpops_cfconv_double_backward_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_cfconv_set_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_split_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_long]),
    "nnpops_rows_dot": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "nnpops_gemm_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_long, C.c_void_p,
                                    C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_long,
                                    C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                    C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "nnpops_gemm_split_last": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nnpops_mlp_packed_halves": (C.c_int64, [C.c_int, C.c_int]),
    "nnpops_mlp_d1_halves": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "nnpops_mlp_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]),
    "nnpops_mlp_networks_plane_halves": (C.c_int64, [C.c_void_p, C.c_int]),
    "nnpops_mlp_networks_floats": (C.c_int64, [C.c_void_p]),
    "nnpops_mlp_pack_networks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_mlp_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "nnpops_mlp_input_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nnpops_mlp_weight_grad_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "nnpops_mlp_weight_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_mlp_weight_grad_tangent_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "nnpops_mlp_weight_grad_tangent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_mlp_energy_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "nnpops_mlp_energy_mean_shifted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "nnpops_scale_by_scalar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "nnpops_mlp_energy_mean_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                                  C.c_void_p]),
    "nnpops_mlp_energy_mean_segments_shifted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                                          C.c_void_p, C.c_void_p]),
    "nnpops_scale_by_segment": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "nnpops_mlp_member_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nnpops_mlp_member_sums_shifted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "nnpops_neighbor_pairs_workspace_bytes": (C.c_int64, [C.c_int]),
    "nnpops_neighbor_pairs_forward": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int64,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_neighbor_pairs_read_grid": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]),
    "nnpops_pme_direct_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "nnpops_pme_direct": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_direct_indexed_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "nnpops_pme_direct_indexed": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_reciprocal_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nnpops_pme_reciprocal_spread": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_reciprocal_convolve": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_reciprocal_interpolate": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_direct_box_workspace_bytes": (C.c_int64, [C.c_int64]),
    "nnpops_pme_direct_box": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_reciprocal_box_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nnpops_pme_reciprocal_convolve_box": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_reciprocal_box_gradient": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_direct_double_backward_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "nnpops_pme_direct_double_backward": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_reciprocal_second_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nnpops_pme_reciprocal_spread_directional": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_pme_reciprocal_interpolate_second": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p]),
    "nnpops_neighbor_pairs_backward": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_neighbor_pairs_backward_workspace_bytes": (C.c_int64, [C.c_int]),
    "nnpops_neighbor_pairs_index_ints": (C.c_int64, [C.c_int, C.c_int64]),
    "nnpops_neighbor_pairs_index_workspace_bytes": (C.c_int64, [C.c_int, C.c_int64]),
    "nnpops_neighbor_pairs_build_index": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_neighbor_pairs_backward_indexed_workspace_bytes": (C.c_int64, [C.c_int, C.c_int64]),
    "nnpops_neighbor_pairs_backward_indexed": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_neighbor_pairs_box_backward_workspace_bytes": (C.c_int64, [C.c_int64]),
    "nnpops_neighbor_pairs_box_backward": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_neighbor_pairs_double_backward": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "nnpops_neighbor_pairs_backward_ws": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


class NNPOpsHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"[nnpops_hip {code}] {message}")
        self.code = code


def lib():
    """Load libnnpops_hip.so (once).  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m nnpops_amd.build` "
                          "(hipcc --offload-arch=gfx950). nnpops_amd has no CPU fallback.")
    handle = C.CDLL(LIB_PATH)
    missing = [name for name in SIGNATURES if not hasattr(handle, name)]
    if missing:                             # header/library mismatch: fail loudly
        raise ImportError(f"{LIB_PATH} does not export {missing}; rebuild with `python -m nnpops_amd.build --force`")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype = restype
        fn.argtypes = argtypes
    # the binary must have been built from the sources next to it (build.py embeds their hash in nnpops_version())
    from . import build as _build
    have, want = handle.nnpops_version().decode(), _build.source_hash()
    if not have.endswith("src:" + want):
        raise ImportError(f"{LIB_PATH} is stale: it reports '{have}' but the sources hash to {want}; "
                          "rebuild with `python -m nnpops_amd.build`")
    _lib = handle
    return _lib


def _check(code):
    if code != OK:
        raise NNPOpsHipError(code, lib().nnpops_last_error().decode())


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev_f32(t, name, shape=None):
    if not t.is_cuda:
        raise ValueError(f'"{name}" must live on the HIP device (nnpops_amd has no CPU path)')
    if t.dtype != torch.float32:
        raise ValueError(f'"{name}" must be float32')
    if not t.is_contiguous():
        raise ValueError(f'"{name}" must be contiguous')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'"{name}" has shape {tuple(t.shape)}, expected {tuple(shape)}')
    return t


GRID_FIELDS = ("nx", "ny", "nz", "ncells", "m", "ok", "bin_overflow", "periodic")


def _grid_dict(words):
    return dict(zip(GRID_FIELDS, (int(v) for v in words)))


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class AniSymmetryFunctions:
    """One molecule / frame's ANI symmetry-function evaluator on one GPU.

    Mirrors the reference object: construct once with the frozen parameters, ``compute`` then
    ``backprop`` (which relies on state left by the last ``compute``)."""

    def __init__(self, num_species, radial_cutoff, angular_cutoff, atom_species, radial_functions, angular_functions,
                 periodic=False, torchani=True, device=0):
        self._lib = lib()
        self._h = C.c_void_p()
        species = np.ascontiguousarray(atom_species, dtype=np.int32)
        rf = np.ascontiguousarray(radial_functions, dtype=np.float32).reshape(-1, 2)
        af = np.ascontiguousarray(angular_functions, dtype=np.float32).reshape(-1, 4)
        self.num_atoms, self.num_species = int(species.shape[0]), int(num_species)
        self.num_radial, self.num_angular = int(rf.shape[0]), int(af.shape[0])
        self.periodic = bool(periodic)
        self.num_molecules = 0          # > 0: set_molecules is in force; a periodic evaluator then takes one box per molecule
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        _check(self._lib.nnpops_ani_create(C.byref(self._h), self.num_atoms, self.num_species, radial_cutoff,
                                           angular_cutoff, int(self.periodic), species.ctypes.data_as(C.c_void_p),
                                           self.num_radial, rf.ctypes.data_as(C.c_void_p), self.num_angular,
                                           af.ctypes.data_as(C.c_void_p), int(bool(torchani)), self.device.index))
        self.radial_width = self.num_species * self.num_radial
        self.angular_width = self.num_species * (self.num_species + 1) // 2 * self.num_angular

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.nnpops_ani_destroy(h)
            self._h = None

    def set_molecules(self, molecule_offsets):
        """Treat the handle's atoms as a batch of independent molecules: atoms [offsets[m], offsets[m+1]) belong to molecule m
        (None restores one system).  On a periodic evaluator every molecule is a frame in a box of its own: ``compute`` and
        ``backprop_box`` then take ``box [M,3,3]`` (all-pairs search inside the frame: frames of tens to a few hundred atoms)."""
        if molecule_offsets is None:
            _check(self._lib.nnpops_ani_set_molecules(self._h, 0, None))
            self.num_molecules = 0
            return
        off = np.ascontiguousarray(molecule_offsets, dtype=np.int32)
        _check(self._lib.nnpops_ani_set_molecules(self._h, int(off.shape[0]) - 1, off.ctypes.data_as(C.c_void_p)))
        self.num_molecules = int(off.shape[0]) - 1

    def _box_shape(self):
        return (self.num_molecules, 3, 3) if self.num_molecules > 0 else (3, 3)

    def set_neighbor_algorithm(self, algorithm):
        _check(self._lib.nnpops_ani_set_neighbor_algorithm(self._h, int(algorithm)))

    def set_grid_build(self, one_launch):
        """True: the one-launch build of the periodic cell grid (where the system is small enough for it), False: the two-launch
        build; describe()["grid_build"] says which the handle runs.  Bit-identical results (tests, A/B)."""
        _check(self._lib.nnpops_ani_set_grid_build(self._h, int(bool(one_launch))))

    def compute(self, positions, box=None, radial=None, angular=None, check=True):
        """positions [N,3] (device fp32), box [3,3] ([M,3,3] when molecules are set on a periodic evaluator) or None
        -> (radial [N,S*nR], angular [N,NB*nA]).

        ``check=True`` blocks once on the stream to see whether a neighbour row overflowed and, if
        so, repeats the computation with the grown buffers (the C ABI reports, never truncates)."""
        _dev_f32(positions, "positions", (self.num_atoms, 3))
        if self.periodic:
            if box is None:
                raise ValueError("periodic evaluator needs box vectors")
            _dev_f32(box, "box", self._box_shape())
        if radial is None:
            radial = torch.empty((self.num_atoms, self.radial_width), dtype=torch.float32, device=positions.device)
        if angular is None:
            angular = torch.empty((self.num_atoms, self.angular_width), dtype=torch.float32, device=positions.device)
        _check(self._lib.nnpops_ani_set_stream(self._h, _stream_ptr(positions.device)))
        for _ in range(8):
            _check(self._lib.nnpops_ani_compute(self._h, _ptr(positions), _ptr(box if self.periodic else None),
                                                _ptr(radial), _ptr(angular)))
            if not check:
                break
            code = self._lib.nnpops_ani_check(self._h, None, None)
            if code == OK:
                break
            if code != ERR_CAPACITY:
                _check(code)
        else:
            raise NNPOpsHipError(ERR_CAPACITY, "neighbour buffers kept overflowing")
        return radial, angular

    def backprop(self, radial_grad, angular_grad, position_grad=None):
        _dev_f32(radial_grad, "radial_grad", (self.num_atoms, self.radial_width))
        _dev_f32(angular_grad, "angular_grad", (self.num_atoms, self.angular_width))
        if position_grad is None:
            position_grad = torch.empty((self.num_atoms, 3), dtype=torch.float32, device=radial_grad.device)
        _check(self._lib.nnpops_ani_set_stream(self._h, _stream_ptr(radial_grad.device)))
        _check(self._lib.nnpops_ani_backprop(self._h, _ptr(radial_grad), _ptr(angular_grad), _ptr(position_grad)))
        return position_grad

    def backprop_box(self, positions, box, radial_grad, angular_grad, position_grad=None, box_grad=None):
        """``backprop`` plus the box-vector gradient (virial) of the same scalar -> (position_grad [N,3], box_grad [3,3]);
        with molecules set on a periodic evaluator ``box`` and ``box_grad`` are [M,3,3], molecule m's entries summed over its own atoms.

        ``box_grad[k][c] = sum n_k (dL/dd)_c`` over every displacement ``d = x_j - x_i + n @ box`` the AEV used, the integer
        minimum-image shifts ``n`` held fixed; all nine entries.  ``positions`` and ``box`` must be the tensors of the preceding
        ``compute`` (the shifts are recovered from them).  Periodic evaluators only."""
        _dev_f32(positions, "positions", (self.num_atoms, 3))
        shape = self._box_shape() if self.periodic else (3, 3)
        _dev_f32(box, "box", shape)
        _dev_f32(radial_grad, "radial_grad", (self.num_atoms, self.radial_width))
        _dev_f32(angular_grad, "angular_grad", (self.num_atoms, self.angular_width))
        if position_grad is None:
            position_grad = torch.empty((self.num_atoms, 3), dtype=torch.float32, device=radial_grad.device)
        if box_grad is None:
            box_grad = torch.empty(shape, dtype=torch.float32, device=radial_grad.device)
        else:
            _dev_f32(box_grad, "box_grad", shape)
        _check(self._lib.nnpops_ani_set_stream(self._h, _stream_ptr(radial_grad.device)))
        _check(self._lib.nnpops_ani_backprop_box_strided(self._h, _ptr(positions), _ptr(box), _ptr(radial_grad), 0, _ptr(angular_grad), 0,
                                                         _ptr(position_grad), _ptr(box_grad)))
        return position_grad, box_grad

    def tangent(self, position_tangent, radial_tangent=None, angular_tangent=None):
        """The tangent ``J.v`` of the AEV of the preceding ``compute`` along ``position_tangent`` [N,3] -> (radial [N,S*nR], angular
        [N,NB*nA]): ``d/dt aev(x + t v)`` at ``t = 0`` on the lists the handle holds, shifts and box fixed.  The adjoint of ``backprop``
        (``<w, tangent(v)> == <backprop(w), v>``) and what the parameter gradient of a force loss needs of the AEV.  Outputs may be
        row-strided views (one [N, W_r + W_a] array, as ``compute_strided`` writes); they are fully overwritten, bit-reproducibly."""
        _dev_f32(position_tangent, "position_tangent", (self.num_atoms, 3))
        dev = position_tangent.device
        if radial_tangent is None:
            radial_tangent = torch.empty((self.num_atoms, self.radial_width), dtype=torch.float32, device=dev)
        if angular_tangent is None:
            angular_tangent = torch.empty((self.num_atoms, self.angular_width), dtype=torch.float32, device=dev)
        lds = []
        for t, width, name in ((radial_tangent, self.radial_width, "radial_tangent"), (angular_tangent, self.angular_width, "angular_tangent")):
            if (t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (self.num_atoms, width) or t.stride(1) != 1
                    or t.stride(0) < width):
                raise ValueError(f"{name} must be a float32 [{self.num_atoms}, {width}] device array with unit inner stride")
            lds.append(int(t.stride(0)))
        _check(self._lib.nnpops_ani_set_stream(self._h, _stream_ptr(dev)))
        _check(self._lib.nnpops_ani_tangent_strided(self._h, _ptr(position_tangent), C.c_void_p(radial_tangent.data_ptr()), lds[0],
                                                    C.c_void_p(angular_tangent.data_ptr()), lds[1]))
        return radial_tangent, angular_tangent

    KERNELS = ("neighbors", "radial_forward", "angular_forward", "radial_backward", "angular_backward", "cell_grid")

    def enable_timing(self, enable=True, only=None, every=1):
        """HIP-event timing of the kernels: all of them, or just the names in ``only``, on every ``every``-th launch
        (each event costs a few microseconds of stream time, so benchmarks time one kernel on a sample of the steps
        inside their timed region)."""
        mask = int(bool(enable))
        if enable and only:
            mask = sum(1 << (self.KERNELS.index(k) + 1) for k in only)
        _check(self._lib.nnpops_ani_set_timing_stride(self._h, int(every)))
        _check(self._lib.nnpops_ani_enable_timing(self._h, mask))

    def describe(self):
        """-> {key: value} of nnpops_ani_describe: which kernels this handle runs (forward, backward, uniform, grid, literal, ...);
        ``batch_boxes`` is there ('1') only while molecules are set on a periodic evaluator."""
        buf = C.create_string_buffer(512)
        _check(self._lib.nnpops_ani_describe(self._h, buf, 512))
        return dict(word.split("=", 1) for word in buf.value.decode().split())

    def overflow_word(self):
        """The builders' sticky overflow word (bit 0 rows, 1 box too small for the grid, 2 cell bins, 3 an atom outgrew its backward
        class), read from the device (blocks on the handle's stream's device)."""
        word = C.c_int32(0)
        torch.cuda.synchronize()
        _check(self._lib.nnpops_ani_read_overflow(self._h, C.byref(word)))     # (copied by the library's own runtime: ADVICE r05)
        return word.value

    def read_grid(self):
        """The cell grid the last compute() decided, {nx, ny, nz, ncells, m, ok, bin_overflow, periodic} (blocks; diagnostics only,
        meaningful once a compute() has gone through the grid: describe()["cells"])."""
        words = (C.c_int32 * 8)()
        _check(self._lib.nnpops_ani_read_grid(self._h, words))
        return _grid_dict(words)

    def set_timing_merge(self, merge):
        """True: one bracket around build + angular forward (reported as "neighbors") and one around the two backward kernels (reported as
        "angular_backward") instead of the four single ones: single + single - merged = what a bracket costs, measured in place."""
        _check(self._lib.nnpops_ani_set_timing_merge(self._h, int(bool(merge))))

    def get_timing(self):
        """-> {kernel: (total_ms, launches)} since the last call; blocks on the stream."""
        ms = (C.c_double * len(self.KERNELS))()
        cnt = (C.c_int * len(self.KERNELS))()
        _check(self._lib.nnpops_ani_get_timing(self._h, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(self.KERNELS)}

    def timing_overhead(self):
        """Seconds an event pair reports for an empty bracket on this handle's stream (blocks)."""
        ms = C.c_double(0)
        _check(self._lib.nnpops_ani_timing_overhead(self._h, C.byref(ms)))
        return 1e-3 * ms.value

    def check_begin(self):
        """First half of the deferred capacity check (right after compute(check=False)): True when the check is in flight and
        check_end() will finish it, False when it cannot be deferred (call neighbor_stats() / compute(check=True) instead)."""
        return self._lib.nnpops_ani_check_begin(self._h) == 1

    def check_end(self):
        """Second half: OK, or ERR_CAPACITY after the buffers have grown (compute() and its consumers must be issued again)."""
        code = self._lib.nnpops_ani_check_end(self._h)
        if code not in (OK, ERR_CAPACITY):
            _check(code)
        return code

    def neighbor_stats(self):
        """(max neighbours within Rcr, max neighbours within Rca) of the last compute; blocks."""
        a, b = C.c_int(0), C.c_int(0)
        code = self._lib.nnpops_ani_check(self._h, C.byref(a), C.byref(b))
        if code not in (OK, ERR_CAPACITY):
            _check(code)
        return a.value, b.value


# ---------------------------------------------------------------------------------------------
# getNeighborPairs (reference src/pytorch/neighbors/getNeighborPairsCUDA.cu)
# ---------------------------------------------------------------------------------------------
_DTYPE_CODE = {torch.float32: 0, torch.float64: 1}


def neighbor_pairs_forward(positions, cutoff, max_num_pairs=-1, box=None, return_grid=False):
    """-> (neighbors int32[2,P], deltas[P,3], distances[P], num_pairs int32[1]) on positions' device.

    P = N(N-1)/2 when max_num_pairs == -1, else max_num_pairs.  No host synchronisation.
    return_grid=True (diagnostics: blocks) appends the cell grid the call left in its workspace, as AniSymmetryFunctions.read_grid,
    or None when the call built none (max_num_pairs == -1, or fewer than 8 192 atoms)."""
    if not positions.is_cuda:
        raise ValueError('"positions" must live on the HIP device (nnpops_amd has no CPU path)')
    if positions.dtype not in _DTYPE_CODE:
        raise ValueError('"positions" must be float32 or float64')
    if positions.dim() != 2 or positions.size(1) != 3 or not positions.is_contiguous():
        raise ValueError('Expected "positions" to be a contiguous (num_atoms, 3) tensor')
    n = positions.size(0)
    max_num_pairs = int(max_num_pairs)
    if not (max_num_pairs > 0 or max_num_pairs == -1):
        raise ValueError('Expected "max_num_pairs" to be positive or equal to -1')
    slots = n * (n - 1) // 2 if max_num_pairs == -1 else max_num_pairs
    dev, dt = positions.device, positions.dtype
    if box is not None and box.numel():
        if tuple(box.shape) != (3, 3):
            raise ValueError('Expected "box_vectors" to have shape (3, 3)')
        box = box.to(device=dev, dtype=dt).contiguous()
    else:
        box = None
    neighbors = torch.empty((2, slots), dtype=torch.int32, device=dev)
    deltas = torch.empty((slots, 3), dtype=dt, device=dev)
    distances = torch.empty((slots,), dtype=dt, device=dev)
    num_pairs = torch.empty((1,), dtype=torch.int32, device=dev)
    L = lib()
    ws = torch.empty((int(L.nnpops_neighbor_pairs_workspace_bytes(n)),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(L.nnpops_neighbor_pairs_forward(_DTYPE_CODE[dt], n, _ptr(positions), _ptr(box), float(cutoff), max_num_pairs,
                                               _ptr(neighbors), _ptr(deltas), _ptr(distances), _ptr(num_pairs), _ptr(ws),
                                               _stream_ptr(dev)))
        if return_grid:
            grid = None
            if max_num_pairs != -1 and n >= 8192:
                words = (C.c_int32 * 8)()
                _check(L.nnpops_neighbor_pairs_read_grid(_ptr(ws), n, _stream_ptr(dev), words))
                grid = _grid_dict(words)
            return neighbors, deltas, distances, num_pairs, grid
    return neighbors, deltas, distances, num_pairs


def neighbor_pairs_backward(num_atoms, neighbors, deltas, distances, grad_deltas, grad_distances):
    dev, dt = deltas.device, deltas.dtype
    grad_positions = torch.empty((num_atoms, 3), dtype=dt, device=dev)
    with torch.cuda.device(dev):
        ws = torch.empty((int(lib().nnpops_neighbor_pairs_backward_workspace_bytes(num_atoms)) // 8,), dtype=torch.int64, device=dev)
        _check(lib().nnpops_neighbor_pairs_backward_ws(_DTYPE_CODE[dt], num_atoms, distances.numel(), _ptr(neighbors),
                                                       _ptr(deltas.contiguous()), _ptr(distances.contiguous()),
                                                       _ptr(grad_deltas.contiguous()), _ptr(grad_distances.contiguous()),
                                                       _ptr(grad_positions), _ptr(ws), _stream_ptr(dev)))
    return grad_positions


def neighbor_pairs_build_index(num_atoms, neighbors):
    """Transposed index of a list the forward op emitted: int32 tensor for neighbor_pairs_backward_indexed and pme_direct(index=).

    The list must be compacted (max_num_pairs > 0): used slots first, grouped by neighbors[0], -1 only behind them.  A
    max_num_pairs == -1 list interleaves -1 slots with the pairs and must take neighbor_pairs_backward instead.  Slots whose
    neighbors[1] lies outside [0, num_atoms) are dropped from the transposed view like unused slots.  Up to 262 144 atoms
    (NNPOPS_PAIRS_INDEX_MAX_ATOMS); beyond, NNPOpsHipError with NNPOPS_ERR_UNSUPPORTED."""
    dev = neighbors.device
    L = lib()
    slots = neighbors.size(1)
    index = torch.empty((int(L.nnpops_neighbor_pairs_index_ints(num_atoms, slots)),), dtype=torch.int32, device=dev)
    ws = torch.empty((int(L.nnpops_neighbor_pairs_index_workspace_bytes(num_atoms, slots)) // 8 + 1,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _check(L.nnpops_neighbor_pairs_build_index(num_atoms, slots, _ptr(neighbors), _ptr(index), _ptr(ws), _stream_ptr(dev)))
    return index


def neighbor_pairs_backward_indexed(num_atoms, neighbors, deltas, distances, grad_deltas, grad_distances, index):
    """The backward pass without atomics (owner-computes gather over the transposed index).  `index` must have been built by
    neighbor_pairs_build_index from exactly this `neighbors`, a compacted list (see there); any other list takes neighbor_pairs_backward."""
    dev, dt = deltas.device, deltas.dtype
    grad_positions = torch.empty((num_atoms, 3), dtype=dt, device=dev)
    L = lib()
    with torch.cuda.device(dev):
        ws = torch.empty((int(L.nnpops_neighbor_pairs_backward_indexed_workspace_bytes(_DTYPE_CODE[dt], distances.numel())) // 8 + 1,),
                         dtype=torch.int64, device=dev)
        _check(L.nnpops_neighbor_pairs_backward_indexed(_DTYPE_CODE[dt], num_atoms, distances.numel(), _ptr(neighbors),
                                                        _ptr(deltas.contiguous()), _ptr(distances.contiguous()),
                                                        _ptr(grad_deltas.contiguous()), _ptr(grad_distances.contiguous()),
                                                        _ptr(index), _ptr(grad_positions), _ptr(ws), _stream_ptr(dev)))
    return grad_positions


def neighbor_pairs_box_backward(num_atoms, neighbors, positions, box, deltas, distances, grad_deltas, grad_distances):
    """grad_box [3,3] = - sum_k n_k (x) G_k of the backward pass (n_k: the slot's minimum-image shift, recovered from positions, box and
    deltas).  Any list, compacted or not, in any order; float64 sums in a fixed order (bitwise reproducible).  box in deltas' dtype."""
    dev, dt = deltas.device, deltas.dtype
    grad_box = torch.empty((3, 3), dtype=dt, device=dev)
    L = lib()
    slots = distances.numel()
    with torch.cuda.device(dev):
        ws = torch.empty((int(L.nnpops_neighbor_pairs_box_backward_workspace_bytes(slots)) // 8,), dtype=torch.float64, device=dev)
        _check(L.nnpops_neighbor_pairs_box_backward(_DTYPE_CODE[dt], num_atoms, slots, _ptr(neighbors), _ptr(positions.contiguous()),
                                                    _ptr(box.contiguous()), _ptr(deltas.contiguous()), _ptr(distances.contiguous()),
                                                    _ptr(grad_deltas.contiguous()), _ptr(grad_distances.contiguous()), _ptr(grad_box),
                                                    _ptr(ws), _stream_ptr(dev)))
    return grad_box


def neighbor_pairs_double_backward(num_atoms, neighbors, deltas, distances, grad_distances, gg_positions=None, gg_box=None,
                                   positions=None, box=None):
    """Vector-Jacobian product of the backward pass with (gg_positions [N,3], gg_box [3,3]), either may be None.
    -> (d_grad_deltas [P,3], d_grad_distances [P], d_deltas [P,3], d_distances [P]).  positions and box are needed with gg_box only."""
    dev, dt = deltas.device, deltas.dtype
    slots = distances.numel()
    outs = (torch.empty((slots, 3), dtype=dt, device=dev), torch.empty((slots,), dtype=dt, device=dev),
            torch.empty((slots, 3), dtype=dt, device=dev), torch.empty((slots,), dtype=dt, device=dev))
    ins = [None if t is None else t.contiguous() for t in (positions, box, deltas, distances, grad_distances, gg_positions, gg_box)]
    with torch.cuda.device(dev):
        _check(lib().nnpops_neighbor_pairs_double_backward(_DTYPE_CODE[dt], num_atoms, slots, _ptr(neighbors), *(_ptr(t) for t in ins),
                                                           *(_ptr(t) for t in outs), _stream_ptr(dev)))
    return outs


def pme_direct(positions, charges, neighbors, deltas, distances, exclusions, alpha, coulomb, index=None, workspace_guard=False):
    """Direct-space PME on a pair list (reference src/pytorch/pme/pmeCUDA.cu:30-100) through the C ABI.
    -> (energy float32[1], dE/dpositions [N, 3], dE/dcharges [N]); `exclusions` int32 [N, max], rows sorted descending.
    index: the list's transposed index (neighbor_pairs_build_index) -- the list must then be a compacted one the forward op emitted
    (used slots first, grouped by neighbors[0], -1 only behind them): no atomics.
    workspace_guard: the workspace is exactly nnpops_pme_direct[_indexed]_workspace_bytes long, 256-byte aligned, filled with and
    followed by a guard pattern (as pme_reciprocal_passes): a kernel that writes past it raises; the outputs start as NaN."""
    _dev_f32(positions, "positions")
    _dev_f32(charges, "charges")
    n, pairs = positions.size(0), neighbors.size(1)
    dev = positions.device
    exclusions = exclusions.to(device=dev, dtype=torch.int32).contiguous()
    max_excl = exclusions.size(1)
    energy = torch.empty((1,), dtype=torch.float32, device=dev)
    pos_deriv = torch.empty((n, 3), dtype=torch.float32, device=dev)
    charge_deriv = torch.empty((n,), dtype=torch.float32, device=dev)
    L = lib()
    nbytes = int(L.nnpops_pme_direct_indexed_workspace_bytes(pairs, n) if index is not None else
                 L.nnpops_pme_direct_workspace_bytes(pairs, n, max_excl))
    if workspace_guard:
        # (0x7F bytes: a large finite float, a large double and an int far above any row -- what a call fails to clear shows)
        pattern = 0x7F
        buf = torch.full((nbytes + _PASSES_GUARD + 256,), pattern, dtype=torch.uint8, device=dev)
        off = (-buf.data_ptr()) % 256
        ws_ptr = C.c_void_p(buf.data_ptr() + off)
        for out in (energy, pos_deriv, charge_deriv):          # every output is fully overwritten: an element left out stays NaN
            out.fill_(float("nan"))
    else:
        buf = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        ws_ptr = _ptr(buf)

    def guard_intact():
        if workspace_guard and not (bool((buf[:off] == pattern).all()) and bool((buf[off + nbytes:] == pattern).all())):
            raise RuntimeError(f"pme_direct wrote outside its workspace of {nbytes} bytes")

    if index is not None:
        with torch.cuda.device(dev):
            _check(L.nnpops_pme_direct_indexed(n, pairs, max_excl, _ptr(positions), _ptr(charges), _ptr(neighbors.contiguous()),
                                               _ptr(deltas.contiguous()), _ptr(distances.contiguous()), _ptr(exclusions) if max_excl else None,
                                               _ptr(index), float(alpha), float(coulomb), _ptr(energy), _ptr(pos_deriv), _ptr(charge_deriv),
                                               ws_ptr, _stream_ptr(dev)))
        guard_intact()
        return energy, pos_deriv, charge_deriv
    with torch.cuda.device(dev):
        _check(L.nnpops_pme_direct(n, pairs, max_excl, _ptr(positions), _ptr(charges), _ptr(neighbors.contiguous()),
                                   _ptr(deltas.contiguous()), _ptr(distances.contiguous()), _ptr(exclusions) if max_excl else None,
                                   float(alpha), float(coulomb), _ptr(energy), _ptr(pos_deriv), _ptr(charge_deriv), ws_ptr,
                                   _stream_ptr(dev)))
    guard_intact()
    return energy, pos_deriv, charge_deriv


_PASSES_GUARD, _PASSES_PATTERN = 4096, 0xA5


def pme_reciprocal_passes(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli, zmoduli):
    """pme_reciprocal with every pass's output kept: -> (real grid [Kx, Ky, Kz] of the spread, complex grid [Kx, Ky, Kz/2 + 1] before
    scaling, scaled complex grid, potential grid (irfftn, norm="forward"), energy float32[1], dE/dpositions [N, 3], dE/dcharges [N]).
    The real grid starts as NaN (the spread writes every point exactly once and needs no clearing), and the workspace is exactly
    nnpops_pme_reciprocal_workspace_bytes long, 256-byte aligned and followed by a guard pattern: a pass that writes past it raises."""
    _dev_f32(positions, "positions")
    _dev_f32(charges, "charges")
    _dev_f32(box_vectors, "box_vectors", (3, 3))
    dev = positions.device
    n = positions.size(0)
    mods = [_dev_f32(m.to(device=dev, dtype=torch.float32).contiguous(), name, (k,))
            for m, name, k in ((xmoduli, "xmoduli", gridx), (ymoduli, "ymoduli", gridy), (zmoduli, "zmoduli", gridz))]
    L = lib()
    nbytes = int(L.nnpops_pme_reciprocal_workspace_bytes(n, gridx, gridy, gridz, order))
    buf = torch.full((nbytes + _PASSES_GUARD + 256,), _PASSES_PATTERN, dtype=torch.uint8, device=dev)
    off = (-buf.data_ptr()) % 256
    ws = C.c_void_p(buf.data_ptr() + off)
    real = torch.full((gridx, gridy, gridz), float("nan"), dtype=torch.float32, device=dev)
    energy = torch.empty((1,), dtype=torch.float32, device=dev)
    pos_deriv = torch.empty((n, 3), dtype=torch.float32, device=dev)
    charge_deriv = torch.empty((n,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(L.nnpops_pme_reciprocal_spread(n, gridx, gridy, gridz, order, _ptr(positions), _ptr(charges), _ptr(box_vectors),
                                              float(coulomb), _ptr(real), ws, _stream_ptr(dev)))
        before = torch.fft.rfftn(real).contiguous()
        recip = before.clone()
        _check(L.nnpops_pme_reciprocal_convolve(n, gridx, gridy, gridz, order, _ptr(box_vectors), float(alpha), _ptr(mods[0]),
                                                _ptr(mods[1]), _ptr(mods[2]), _ptr(recip), _ptr(energy), ws, _stream_ptr(dev)))
        grid = torch.fft.irfftn(recip, s=(gridx, gridy, gridz), norm="forward").contiguous()
        _check(L.nnpops_pme_reciprocal_interpolate(n, gridx, gridy, gridz, order, _ptr(charges), _ptr(box_vectors), float(coulomb),
                                                   _ptr(grid), _ptr(pos_deriv), _ptr(charge_deriv), ws, _stream_ptr(dev)))
    if not bool((buf[:off] == _PASSES_PATTERN).all()) or not bool((buf[off + nbytes:] == _PASSES_PATTERN).all()):
        raise RuntimeError(f"pme_reciprocal wrote outside its workspace of {nbytes} bytes")
    return real, before, recip, grid, energy, pos_deriv, charge_deriv


def pme_reciprocal(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli, zmoduli):
    """Reciprocal-space PME (reference src/pytorch/pme/pmeCUDA.cu:102-430) through the C ABI: spread -> torch.fft.rfftn ->
    convolve -> torch.fft.irfftn(norm="forward") -> interpolate.  -> (energy float32[1] without the self energy, dE/dpositions
    [N, 3], dE/dcharges [N]).  Orders 4 and 5."""
    return pme_reciprocal_passes(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli,
                                 zmoduli)[4:]


def pme_direct_box(positions, charges, neighbors, deltas, distances, exclusions, box_vectors, alpha, coulomb):
    """dE/dbox [3, 3] float32 of the direct-space PME energy: - sum_k n_k (x) G_k over the included pairs (n_k: the slot's
    minimum-image shift, recovered from positions, box and deltas).  Any list order; float64 sums in a fixed order."""
    _dev_f32(positions, "positions")
    _dev_f32(charges, "charges")
    _dev_f32(box_vectors, "box_vectors", (3, 3))
    n, pairs = positions.size(0), neighbors.size(1)
    dev = positions.device
    exclusions = exclusions.to(device=dev, dtype=torch.int32).contiguous()
    max_excl = exclusions.size(1)
    grad_box = torch.empty((3, 3), dtype=torch.float32, device=dev)
    L = lib()
    with torch.cuda.device(dev):
        ws = torch.empty((int(L.nnpops_pme_direct_box_workspace_bytes(pairs)) // 8,), dtype=torch.float64, device=dev)
        _check(L.nnpops_pme_direct_box(n, pairs, max_excl, _ptr(positions.contiguous()), _ptr(charges.contiguous()),
                                       _ptr(neighbors.to(torch.int32).contiguous()), _ptr(deltas.contiguous()),
                                       _ptr(distances.contiguous()), _ptr(exclusions) if max_excl else None,
                                       _ptr(box_vectors.contiguous()), float(alpha), float(coulomb), _ptr(grad_box), _ptr(ws),
                                       _stream_ptr(dev)))
    return grad_box


def pme_reciprocal_box(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli, zmoduli):
    """pme_reciprocal with the box gradient: spread -> rfftn -> convolve_box -> irfftn -> interpolate -> box_gradient.
    -> (energy float32[1], dE/dpositions [N, 3], dE/dcharges [N], dE/dbox [3, 3])."""
    _dev_f32(positions, "positions")
    _dev_f32(charges, "charges")
    _dev_f32(box_vectors, "box_vectors", (3, 3))
    dev = positions.device
    n = positions.size(0)
    mods = [_dev_f32(m.to(device=dev, dtype=torch.float32).contiguous(), name, (k,))
            for m, name, k in ((xmoduli, "xmoduli", gridx), (ymoduli, "ymoduli", gridy), (zmoduli, "zmoduli", gridz))]
    L = lib()
    ws = torch.empty((int(L.nnpops_pme_reciprocal_workspace_bytes(n, gridx, gridy, gridz, order)),), dtype=torch.uint8, device=dev)
    box_ws = torch.empty((int(L.nnpops_pme_reciprocal_box_workspace_bytes(n, gridx, gridy, gridz, order)),), dtype=torch.uint8,
                         device=dev)
    real = torch.empty((gridx, gridy, gridz), dtype=torch.float32, device=dev)
    energy = torch.empty((1,), dtype=torch.float32, device=dev)
    pos_deriv = torch.empty((n, 3), dtype=torch.float32, device=dev)
    charge_deriv = torch.empty((n,), dtype=torch.float32, device=dev)
    grad_box = torch.empty((3, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(L.nnpops_pme_reciprocal_spread(n, gridx, gridy, gridz, order, _ptr(positions), _ptr(charges), _ptr(box_vectors),
                                              float(coulomb), _ptr(real), _ptr(ws), _stream_ptr(dev)))
        recip = torch.fft.rfftn(real).contiguous()
        _check(L.nnpops_pme_reciprocal_convolve_box(n, gridx, gridy, gridz, order, _ptr(box_vectors), float(alpha), _ptr(mods[0]),
                                                    _ptr(mods[1]), _ptr(mods[2]), _ptr(recip), _ptr(energy), _ptr(ws), _ptr(box_ws),
                                                    _stream_ptr(dev)))
        grid = torch.fft.irfftn(recip, s=(gridx, gridy, gridz), norm="forward").contiguous()
        _check(L.nnpops_pme_reciprocal_interpolate(n, gridx, gridy, gridz, order, _ptr(charges), _ptr(box_vectors), float(coulomb),
                                                   _ptr(grid), _ptr(pos_deriv), _ptr(charge_deriv), _ptr(ws), _stream_ptr(dev)))
        _check(L.nnpops_pme_reciprocal_box_gradient(n, gridx, gridy, gridz, order, _ptr(positions), _ptr(box_vectors), _ptr(pos_deriv),
                                                    _ptr(grad_box), _ptr(box_ws), _stream_ptr(dev)))
    return energy, pos_deriv, charge_deriv, grad_box


def pme_direct_double_backward(positions, charges, neighbors, deltas, distances, exclusions, v, w, alpha, coulomb, index=None):
    """Double backward of direct-space PME through the C ABI: with P = dE/dpositions, C = dE/dcharges of pme_direct and the
    cotangents v [N, 3], w [N] -> (d/dpositions [N, 3], d/dcharges [N]) of sum v . P + sum w C (deltas and distances as data).
    index: the transposed index of a list grouped by neighbors[0] (as for pme_direct).  None: any list -- any order, -1 slots
    anywhere; both sides' indices are built here from a copy with the unused entries replaced by N.  No atomics."""
    _dev_f32(positions, "positions")
    _dev_f32(charges, "charges")
    n, pairs = positions.size(0), neighbors.size(1)
    dev = positions.device
    _dev_f32(v, "v", (n, 3))
    _dev_f32(w, "w", (n,))
    exclusions = exclusions.to(device=dev, dtype=torch.int32).contiguous()
    max_excl = exclusions.size(1)
    neighbors = neighbors.to(torch.int32).contiguous()
    first_index = None
    if index is None:
        clean = torch.where(neighbors < 0, torch.full_like(neighbors, n), neighbors).contiguous()
        index = neighbor_pairs_build_index(n, clean)
        first_index = neighbor_pairs_build_index(n, clean.flip(0).contiguous())
    grad_positions = torch.empty((n, 3), dtype=torch.float32, device=dev)
    grad_charges = torch.empty((n,), dtype=torch.float32, device=dev)
    L = lib()
    ws = torch.empty((int(L.nnpops_pme_direct_double_backward_workspace_bytes(pairs, n)),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(L.nnpops_pme_direct_double_backward(n, pairs, max_excl, _ptr(positions), _ptr(charges), _ptr(neighbors),
                                                   _ptr(deltas.contiguous()), _ptr(distances.contiguous()),
                                                   _ptr(exclusions) if max_excl else None, _ptr(index),
                                                   None if first_index is None else _ptr(first_index), _ptr(v), _ptr(w), float(alpha),
                                                   float(coulomb), _ptr(grad_positions), _ptr(grad_charges), _ptr(ws), _stream_ptr(dev)))
    return grad_positions, grad_charges


def pme_reciprocal_double_backward(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli, zmoduli,
                                   v, w):
    """Double backward of reciprocal-space PME through the C ABI (steps 1-4 of pme_reciprocal, then spread_directional -> rfftn ->
    convolve -> irfftn -> interpolate_second): with the cotangents v [N, 3] of dE/dpositions and w [N] of dE/dcharges
    -> (d/dpositions [N, 3], d/dcharges [N]) of sum v . dE/dpositions + sum w dE/dcharges.  Orders 4 and 5."""
    _dev_f32(positions, "positions")
    _dev_f32(charges, "charges")
    _dev_f32(box_vectors, "box_vectors", (3, 3))
    dev = positions.device
    n = positions.size(0)
    _dev_f32(v, "v", (n, 3))
    _dev_f32(w, "w", (n,))
    mods = [_dev_f32(m.to(device=dev, dtype=torch.float32).contiguous(), name, (k,))
            for m, name, k in ((xmoduli, "xmoduli", gridx), (ymoduli, "ymoduli", gridy), (zmoduli, "zmoduli", gridz))]
    L = lib()
    dims = (gridx, gridy, gridz, order)
    ws = torch.empty((int(L.nnpops_pme_reciprocal_workspace_bytes(n, *dims)),), dtype=torch.uint8, device=dev)
    ws2 = torch.empty((int(L.nnpops_pme_reciprocal_second_workspace_bytes(n, *dims)),), dtype=torch.uint8, device=dev)
    real = torch.empty((gridx, gridy, gridz), dtype=torch.float32, device=dev)
    real2 = torch.empty_like(real)
    energy = torch.empty((1,), dtype=torch.float32, device=dev)
    grad_positions = torch.empty((n, 3), dtype=torch.float32, device=dev)
    grad_charges = torch.empty((n,), dtype=torch.float32, device=dev)

    def convolved(grid):
        recip = torch.fft.rfftn(grid).contiguous()
        _check(L.nnpops_pme_reciprocal_convolve(n, *dims, _ptr(box_vectors), float(alpha), _ptr(mods[0]), _ptr(mods[1]), _ptr(mods[2]),
                                                _ptr(recip), _ptr(energy), _ptr(ws), _stream_ptr(dev)))
        # the inverse transform in double, rounded once (as the torch op does on the device): interpolate_second differences the grid twice, and the float transform's
        # error, white across the grid, grew there with the square of the grid size
        return torch.fft.irfftn(recip.to(torch.complex128), s=(gridx, gridy, gridz), norm="forward").float().contiguous()

    with torch.cuda.device(dev):
        _check(L.nnpops_pme_reciprocal_spread(n, *dims, _ptr(positions), _ptr(charges), _ptr(box_vectors), float(coulomb), _ptr(real),
                                              _ptr(ws), _stream_ptr(dev)))
        phi = convolved(real)
        _check(L.nnpops_pme_reciprocal_spread_directional(n, *dims, _ptr(positions), _ptr(charges), _ptr(box_vectors), float(coulomb),
                                                          _ptr(v), _ptr(w), _ptr(real2), _ptr(ws), _ptr(ws2), _stream_ptr(dev)))
        phi2 = convolved(real2)
        _check(L.nnpops_pme_reciprocal_interpolate_second(n, *dims, _ptr(charges), _ptr(box_vectors), float(coulomb), _ptr(w), _ptr(phi),
                                                          _ptr(phi2), _ptr(grad_positions), _ptr(grad_charges), _ptr(ws), _ptr(ws2),
                                                          _stream_ptr(dev)))
    return grad_positions, grad_charges


# ---------------------------------------------------------------------------------------------
# SchNet CFConv (reference src/schnet/CFConv.h)
# ---------------------------------------------------------------------------------------------
class CFConvNeighbors:
    """Neighbour list of the continuous-filter convolution (reference CFConvNeighbors, CFConv.h:37-85)."""

    def __init__(self, num_atoms, cutoff, periodic=False, device=0):
        self._lib = lib()
        self._h = C.c_void_p()
        self.num_atoms, self.cutoff, self.periodic = int(num_atoms), float(cutoff), bool(periodic)
        self.batched = False
        self.num_frames = 0             # > 0: set_frames is in force; build() and CFConv.backprop_box() then take one box per frame
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        _check(self._lib.nnpops_cfconv_neighbors_create(C.byref(self._h), self.num_atoms, self.cutoff, int(self.periodic),
                                                        self.device.index))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.nnpops_cfconv_neighbors_destroy(h)
            self._h = None

    def set_molecules(self, molecule_offsets):
        """Treat the list's atoms as a batch of independent non-periodic molecules: atoms [offsets[m], offsets[m+1]) belong to
        molecule m and never pair with another molecule's (None or an empty list restores one system).  Invalidates the current build."""
        if molecule_offsets is None or len(molecule_offsets) == 0:
            _check(self._lib.nnpops_cfconv_neighbors_set_molecules(self._h, 0, None))
            self.batched = False
            return
        off = np.ascontiguousarray(molecule_offsets, dtype=np.int32)
        _check(self._lib.nnpops_cfconv_neighbors_set_molecules(self._h, int(off.shape[0]) - 1, off.ctypes.data_as(C.c_void_p)))
        self.batched = True

    def set_frames(self, frame_offsets):
        """Treat a periodic list's atoms as a batch of periodic frames, each in its own box: atoms [offsets[m], offsets[m+1]) belong
        to frame m and pair only with each other, through the minimum image of box[m]; build() then takes box [B, 3, 3] (None or an
        empty list restores one system).  Invalidates the current build."""
        if frame_offsets is None or len(frame_offsets) == 0:
            _check(self._lib.nnpops_cfconv_neighbors_set_frames(self._h, 0, None))
            self.num_frames = 0
            return
        off = np.ascontiguousarray(frame_offsets, dtype=np.int32)
        _check(self._lib.nnpops_cfconv_neighbors_set_frames(self._h, int(off.shape[0]) - 1, off.ctypes.data_as(C.c_void_p)))
        self.num_frames = int(off.shape[0]) - 1

    def box_shape(self):
        return (self.num_frames, 3, 3) if self.num_frames else (3, 3)

    def build(self, positions, box=None, check=True):
        _dev_f32(positions, "positions", (self.num_atoms, 3))
        if self.periodic and box is not None:
            _dev_f32(box, "box", self.box_shape())
        elif self.periodic and not self.num_frames:
            raise ValueError("periodic neighbour list needs box vectors")
        _check(self._lib.nnpops_cfconv_neighbors_set_stream(self._h, _stream_ptr(positions.device)))
        for _ in range(8):
            # (a non-periodic single-system list ignores a box; a batch of molecules hands it on and is refused)
            _check(self._lib.nnpops_cfconv_neighbors_build(self._h, _ptr(positions), _ptr(box if self.periodic or self.batched else None)))
            if not check:
                return
            code = self._lib.nnpops_cfconv_neighbors_check(self._h, None)
            if code == OK:
                return
            if code != ERR_CAPACITY:
                _check(code)
        raise NNPOpsHipError(ERR_CAPACITY, "neighbour buffers kept overflowing")

    def num_pairs(self):
        n = C.c_int(0)
        _check(self._lib.nnpops_cfconv_neighbors_check(self._h, C.byref(n)))
        return n.value

    def build_count(self):
        """The number of the last build (a process-wide counter; 0 before the first build)."""
        n = C.c_ulonglong(0)
        _check(self._lib.nnpops_cfconv_neighbors_build_count(self._h, C.byref(n)))
        return n.value

    def read_grid(self):
        """The cell grid of the last build() that went through one, as AniSymmetryFunctions.read_grid (blocks; diagnostics only)."""
        words = (C.c_int32 * 8)()
        _check(self._lib.nnpops_cfconv_neighbors_read_grid(self._h, words))
        return _grid_dict(words)

    def export(self):
        """-> (pair_atoms int32[2,P], distances f32[P]) of the half list {(i, j>i)}, i ascending, j ascending (host arrays)."""
        P = self.num_pairs()
        cap = max(P, 1)
        atoms = np.empty((2, cap), np.int32)
        dist = np.empty((cap,), np.float32)
        _check(self._lib.nnpops_cfconv_neighbors_export(self._h, cap, atoms.ctypes.data_as(C.c_void_p),
                                                        dist.ctypes.data_as(C.c_void_p)))
        return atoms[:, :P], dist[:P]


CFCONV_PATHS = ("vector", "matrix", "split_planes", "split_registers")


def _plan_dict(words):
    """The eight words of nnpops_cfconv_plan / nnpops_cfconv_describe (nnpops_hip.h) by name."""
    w = [int(v) for v in words]
    return dict(path=CFCONV_PATHS[w[0]], waves_fwd=w[1], lds_fwd=w[2], waves_bwd=w[3], lds_bwd=w[4], channels_per_lane=w[5],
                weights_in_lds_fwd=bool(w[6] & 1), weights_in_lds_bwd=bool(w[6] & 2), dy_scale_log2=w[7])


def cfconv_plan(width, num_gaussians, gaussian_width, activation, w1, b1, w2):
    """-> dict(path, waves_fwd, lds_fwd, waves_bwd, lds_bwd, channels_per_lane, weights_in_lds_fwd, weights_in_lds_bwd,
    dy_scale_log2): the kernels a CFConv of this shape and these weights runs and how they are launched.  Host arithmetic: needs
    no device.  Reads the NNPOPS_CFCONV_* switches as the constructor of CFConv does."""
    act = {"ssp": 0, "tanh": 1, 0: 0, 1: 1}.get(activation)
    if act is None:
        raise ValueError('Invalid value of "activation"')
    w1 = np.ascontiguousarray(w1, np.float32).reshape(-1)
    w2 = np.ascontiguousarray(w2, np.float32).reshape(-1)
    b1 = np.ascontiguousarray(b1, np.float32).reshape(-1)
    if 1 <= width <= 512 and 2 <= num_gaussians <= 256:      # (other shapes are the library's to refuse; it reads nothing then)
        assert w1.size == width * num_gaussians and w2.size == width * width and b1.size == width
    words = (C.c_int32 * 8)()
    _check(lib().nnpops_cfconv_plan(int(width), int(num_gaussians), gaussian_width, act, w1.ctypes.data_as(C.c_void_p),
                                    b1.ctypes.data_as(C.c_void_p), w2.ctypes.data_as(C.c_void_p), words))
    return _plan_dict(words)


class CFConv:
    """Continuous-filter convolution (reference CFConv, CFConv.h:109-217).  ``w1`` is the core-level
    [width][num_gaussians] array, ``w2`` is [out][in]."""

    def __init__(self, num_atoms, width, num_gaussians, cutoff, gaussian_width, activation, w1, b1, w2, b2,
                 periodic=False, device=0):
        self._lib = lib()
        self._h = C.c_void_p()
        act = {"ssp": 0, "tanh": 1, 0: 0, 1: 1}.get(activation)
        if act is None:
            raise ValueError('Invalid value of "activation"')
        self.num_atoms, self.width, self.num_gaussians = int(num_atoms), int(width), int(num_gaussians)
        w1 = np.ascontiguousarray(w1, np.float32).reshape(-1)
        w2 = np.ascontiguousarray(w2, np.float32).reshape(-1)
        b1 = np.ascontiguousarray(b1, np.float32).reshape(-1)
        b2 = np.ascontiguousarray(b2, np.float32).reshape(-1)
        assert w1.size == width * num_gaussians and w2.size == width * width and b1.size == width and b2.size == width
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        _check(self._lib.nnpops_cfconv_create(C.byref(self._h), self.num_atoms, self.width, self.num_gaussians, cutoff,
                                              int(bool(periodic)), gaussian_width, act, w1.ctypes.data_as(C.c_void_p),
                                              b1.ctypes.data_as(C.c_void_p), w2.ctypes.data_as(C.c_void_p),
                                              b2.ctypes.data_as(C.c_void_p), self.device.index))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.nnpops_cfconv_destroy(h)
            self._h = None

    def describe(self):
        """-> the dict of cfconv_plan for this handle: what its compute() and backprop() launches use."""
        words = (C.c_int32 * 8)()
        _check(self._lib.nnpops_cfconv_describe(self._h, words))
        return _plan_dict(words)

    def compute(self, neighbors, positions, x, box=None, out=None):
        _dev_f32(positions, "positions", (self.num_atoms, 3))
        _dev_f32(x, "input", (self.num_atoms, self.width))
        if out is None:
            out = torch.empty_like(x)
        _check(self._lib.nnpops_cfconv_set_stream(self._h, _stream_ptr(x.device)))
        _check(self._lib.nnpops_cfconv_compute(self._h, neighbors._h, _ptr(positions), _ptr(box), _ptr(x), _ptr(out)))
        return out

    def backprop(self, neighbors, positions, x, out_grad, box=None):
        _dev_f32(positions, "positions", (self.num_atoms, 3))
        _dev_f32(x, "input", (self.num_atoms, self.width))
        _dev_f32(out_grad, "output_grad", (self.num_atoms, self.width))
        x_grad = torch.empty_like(x)
        pos_grad = torch.empty((self.num_atoms, 3), dtype=torch.float32, device=x.device)
        _check(self._lib.nnpops_cfconv_set_stream(self._h, _stream_ptr(x.device)))
        _check(self._lib.nnpops_cfconv_backprop(self._h, neighbors._h, _ptr(positions), _ptr(box), _ptr(x), _ptr(out_grad),
                                                _ptr(x_grad), _ptr(pos_grad)))
        return x_grad, pos_grad

    def backprop_box(self, neighbors, positions, x, out_grad, box):
        """backprop() and the box-vector gradient of a periodic list -> (input_grad, position_grad, box_grad float32 (3, 3), or
        [B, 3, 3] on a list of B frames).  ``positions`` and ``box`` must be those of the list's last build()."""
        _dev_f32(positions, "positions", (self.num_atoms, 3))
        _dev_f32(x, "input", (self.num_atoms, self.width))
        _dev_f32(out_grad, "output_grad", (self.num_atoms, self.width))
        if box is not None:
            _dev_f32(box, "box", neighbors.box_shape())
        x_grad = torch.empty_like(x)
        pos_grad = torch.empty((self.num_atoms, 3), dtype=torch.float32, device=x.device)
        box_grad = torch.empty(neighbors.box_shape(), dtype=torch.float32, device=x.device)
        _check(self._lib.nnpops_cfconv_set_stream(self._h, _stream_ptr(x.device)))
        _check(self._lib.nnpops_cfconv_backprop_box(self._h, neighbors._h, _ptr(positions), _ptr(box), _ptr(x), _ptr(out_grad),
                                                    _ptr(x_grad), _ptr(pos_grad), _ptr(box_grad)))
        return x_grad, pos_grad, box_grad

    def double_backward(self, neighbors, positions, x, out_grad, gg_x=None, gg_pos=None):
        """The backward of backprop(): with cotangents ``gg_x`` (N, W) of its input gradient and ``gg_pos`` (N, 3) of its position
        gradient (either may be None = zero, not both) -> the gradients of <gg_x, x_grad> + <gg_pos, pos_grad> with respect to
        (out_grad, x, positions), the pair list of the last build() held fixed."""
        _dev_f32(positions, "positions", (self.num_atoms, 3))
        _dev_f32(x, "input", (self.num_atoms, self.width))
        _dev_f32(out_grad, "output_grad", (self.num_atoms, self.width))
        if gg_x is not None:
            _dev_f32(gg_x, "gg_input_grad", (self.num_atoms, self.width))
        if gg_pos is not None:
            _dev_f32(gg_pos, "gg_position_grad", (self.num_atoms, 3))
        d_out_grad, d_x = torch.empty_like(x), torch.empty_like(x)
        d_pos = torch.empty((self.num_atoms, 3), dtype=torch.float32, device=x.device)
        _check(self._lib.nnpops_cfconv_set_stream(self._h, _stream_ptr(x.device)))
        _check(self._lib.nnpops_cfconv_double_backward(self._h, neighbors._h, _ptr(positions), _ptr(x), _ptr(out_grad), _ptr(gg_x),
                                                       _ptr(gg_pos), _ptr(d_out_grad), _ptr(d_x), _ptr(d_pos)))
        return d_out_grad, d_x, d_pos

    def backprop_weights(self, neighbors, x, out_grad):
        """The gradients of the filter network's weights for ``out_grad`` = dL/d(output of compute) on the list's last build()
        -> (w1_grad [width][num_gaussians], b1_grad, w2_grad [out][in], b2_grad), float32 on the device."""
        _dev_f32(x, "input", (self.num_atoms, self.width))
        _dev_f32(out_grad, "output_grad", (self.num_atoms, self.width))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        w1_grad, b1_grad = new(self.width, self.num_gaussians), new(self.width)
        w2_grad, b2_grad = new(self.width, self.width), new(self.width)
        _check(self._lib.nnpops_cfconv_set_stream(self._h, _stream_ptr(x.device)))
        _check(self._lib.nnpops_cfconv_backprop_weights(self._h, neighbors._h, _ptr(x), _ptr(out_grad), _ptr(w1_grad), _ptr(b1_grad),
                                                        _ptr(w2_grad), _ptr(b2_grad)))
        return w1_grad, b1_grad, w2_grad, b2_grad

    def double_backward_weights(self, neighbors, x, out_grad, gg_x=None, gg_pos=None):
        """The weight gradients of what double_backward() differentiates: with cotangents ``gg_x`` (N, W) and ``gg_pos`` (N, 3) of
        backprop()'s two gradients (either may be None = zero, not both) -> the gradients of <gg_x, x_grad> + <gg_pos, pos_grad> with
        respect to the four weight arrays, (w1_grad [width][num_gaussians], b1_grad, w2_grad [out][in], b2_grad), float32 on the
        device, for the list's last build()."""
        _dev_f32(x, "input", (self.num_atoms, self.width))
        _dev_f32(out_grad, "output_grad", (self.num_atoms, self.width))
        if gg_x is not None:
            _dev_f32(gg_x, "gg_input_grad", (self.num_atoms, self.width))
        if gg_pos is not None:
            _dev_f32(gg_pos, "gg_position_grad", (self.num_atoms, 3))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        w1_grad, b1_grad = new(self.width, self.num_gaussians), new(self.width)
        w2_grad, b2_grad = new(self.width, self.width), new(self.width)
        _check(self._lib.nnpops_cfconv_set_stream(self._h, _stream_ptr(x.device)))
        _check(self._lib.nnpops_cfconv_double_backward_weights(self._h, neighbors._h, _ptr(x), _ptr(out_grad), _ptr(gg_x), _ptr(gg_pos),
                                                               _ptr(w1_grad), _ptr(b1_grad), _ptr(w2_grad), _ptr(b2_grad)))
        return w1_grad, b1_grad, w2_grad, b2_grad

    def set_weights(self, w1, b1, w2, b2):
        """New weights for this handle (host arrays as the constructor takes them): the plan is made again and every packed form
        uploaded again, as for a fresh handle.  Blocks on the handle's stream."""
        w1 = np.ascontiguousarray(w1, np.float32).reshape(-1)
        w2 = np.ascontiguousarray(w2, np.float32).reshape(-1)
        b1 = np.ascontiguousarray(b1, np.float32).reshape(-1)
        b2 = np.ascontiguousarray(b2, np.float32).reshape(-1)
        assert w1.size == self.width * self.num_gaussians and w2.size == self.width * self.width
        assert b1.size == self.width and b2.size == self.width
        _check(self._lib.nnpops_cfconv_set_weights(self._h, w1.ctypes.data_as(C.c_void_p), b1.ctypes.data_as(C.c_void_p),
                                                   w2.ctypes.data_as(C.c_void_p), b2.ctypes.data_as(C.c_void_p)))


# ---- dense layers (batched_nn.hip) ----
def split_planes(w, transpose=False, src_cols=None, ldp=None):
    """fp32 matrix [rows][cols] on the device -> (hi, lo) fp16 planes [R][ldp] of it (or of its transpose), ldp = the row
    length rounded up to 32, zero padded; what nnpops_gemm_split takes as its B operand.  ``src_cols``: the matrix is the first
    src_cols columns of ``w`` (its leading dimension stays w's row length); ``ldp``: a longer plane row (a multiple of 32)."""
    w = _dev_f32(w, "w")
    src_rows, ldw = w.shape
    src_cols = ldw if src_cols is None else int(src_cols)
    if not 0 < src_cols <= ldw:
        raise ValueError('"src_cols" must lie within the rows of "w"')
    rows, cols = (src_cols, src_rows) if transpose else (src_rows, src_cols)
    ldp = (cols + 31) // 32 * 32 if ldp is None else int(ldp)
    hi = torch.empty((rows, ldp), dtype=torch.float16, device=w.device)
    lo = torch.empty_like(hi)
    _check(lib().nnpops_split_planes(_stream_ptr(w.device), rows, cols, _ptr(w), ldw, int(transpose), _ptr(hi), _ptr(lo), ldp))
    return hi, lo


def _operand(t, name, dtype):
    """the device pointer of an operand given as a tensor or a view into a larger buffer (its own data pointer: a view may start
    anywhere), or NULL for None"""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError(f'"{name}" must live on the HIP device (nnpops_amd has no CPU path)')
    if t.dtype != dtype:
        raise ValueError(f'"{name}" must be {dtype}')
    return _ptr(t)


def gemm_split_strided(M, N, K, batch, A, lda, strideA, Bh, Bl, ldb, strideB, C_out, ldc, strideC, epilogue=0, bias=None, strideBias=0,
                       Y=None, ldy=0, strideY=0, prologue=0, PY=None, ldpy=0, stridePY=0, pv=None, stridePv=0, alpha=0.1, a_scale=1.0,
                       a_rows=None, c_rows=None):
    """nnpops_gemm_split with its whole argument list (nnpops_hip.h), on buffers the caller owns: every tensor stands for the address
    of its first element (a view into a larger buffer is taken where it starts), leading dimensions and strides count elements, and
    nothing is allocated, copied or checked for extent here -- the caller vouches for ``batch`` problems ``stride*`` apart with rows
    ``ld*`` apart.  A, bias, Y, PY, pv: float32; Bh, Bl: float16 planes; a_rows, c_rows: int32.  Writes C_out and returns it."""
    dev = C_out.device
    _check(lib().nnpops_gemm_split(_stream_ptr(dev), int(M), int(N), int(K), int(batch), _operand(A, "A", torch.float32), int(lda), int(strideA),
                                   _operand(Bh, "Bh", torch.float16), _operand(Bl, "Bl", torch.float16), int(ldb), int(strideB),
                                   _operand(C_out, "C_out", torch.float32), int(ldc), int(strideC), int(epilogue),
                                   _operand(bias, "bias", torch.float32), int(strideBias), _operand(Y, "Y", torch.float32), int(ldy), int(strideY),
                                   int(prologue), _operand(PY, "PY", torch.float32), int(ldpy), int(stridePY), _operand(pv, "pv", torch.float32),
                                   int(stridePv), float(alpha), float(a_scale), _operand(a_rows, "a_rows", torch.int32),
                                   _operand(c_rows, "c_rows", torch.int32)))
    return C_out


def gemm_split_last():
    """-> (bn, k_split, fast) of the calling thread's last nnpops_gemm_split launch: the tile's columns (128 or 64), 2 where eight
    waves split every K step, and whether the staging loads took the straight-line path.  Raises before the thread's first launch."""
    bn, ks, fast = C.c_int(), C.c_int(), C.c_int()
    _check(lib().nnpops_gemm_split_last(C.byref(bn), C.byref(ks), C.byref(fast)))
    return bn.value, ks.value, fast.value


def rows_dot(M, K, A, lda, w, bias, out, out_rows=None):
    """nnpops_rows_dot on buffers the caller owns (as gemm_split_strided): out[out_rows ? out_rows[m] : m] = A[m][0..K) . w + bias
    for m < M, rows of A ``lda`` floats apart.  A, w, out: float32; out_rows: int32; bias: a number.  Returns out."""
    _check(lib().nnpops_rows_dot(_stream_ptr(out.device), int(M), int(K), _operand(A, "A", torch.float32), int(lda), _operand(w, "w", torch.float32),
                                 float(bias), _operand(out, "out", torch.float32), _operand(out_rows, "out_rows", torch.int32)))
    return out


def gemm_split(a, planes, bias=None, celu_of=None, alpha=0.1, a_scale=1.0, out=None, a_rows=None, c_rows=None, rows=None):
    """out[M][N] = a[M][K] @ B, B = the planes of an [N][K] matrix (see split_planes).  ``bias``: add it and apply CELU;
    ``celu_of``: multiply by CELU'(.) of that saved activation instead.  Single problem with dense rows (gemm_split_strided takes
    the batched / strided form the torch op uses)."""
    a = _dev_f32(a, "a")
    hi, lo = planes
    m, k = a.shape
    if rows is not None:
        m = int(rows)                                            # (with a_rows: the number of mapped rows)
    n = hi.shape[0]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    epi = 1 if bias is not None else 2 if celu_of is not None else 0
    return gemm_split_strided(m, n, k, 1, a, k, 0, hi, lo, hi.shape[1], 0, out, n, 0, epilogue=epi, bias=bias, Y=celu_of, ldy=n,
                              alpha=alpha, a_scale=a_scale, a_rows=a_rows, c_rows=c_rows)


# ---- the atomic networks of a frame in two launches (mlp_fused.hip) ----
MLP_MAX_KINDS = 8


class _MlpKind(C.Structure):
    _fields_ = [("num_atoms", C.c_int), ("h1", C.c_int), ("h2", C.c_int), ("h3", C.c_int),
                ("w0", C.c_void_p), ("w2", C.c_void_p), ("w4", C.c_void_p), ("w4t", C.c_void_p), ("w2t", C.c_void_p), ("w0t", C.c_void_p),
                ("b0", C.c_void_p), ("b2", C.c_void_p), ("b4", C.c_void_p), ("w6", C.c_void_p), ("b6", C.c_void_p), ("d1", C.c_void_p),
                ("w0tm", C.c_void_p)]


class _MlpFrame(C.Structure):
    _fields_ = [("num_kinds", C.c_int), ("num_features", C.c_int), ("num_members", C.c_int), ("x", C.c_void_p), ("ldx", C.c_int),
                ("rows", C.c_void_p), ("energies", C.c_void_p), ("alpha", C.c_float), ("dx", C.c_void_p), ("lddx", C.c_int),
                ("upstream", C.c_void_p), ("dx_scale", C.c_float), ("kinds", _MlpKind * MLP_MAX_KINDS),
                ("x_groups", C.c_void_p), ("dead_groups", C.c_void_p), ("num_dead_groups", C.c_int), ("dx_partial", C.c_void_p),
                ("mean_scale", C.c_float), ("mean_out", C.c_void_p), ("mean_shift", C.c_void_p), ("mean_out_shifted", C.c_void_p),
                ("publish_word", C.c_void_p), ("publish_to", C.c_void_p), ("publish_stamp", C.c_int32), ("act_scale_log2", C.c_int),
                ("segment_offsets", C.c_void_p), ("segment_positions", C.c_void_p), ("num_segments", C.c_int),
                ("member_weights", C.c_void_p), ("member_weights_ld", C.c_int)]


MLP_GRADIENTS = ("dw0", "db0", "dw2", "db2", "dw4", "db4", "dw6", "db6")


class _MlpWeightGradKind(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in MLP_GRADIENTS]


class _MlpWeightGradOut(C.Structure):
    _fields_ = [("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("kinds", _MlpWeightGradKind * MLP_MAX_KINDS)]


class _MlpWeightGradTangentOut(C.Structure):
    _fields_ = [("t", C.c_void_p), ("ldt", C.c_int), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("tangent_energies", C.c_void_p), ("kinds", _MlpWeightGradKind * MLP_MAX_KINDS)]


MLP_PACK_STATUS_BYTES = 176
MLP_PARAMETERS = tuple(f"layer{layer}_{what}" for layer in (0, 2, 4, 6) for what in ("weights", "biases"))


class _MlpNetworks(C.Structure):
    _fields_ = [("num_kinds", C.c_int), ("num_members", C.c_int), ("num_features", C.c_int),
                ("out0", C.c_int), ("out2", C.c_int), ("in2", C.c_int), ("out4", C.c_int), ("in4", C.c_int), ("out6", C.c_int), ("in6", C.c_int),
                *[(name, C.c_void_p) for name in MLP_PARAMETERS],
                ("widths", C.c_int * (3 * MLP_MAX_KINDS)), ("live_blocks", C.c_void_p), ("num_live_blocks", C.c_int)]


def mlp_networks(shapes, widths, num_live_blocks=0):
    """The descriptor of nnpops_mlp_pack_networks for parameter arrays of these shapes (layer{0,2,4,6}_weights [kinds, M, out, in], in that
    order) and packed widths (h1, h2, h3 per kind); pointers unset.  Shapes the descriptor cannot hold are the library's to refuse."""
    w0, w2, w4, w6 = (tuple(int(v) for v in s) for s in shapes)
    nets = _MlpNetworks()
    nets.num_kinds, nets.num_members, nets.num_features = w0[0], w0[1], w0[3]
    nets.out0, nets.out2, nets.in2, nets.out4, nets.in4, nets.out6, nets.in6 = w0[2], w2[2], w2[3], w4[2], w4[3], w6[2], w6[3]
    for i, h in enumerate(list(widths)[:3 * MLP_MAX_KINDS]):
        nets.widths[i] = int(h)
    nets.num_live_blocks = int(num_live_blocks)
    return nets


def mlp_pack(w, rows, cols, transpose=False, permute=False):
    """fp32 device matrix -> the fragment planes nnpops_mlp_forward / _input_grad take as the LEFT operand of a product with
    `rows` outputs and `cols` inputs (`w` is [rows][cols], or [cols][rows] with transpose)."""
    w = _dev_f32(w, "w")
    out = torch.empty((lib().nnpops_mlp_packed_halves(rows, cols),), dtype=torch.float16, device=w.device)
    _check(lib().nnpops_mlp_pack(_stream_ptr(w.device), rows, cols, _ptr(w), w.shape[1], int(transpose), int(permute), _ptr(out)))
    return out


def _up32(v):
    return (v + 31) // 32 * 32


class FusedMLP:
    """The atomic networks of one frame (reference BatchedNN.py:37-122) on nnpops_mlp_forward / nnpops_mlp_input_grad.
    ``kinds``: one dict per species present, in the order the atoms are grouped: w0 [M,H1,F], b0 [M,H1], w2 [M,H2,H1], b2,
    w4 [M,H3,H2], b4, w6 [M,H3], b6 [M] (float32 device tensors, torch Linear layout) and ``atoms`` (int32 device tensor:
    the rows of x that hold the atoms of the kind).  Widths are zero padded to multiples of 32 here.

    ``live_groups`` (optional): the 16-column blocks of x that can be non-zero (the AEV blocks of the species the molecule
    contains).  The first layer is then packed over those columns only (nnpops_hip.h: x_groups), the others are neither read nor
    multiplied, and their gradient is written as zero; with at most 256 live columns the forward launch also forms the input
    gradient member by member (dx_partial) and input_grad() only adds the members up."""

    def __init__(self, kinds, num_features, alpha=0.1, live_groups=None, act_scale_log2=4):
        if not 1 <= len(kinds) <= MLP_MAX_KINDS:
            raise ValueError(f"1..{MLP_MAX_KINDS} kinds")
        self.x_width = int(num_features)
        self.live = None
        if live_groups is not None:
            assert self.x_width % 16 == 0, "column blocks of 16: the width of x must be a multiple of 16"
            self.live = sorted(int(g) for g in live_groups)
            cols = torch.tensor([16 * g + c for g in self.live for c in range(16)], dtype=torch.long)
            kinds = [dict(kd, w0=kd["w0"][:, :, cols.to(kd["w0"].device)].contiguous()) for kd in kinds]
            num_features = 16 * len(self.live)
        self.F, self.alpha = int(num_features), float(alpha)
        self.M = int(kinds[0]["w0"].shape[0])
        self._keep = []
        self._shapes, self._packed = [], []                   # per kind, the eight parameter arrays as given and at the packed widths
        self.frame = _MlpFrame()
        self.frame.num_kinds, self.frame.num_features, self.frame.num_members, self.frame.alpha = len(kinds), self.F, self.M, self.alpha
        self.frame.act_scale_log2 = int(act_scale_log2)       # activations are scaled by 2^-k before the fp16 split (nnpops_hip.h)
        dev = kinds[0]["w0"].device
        self.device = dev
        rows = []
        for k, kd in enumerate(kinds):
            M, H1, F = kd["w0"].shape
            H2, H3 = kd["w2"].shape[1], kd["w4"].shape[1]
            assert F == self.F and M == self.M
            h1, h2, h3 = _up32(H1), _up32(H2), _up32(H3)

            def pad(t, *shape):
                out = torch.zeros(shape, dtype=torch.float32, device=dev)
                out[tuple(slice(0, n) for n in t.shape)] = t
                return out.contiguous()
            w0, w2, w4 = pad(kd["w0"], M, h1, F), pad(kd["w2"], M, h2, h1), pad(kd["w4"], M, h3, h2)
            b0, b2, b4, w6 = pad(kd["b0"], M, h1), pad(kd["b2"], M, h2), pad(kd["b4"], M, h3), pad(kd["w6"], M, h3)
            b6 = kd["b6"].to(torch.float32).contiguous()
            planes = {
                "w0": torch.cat([mlp_pack(w0[m], h1, F) for m in range(M)]),
                "w2": torch.cat([mlp_pack(w2[m], h2, h1, permute=True) for m in range(M)]),
                "w4": torch.cat([mlp_pack(w4[m], h3, h2, permute=True) for m in range(M)]),
                "w4t": torch.cat([mlp_pack(w4[m], h2, h3, transpose=True, permute=True) for m in range(M)]),
                "w2t": torch.cat([mlp_pack(w2[m], h1, h2, transpose=True, permute=True) for m in range(M)]),
                "w0t": mlp_pack(w0.reshape(M * h1, F), F, M * h1, transpose=True, permute=True),
            }
            if self.live is not None and F <= 256:
                planes["w0tm"] = torch.cat([mlp_pack(w0[m], F, h1, transpose=True, permute=True) for m in range(M)])
            n = int(kd["atoms"].numel())
            d1 = torch.empty((max(int(lib().nnpops_mlp_d1_halves(n, M, h1)), 1),), dtype=torch.float16, device=dev)
            self._keep += [planes, b0, b2, b4, w6, b6, d1]
            self._shapes.append(((M, H1, F), (M, H1), (M, H2, H1), (M, H2), (M, H3, H2), (M, H3), (M, H3), (M,)))
            self._packed.append(((M, h1, F), (M, h1), (M, h2, h1), (M, h2), (M, h3, h2), (M, h3), (M, h3), (M,)))
            fk = self.frame.kinds[k]
            fk.num_atoms, fk.h1, fk.h2, fk.h3 = n, h1, h2, h3
            for name, t in planes.items():
                setattr(fk, name, t.data_ptr())
            fk.b0, fk.b2, fk.b4, fk.w6, fk.b6, fk.d1 = b0.data_ptr(), b2.data_ptr(), b4.data_ptr(), w6.data_ptr(), b6.data_ptr(), d1.data_ptr()
            rows.append(kd["atoms"].to(torch.int32))
        self.rows = torch.cat(rows).contiguous()
        self.frame.rows = self.rows.data_ptr()
        self.energies = torch.empty((self.rows.numel(), self.M), dtype=torch.float32, device=dev)
        self.frame.energies = self.energies.data_ptr()
        if self.live is not None:
            dead = [g for g in range(self.x_width // 16) if g not in set(self.live)]
            self.x_groups = torch.tensor(self.live, dtype=torch.int32, device=dev)
            self.dead_groups = torch.tensor(dead if dead else [0], dtype=torch.int32, device=dev)
            self.frame.x_groups, self.frame.dead_groups, self.frame.num_dead_groups = self.x_groups.data_ptr(), self.dead_groups.data_ptr(), len(dead)
            if self.F <= 256:
                self.dx_partial = torch.empty((self.M, self.rows.numel(), self.F), dtype=torch.float32, device=dev)
                self.frame.dx_partial = self.dx_partial.data_ptr()

    def forward(self, x, with_gradient=True):
        """x [atoms][>= F] float32 -> energies [grouped atoms][M] (every member's network output per atom)."""
        x = _dev_f32(x, "x")
        self.frame.x, self.frame.ldx = x.data_ptr(), x.shape[1]
        _check(lib().nnpops_mlp_forward(_stream_ptr(x.device), C.byref(self.frame), int(with_gradient)))
        return self.energies

    def energy_mean(self, scale=1.0):
        """scale * sum of the energies of the last forward(): one launch, double accumulation, fixed order."""
        out = torch.empty((1,), dtype=torch.float32, device=self.energies.device)
        _check(lib().nnpops_mlp_energy_mean(_stream_ptr(out.device), _ptr(self.energies), self.energies.numel(), float(scale), _ptr(out)))
        return out

    def energy_mean_shifted(self, shift, scale=1.0):
        """(double)(float)(scale * sum) + shift[0]: the mean of energy_mean() promoted and shifted like the reference's EnergyShifter
        (``energies + self_energies``); ``shift`` a float64 device tensor, the result float64 [1]."""
        assert shift.dtype == torch.float64 and shift.is_cuda and shift.numel() >= 1
        out = torch.empty((1,), dtype=torch.float64, device=self.energies.device)
        _check(lib().nnpops_mlp_energy_mean_shifted(_stream_ptr(out.device), _ptr(self.energies), self.energies.numel(), float(scale),
                                                    _ptr(shift), _ptr(out)))
        return out

    def input_grad(self, like, upstream=None, out=None, scale=1.0, member_weights=None, molecule_offsets=None):
        """dE/dx of the summed energies of the last forward(with_gradient=True): [atoms][F] float32 (rows of atoms that
        belong to no kind are left as they are).  With ``member_weights`` (float32 device tensor [molecules or 1][M]) the gradient of
        sum_b sum_m member_weights[b][m] E_m(molecule b) instead (nnpops_hip.h: member_weights); ``molecule_offsets`` (int32 device
        tensor [molecules + 1]) says which rows of x are which molecule, without it everything is molecule 0."""
        if out is None:
            out = torch.zeros((like.shape[0], self.x_width), dtype=torch.float32, device=like.device)
        self.frame.dx, self.frame.lddx = out.data_ptr(), out.shape[1]
        self.frame.upstream = upstream.data_ptr() if upstream is not None else None
        self.frame.dx_scale = float(scale)
        if member_weights is not None:
            member_weights = _dev_f32(member_weights, "member_weights")
        saved = self._with_weights(member_weights, molecule_offsets)
        try:
            _check(lib().nnpops_mlp_input_grad(_stream_ptr(out.device), C.byref(self.frame)))
        finally:
            self.frame.member_weights, self.frame.member_weights_ld = None, 0
            self.frame.segment_offsets, self.frame.num_segments = saved
        return out

    def _with_weights(self, member_weights, molecule_offsets):
        """sets member_weights / segment_offsets of the frame; -> what to put back"""
        saved = (self.frame.segment_offsets, self.frame.num_segments)
        if member_weights is not None:
            count = 1 if molecule_offsets is None else molecule_offsets.numel() - 1
            if member_weights.dim() != 2 or tuple(member_weights.shape) != (count, self.M):
                raise ValueError(f"member_weights must be [{count}][{self.M}]")
            self.frame.member_weights, self.frame.member_weights_ld = member_weights.data_ptr(), self.M
            if molecule_offsets is not None:
                if not (molecule_offsets.is_cuda and molecule_offsets.dtype == torch.int32 and molecule_offsets.is_contiguous()):
                    raise ValueError('"molecule_offsets" must be a contiguous int32 device tensor')
                self.frame.segment_offsets, self.frame.num_segments = molecule_offsets.data_ptr(), count
        return saved

    def weight_grad(self, member_weights=None, molecule_offsets=None):
        """The gradient of sum_b sum_m member_weights[b][m] E_m(molecule b) (all ones without the table; tables as for input_grad) with
        respect to the networks' parameters, over the x of the last forward(): one dict per kind with the eight float32 tensors
        dw0 [M,H1,F], db0 [M,H1], dw2 [M,H2,H1], db2, dw4 [M,H3,H2], db4, dw6 [M,H3], db6 [M] in the shapes the constructor was given
        (with live_groups, F counts the live columns in their order).  nnpops_mlp_weight_grad: self-contained, it leaves ``energies``
        and what input_grad() reads as they are."""
        if not self.frame.x:
            raise RuntimeError("weight_grad() reads the x of the last forward(): call forward() first")
        dev = self.device
        if member_weights is not None:
            member_weights = _dev_f32(member_weights, "member_weights")
        full = [[torch.empty(shape, dtype=torch.float32, device=dev) for shape in shapes] for shapes in self._packed]
        out = _MlpWeightGradOut()
        need = int(lib().nnpops_mlp_weight_grad_workspace_bytes(C.byref(self.frame)))
        ws = getattr(self, "_weight_ws", None)
        if ws is None or ws.numel() * 4 < need:
            ws = self._weight_ws = torch.empty((max(need // 4, 64),), dtype=torch.float32, device=dev)
        out.workspace, out.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        for k, arrays in enumerate(full):
            for name, t in zip(MLP_GRADIENTS, arrays):
                setattr(out.kinds[k], name, t.data_ptr())
        saved = self._with_weights(member_weights, molecule_offsets)
        try:
            _check(lib().nnpops_mlp_weight_grad(_stream_ptr(dev), C.byref(self.frame), C.byref(out)))
        finally:
            self.frame.member_weights, self.frame.member_weights_ld = None, 0
            self.frame.segment_offsets, self.frame.num_segments = saved
        return [{name: t[tuple(slice(0, n) for n in shape)].contiguous() for name, t, shape in zip(MLP_GRADIENTS, arrays, shapes)}
                for arrays, shapes in zip(full, self._shapes)]

    def weight_grad_tangent(self, t, member_weights=None, molecule_offsets=None, tangent_energies=False):
        """The gradient, in the networks' parameters, of  sum_b sum_m member_weights[b][m] sum_{a in b} <t_a, dE_m(a)/dx_a>  over the x of
        the last forward(): ``t`` [atoms][>= x width] float32, rows and columns as x (the cotangent of input_grad()'s result under a loss
        on forces).  Dicts as weight_grad() gives them; with ``tangent_energies`` also the float32 tensor [grouped atoms][M] of the
        unweighted <t_a, dE_m(a)/dx_a>.  nnpops_mlp_weight_grad_tangent: self-contained like weight_grad()."""
        if not self.frame.x:
            raise RuntimeError("weight_grad_tangent() reads the x of the last forward(): call forward() first")
        dev = self.device
        t = _dev_f32(t, "t")
        if t.dim() != 2 or t.shape[1] < self.x_width:
            raise ValueError(f'"t" must be [atoms][>= {self.x_width}]')
        if member_weights is not None:
            member_weights = _dev_f32(member_weights, "member_weights")
        full = [[torch.empty(shape, dtype=torch.float32, device=dev) for shape in shapes] for shapes in self._packed]
        out = _MlpWeightGradTangentOut()
        out.t, out.ldt = t.data_ptr(), t.shape[1]
        need = int(lib().nnpops_mlp_weight_grad_tangent_workspace_bytes(C.byref(self.frame)))
        ws = getattr(self, "_tangent_ws", None)
        if ws is None or ws.numel() * 4 < need:
            ws = self._tangent_ws = torch.empty((max(need // 4, 64),), dtype=torch.float32, device=dev)
        out.workspace, out.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        edot = torch.zeros((self.rows.numel(), self.M), dtype=torch.float32, device=dev) if tangent_energies else None
        out.tangent_energies = edot.data_ptr() if edot is not None and edot.numel() else None
        for k, arrays in enumerate(full):
            for name, a in zip(MLP_GRADIENTS, arrays):
                setattr(out.kinds[k], name, a.data_ptr())
        saved = self._with_weights(member_weights, molecule_offsets)
        try:
            _check(lib().nnpops_mlp_weight_grad_tangent(_stream_ptr(dev), C.byref(self.frame), C.byref(out)))
        finally:
            self.frame.member_weights, self.frame.member_weights_ld = None, 0
            self.frame.segment_offsets, self.frame.num_segments = saved
        grads = [{name: a[tuple(slice(0, n) for n in shape)].contiguous() for name, a, shape in zip(MLP_GRADIENTS, arrays, shapes)}
                 for arrays, shapes in zip(full, self._shapes)]
        return (grads, edot) if tangent_energies else grads

    @staticmethod
    def pack_networks(parameters, widths, x_blocks=None):
        """All planes of an ensemble from its eight parameter arrays in a module's layout (nnpops_mlp_pack_networks): ``parameters`` the
        float32 device tensors layer{0,2,4,6}_{weights,biases} [kinds, M, out, in], ``widths`` (h1, h2, h3) per kind, ``x_blocks`` an int32
        device tensor of live 16-column blocks or None -> (planes fp16, floats fp32, live_planes fp16 -- empty without blocks --, status
        int32 [44]; nnpops_hip.h).  Fresh tensors, two launches on the current stream, no synchronisation."""
        parameters = list(parameters)
        if len(parameters) != 8 or any(p.dim() != 4 for p in parameters):
            raise ValueError("eight [kinds, M, out, in] arrays")
        parameters = [_dev_f32(p, name) for p, name in zip(parameters, MLP_PARAMETERS)]
        dev = parameters[0].device
        blocks = 0
        if x_blocks is not None and x_blocks.numel() > 0:
            if not (x_blocks.is_cuda and x_blocks.dtype == torch.int32 and x_blocks.is_contiguous()):
                raise ValueError('"x_blocks" must be a contiguous int32 device tensor')
            blocks = int(x_blocks.numel())
        nets = mlp_networks([p.shape for p in parameters[0::2]], widths, blocks)
        if len(widths) != 3 * nets.num_kinds:
            raise ValueError("three widths per kind")
        for name, w, b in zip(MLP_PARAMETERS[0::2], parameters[0::2], parameters[1::2]):
            if tuple(b.shape) != (*w.shape[:3], 1) or tuple(w.shape[:2]) != tuple(parameters[0].shape[:2]):
                raise ValueError(f"{name}: weights [kinds, M, out, in] come with biases [kinds, M, out, 1]")
        for name, p in zip(MLP_PARAMETERS, parameters):
            setattr(nets, name, p.data_ptr())
        nets.live_blocks = x_blocks.data_ptr() if blocks else None
        sizes = [int(lib().nnpops_mlp_networks_plane_halves(C.byref(nets), 0)), int(lib().nnpops_mlp_networks_floats(C.byref(nets))),
                 int(lib().nnpops_mlp_networks_plane_halves(C.byref(nets), 1))]
        if min(sizes) < 0:
            _check(min(sizes))
        planes = torch.empty((sizes[0],), dtype=torch.float16, device=dev)
        floats = torch.empty((sizes[1],), dtype=torch.float32, device=dev)
        live = torch.empty((sizes[2],), dtype=torch.float16, device=dev)
        status = torch.empty((MLP_PACK_STATUS_BYTES // 4,), dtype=torch.int32, device=dev)
        _check(lib().nnpops_mlp_pack_networks(_stream_ptr(dev), C.byref(nets), _ptr(planes), _ptr(floats), _ptr(live) if blocks else None,
                                              _ptr(status)))
        return planes, floats, live, status


def scale_by_scalar(values, factor):
    """values (float32 device tensor) * float(factor[0]), ``factor`` a float32 or float64 DEVICE scalar: one launch
    (nnpops_scale_by_scalar -- the backward of the one-node OptimizedTorchANI step)."""
    values = _dev_f32(values, "values")
    assert factor.is_cuda and factor.dtype in (torch.float32, torch.float64) and factor.numel() >= 1
    out = torch.empty_like(values)
    _check(lib().nnpops_scale_by_scalar(_stream_ptr(values.device), _ptr(values), values.numel(), _ptr(factor),
                                        int(factor.dtype == torch.float64), _ptr(out)))
    return out


def _segment_tables(molecule_offsets, positions, num_atoms):
    for name, t in (("molecule_offsets", molecule_offsets), ("positions", positions)):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise ValueError(f'"{name}" must be a contiguous int32 device tensor')
    if molecule_offsets.numel() < 2 or positions.numel() != num_atoms:
        raise ValueError("molecule_offsets holds one entry more than there are molecules, positions one per atom")
    return molecule_offsets.numel() - 1


def mlp_energy_mean_segments(energies, molecule_offsets, positions, scale=1.0, shift=None):
    """Per-molecule means of ``energies`` [grouped atoms][members] (nnpops_mlp_energy_mean_segments): molecule b is the rows
    molecule_offsets[b] .. molecule_offsets[b + 1] - 1, ``positions[row]`` the place of a row in the grouped order.  -> float32 [B], or
    -- with ``shift``, a float64 device scalar -- float64 [B] = (double)(float)mean + shift."""
    energies = _dev_f32(energies, "energies")
    n, members = energies.shape
    count = _segment_tables(molecule_offsets, positions, n)
    if shift is None:
        out = torch.empty((count,), dtype=torch.float32, device=energies.device)
        _check(lib().nnpops_mlp_energy_mean_segments(_stream_ptr(out.device), _ptr(energies), n, members, _ptr(molecule_offsets), count,
                                                     _ptr(positions), float(scale), _ptr(out)))
        return out
    assert shift.dtype == torch.float64 and shift.is_cuda and shift.numel() >= 1
    out = torch.empty((count,), dtype=torch.float64, device=energies.device)
    _check(lib().nnpops_mlp_energy_mean_segments_shifted(_stream_ptr(out.device), _ptr(energies), n, members, _ptr(molecule_offsets), count,
                                                         _ptr(positions), float(scale), _ptr(shift), _ptr(out)))
    return out


def mlp_member_sums(energies, molecule_offsets=None, positions=None, shift=None):
    """The energy of every member, molecule by molecule (nnpops_mlp_member_sums): ``energies`` [grouped atoms][members], tables as for
    mlp_energy_mean_segments (both None: one molecule) -> float32 [B][members], or -- with ``shift`` -- float64 = (double)(float)sum + shift."""
    energies = _dev_f32(energies, "energies")
    n, members = energies.shape
    count = 1
    if molecule_offsets is not None or positions is not None:
        count = _segment_tables(molecule_offsets, positions, n)
    tables = (_ptr(molecule_offsets) if molecule_offsets is not None else None, count, _ptr(positions) if positions is not None else None)
    if shift is None:
        out = torch.empty((count, members), dtype=torch.float32, device=energies.device)
        _check(lib().nnpops_mlp_member_sums(_stream_ptr(out.device), _ptr(energies), n, members, *tables, _ptr(out)))
        return out
    assert shift.dtype == torch.float64 and shift.is_cuda and shift.numel() >= 1
    out = torch.empty((count, members), dtype=torch.float64, device=energies.device)
    _check(lib().nnpops_mlp_member_sums_shifted(_stream_ptr(out.device), _ptr(energies), n, members, *tables, _ptr(shift), _ptr(out)))
    return out


def scale_by_segment(values, molecule_offsets, factors):
    """values [atoms][3] (float32 device tensor) times the factor of the molecule each row belongs to; ``factors`` a float32 or
    float64 device tensor, one per molecule (nnpops_scale_by_segment -- the backward of the batched one-node step)."""
    values = _dev_f32(values, "values")
    assert values.dim() == 2 and values.shape[1] == 3
    assert factors.is_cuda and factors.dtype in (torch.float32, torch.float64) and factors.is_contiguous()
    count = molecule_offsets.numel() - 1
    assert molecule_offsets.is_cuda and molecule_offsets.dtype == torch.int32 and molecule_offsets.is_contiguous() and factors.numel() == count >= 1
    out = torch.empty_like(values)
    _check(lib().nnpops_scale_by_segment(_stream_ptr(values.device), _ptr(values), values.shape[0], _ptr(molecule_offsets), count,
                                         _ptr(factors), int(factors.dtype == torch.float64), _ptr(out)))
    return out
