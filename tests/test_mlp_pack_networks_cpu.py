"""The whole-ensemble pack of the fused networks without a GPU: the library and the binding have the new entries, a bad descriptor is
refused before anything is launched, the size queries are the sizes of what the host route packs, and a trainable module on the CPU
keeps rebuilding on the host.
"""
import ctypes

import pytest
import torch

import mlp_pack_cases as P

INVALID_ARGUMENT = -1                          # NNPOPS_ERR_INVALID_ARGUMENT
SYMBOLS = ("nnpops_mlp_pack_networks", "nnpops_mlp_networks_plane_halves", "nnpops_mlp_networks_floats")


def test_library_exports_the_entries():
    from nnpops_amd import build, capi
    handle = ctypes.CDLL(build.build())
    for name in SYMBOLS:
        assert hasattr(handle, name) and name in capi.SIGNATURES
    assert ctypes.sizeof(capi._MlpNetworks) == 10 * 4 + 8 * 8 + 24 * 4 + 8 + 8      # (ten ints, eight pointers, the widths, the block list + its count, padded)
    assert capi.MLP_PACK_STATUS_BYTES == 176 and hasattr(capi.FusedMLP, "pack_networks")


def test_the_op_is_registered_with_its_schema():
    from nnpops_amd import torch_binding
    torch_binding.load()
    assert str(torch.ops.NNPOpsBatchedNN.PackNetworks.default._schema) == (
        "NNPOpsBatchedNN::PackNetworks(Tensor[] parameters, int[] widths, Tensor? x_blocks) -> "
        "(Tensor planes, Tensor floats, Tensor live_planes, Tensor status)")
    # device tensors only: there is no CPU kernel to fall back to
    from NNPOps.BatchedNN import PARAMETER_NAMES
    nets = P.module("F8", False)
    parameters = [getattr(nets, name) for name in PARAMETER_NAMES]
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.NNPOpsBatchedNN.PackNetworks(parameters, [32, 32, 32], None)


def _descriptor(**changes):
    from nnpops_amd import capi
    shapes = dict(kinds=2, members=3, F=40, out=(256, 160, 96), widths=[96, 160, 32, 256, 96, 96], blocks=0)
    shapes.update(changes)
    k, m, o = shapes["kinds"], shapes["members"], shapes["out"]
    return capi.mlp_networks([(k, m, o[0], shapes["F"]), (k, m, o[1], o[0]), (k, m, o[2], o[1]), (k, m, 1, o[2])], shapes["widths"], shapes["blocks"])


@pytest.mark.parametrize("what, changes", [
    ("width that is no multiple of 32", dict(widths=[96, 160, 48, 256, 96, 96])),
    ("width above 256", dict(widths=[96, 160, 32, 288, 96, 96])),
    ("width of zero", dict(widths=[96, 160, 32, 256, 0, 96])),
    ("F % 8", dict(F=44)),
    ("F above 1024", dict(F=1032)),
    ("nine kinds", dict(kinds=9, widths=[32] * 27)),
    ("no kind", dict(kinds=0, widths=[])),
    ("129 members", dict(members=129)),
    ("more live blocks than the input has", dict(F=48, blocks=4)),
    ("live blocks of an input that is no multiple of 16", dict(F=40, blocks=1)),
])
def test_a_bad_descriptor_is_refused_without_a_launch(what, changes):
    from nnpops_amd import capi
    lib = capi.lib()
    nets = _descriptor(**changes)
    out = (ctypes.c_char * 64)()                                       # (never written: the shape is refused first)
    for p in capi.MLP_PARAMETERS:
        setattr(nets, p, ctypes.addressof(out))
    args = [ctypes.byref(nets), ctypes.addressof(out), ctypes.addressof(out), ctypes.addressof(out), ctypes.addressof(out)]
    assert lib.nnpops_mlp_pack_networks(None, *args) == INVALID_ARGUMENT, what
    assert lib.nnpops_mlp_networks_plane_halves(ctypes.byref(nets), 0) == INVALID_ARGUMENT
    assert lib.nnpops_mlp_networks_plane_halves(ctypes.byref(nets), 1) == INVALID_ARGUMENT
    assert lib.nnpops_mlp_networks_floats(ctypes.byref(nets)) == INVALID_ARGUMENT


def test_null_pointers_are_refused_without_a_launch():
    from nnpops_amd import capi
    lib = capi.lib()
    assert lib.nnpops_mlp_pack_networks(None, None, None, None, None, None) == INVALID_ARGUMENT
    assert b"NULL network descriptor" in lib.nnpops_last_error()
    assert lib.nnpops_mlp_networks_floats(None) == INVALID_ARGUMENT and lib.nnpops_mlp_networks_plane_halves(None, 0) == INVALID_ARGUMENT
    nets = _descriptor()                                               # a good shape: the sizes are known, the pointers are missing
    assert lib.nnpops_mlp_networks_floats(ctypes.byref(nets)) > 0
    out = (ctypes.c_char * 64)()
    assert lib.nnpops_mlp_pack_networks(None, ctypes.byref(nets), ctypes.addressof(out), ctypes.addressof(out), None, ctypes.addressof(out)) == INVALID_ARGUMENT
    assert b"NULL parameter pointer" in lib.nnpops_last_error()
    for p in capi.MLP_PARAMETERS:
        setattr(nets, p, ctypes.addressof(out))
    assert lib.nnpops_mlp_pack_networks(None, ctypes.byref(nets), None, ctypes.addressof(out), None, ctypes.addressof(out)) == INVALID_ARGUMENT
    assert b"NULL output pointer" in lib.nnpops_last_error()
    nets = _descriptor(F=48, blocks=2)                                 # live blocks without their list
    for p in capi.MLP_PARAMETERS:
        setattr(nets, p, ctypes.addressof(out))
    assert lib.nnpops_mlp_pack_networks(None, ctypes.byref(nets), *[ctypes.addressof(out)] * 4) == INVALID_ARGUMENT
    assert b"live blocks need" in lib.nnpops_last_error()


@pytest.mark.parametrize("name", list(P.CASES))
def test_size_queries_are_the_host_routes_sizes(name):
    from nnpops_amd import capi
    nets = P.module(name, False)
    F, kinds, members, live = P.CASES[name]
    assert nets.widths == [(h + 31) // 32 * 32 for kind in kinds for h in kind]
    d = capi.mlp_networks([getattr(nets, f"layer{l}_weights").shape for l in (0, 2, 4, 6)], nets.widths, len(live or []))
    lib = capi.lib()
    assert lib.nnpops_mlp_networks_plane_halves(ctypes.byref(d), 0) == nets.mlp_planes.numel() > 0
    assert lib.nnpops_mlp_networks_floats(ctypes.byref(d)) == nets.mlp_floats.numel() > 0
    assert lib.nnpops_mlp_networks_plane_halves(ctypes.byref(d), 1) == nets.live_planes.numel()
    assert (nets.live_planes.numel() > 0) == (live is not None)


def test_a_trainable_module_on_the_cpu_rebuilds_on_the_host():
    nets = P.module("two-kinds", True, wide=False)
    assert nets.device_packs == 0 and not nets._packs_on_device()
    before, built = nets.mlp_planes, nets.plane_rebuilds
    with torch.no_grad():
        nets.layer2_weights.mul_(1.25)
    nets._current_planes()
    nets._current_planes()
    assert nets.plane_rebuilds == built + 1 and nets.device_packs == 0 and nets.mlp_planes is not before
    nets.load_state_dict(nets.state_dict())
    assert nets.plane_rebuilds == built + 2 and nets.device_packs == 0
