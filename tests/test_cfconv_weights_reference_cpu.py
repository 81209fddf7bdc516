"""The float64 judge of the CFConv weight gradients, pinned without a GPU, and the CPU-visible surface of the feature.

tests/cfconv_weights_float64.py holds the judge (autograd over cfconv_float64.Restatement's layer with the four arrays as leaves), the
closed form the kernels evaluate, the float32 witness and the table of cases.  Here:

    the judge's autograd gradients equal its closed form to 1e-12 of the largest entry, on every case of the table;
    they equal central differences of L in float64 for sampled entries of all four arrays;
    with the weights held, the judge's output equals the float32 oracle at cfconv_float64's bars;
    the float32 witness sits inside HALF of the GPU bar on every case (the bar of tests/test_cfconv_weights_gpu.py is not too tight for
    the chosen inputs: the worst witness error over the table is 1.0e-6 of the largest entry, 0.01 of the bar);
    the table names the kernel the LDS formula gives every layer, and each kernel family meets every pair count around its tile;
    the library exports both new symbols and each reports a NULL handle with a message; the two ops are registered with eight and nine
    Tensors; CFConv(..., trainable=True) has four parameters of the right shapes and scripts, the default has none, and trainable with
    twice_differentiable raises ValueError.
"""
import ctypes as C
from typing import Optional

import numpy as np
import pytest
import torch

import cfconv_dispatch_float64 as dispatch
import cfconv_weights_float64 as wf
from cfconv_float64 import OUT_ATOL_FRAC, OUT_RTOL, sigma_of

IDS = [c.name for c in wf.CASES]


def _inputs(case):
    return wf.layer(case.frame, case.W, case.G)


@pytest.mark.parametrize("case", wf.CASES, ids=IDS)
def test_autograd_equals_the_closed_form(case):
    ref = wf.reference(case)
    _, _, _, _, x, g = _inputs(case)
    closed = wf.closed_form(ref["J"], ref["i"], ref["j"], ref["r"], x, g)
    for n, e in wf.errors(closed, ref["judge"]).items():
        assert e <= 1e-12, (n, e)


@pytest.mark.parametrize("name", ["w8_g10-ssp", "w16_g8-tanh", "w32_g50-ssp", "chain17_w24_g10-tanh"])
def test_autograd_equals_central_differences(name):
    case = next(c for c in wf.CASES if c.name == name)
    ref = wf.reference(case)
    J = ref["J"]
    _, _, _, _, x, g = _inputs(case)
    base = [t.numpy().copy() for t in (J.w1, J.b1, J.w2, J.b2)]
    rng = np.random.default_rng(17)
    h = 1e-5
    for k, n in enumerate(wf.NAMES):
        top = np.abs(ref["judge"][n]).max()
        for _ in range(4):
            idx = tuple(int(rng.integers(s)) for s in base[k].shape)
            plus, minus = [w.copy() for w in base], [w.copy() for w in base]
            plus[k][idx] += h
            minus[k][idx] -= h
            fd = (wf.loss(J, plus, ref["i"], ref["j"], ref["r"], x, g) - wf.loss(J, minus, ref["i"], ref["j"], ref["r"], x, g)) / (2 * h)
            # central differences of a smooth function: truncation h^2 L''' / 6 and rounding 1e-16 |L| / h, both far below 1e-7 of the top
            assert abs(fd - ref["judge"][n][idx]) <= 1e-7 * top, (n, idx, fd, ref["judge"][n][idx])


@pytest.mark.parametrize("name", ["w8_g10-ssp", "w48_g7-tanh", "w64_g50-ssp"])
def test_judge_output_equals_the_float32_oracle(name):
    from oracle import CFConvNeighborsOracle, CFConvOracle
    case = next(c for c in wf.CASES if c.name == name)
    ref = wf.reference(case)
    pos, box, cutoff = wf.frame(case.frame)
    w1, b1, w2, b2, x, g = _inputs(case)
    onb = CFConvNeighborsOracle(len(pos), cutoff, False)
    onb.build(pos, None)
    oracle = CFConvOracle(len(pos), case.W, case.G, cutoff, sigma_of(case.G), case.act, w1, b1, w2, b2, periodic=False)
    out = oracle.forward(onb, pos, x, None)
    assert dispatch.bar_fractions(out, ref["judge"]["out"], OUT_RTOL, OUT_ATOL_FRAC) <= 1.0


@pytest.mark.parametrize("case", wf.CASES, ids=IDS)
def test_float32_witness_sits_inside_half_of_the_bar(case):
    ref = wf.reference(case)
    err = wf.errors(ref["witness"], ref["judge"])
    print(f"\n{case.name}: witness {wf.figures(err)}")
    for n, e in err.items():
        assert e <= 0.5 * wf.BAR, (n, e)
    if len(ref["i"]) == 0:
        assert not any(np.any(ref["judge"][n]) for n in wf.NAMES)


def test_the_table_covers_both_kernels_and_their_edges():
    for c in wf.CASES:
        assert wf.expected_kernel(c.W, c.G) == c.kernel, c.name
    for kernel in ("mfma", "vector"):
        counts = {len(wf.reference(c)["i"]) for c in wf.CASES if c.kernel == kernel}
        assert {0, 1, wf.TILE - 1, wf.TILE, wf.TILE + 1} <= counts, kernel
        assert max(counts) > 256 * wf.TILE                               # more pairs than one sweep of 256 workgroups
        assert {c.act for c in wf.CASES if c.kernel == kernel} == {"ssp", "tanh"}
    assert wf.expected_kernel(128, 104) == "mfma" and wf.expected_kernel(128, 105) == "vector"
    # the forward paths the rows name are those nnpops_cfconv_plan gives them
    from nnpops_amd import capi
    import os
    for c in wf.CASES:
        saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("NNPOPS_CFCONV_")}
        try:
            os.environ.update(dict(c.env))
            w1, b1, w2, _, _, _ = _inputs(c)
            assert capi.cfconv_plan(c.W, c.G, sigma_of(c.G), c.act, w1, b1, w2)["path"] == c.path, c.name
        finally:
            for k, _ in c.env:
                os.environ.pop(k, None)
            os.environ.update(saved)


# ---------------------------------------------------------------------------------------------- the surface, without a GPU
def test_library_exports_both_symbols_and_reports_a_null_handle():
    from nnpops_amd import capi
    L = capi.lib()
    assert "nnpops_cfconv_backprop_weights" in capi.SIGNATURES and "nnpops_cfconv_set_weights" in capi.SIGNATURES
    assert L.nnpops_cfconv_backprop_weights(None, None, None, None, None, None, None, None) < 0
    assert b"NULL handle" in L.nnpops_last_error()
    w = (C.c_float * 4)()
    assert L.nnpops_cfconv_set_weights(None, w, w, w, w) < 0
    assert b"NULL handle" in L.nnpops_last_error()
    assert hasattr(capi.CFConv, "backprop_weights") and hasattr(capi.CFConv, "set_weights")


def test_both_ops_are_registered():
    from nnpops_amd import torch_binding
    torch_binding.load()
    for name, tensors in (("operation_weights", 8), ("operation_periodic_weights", 9)):
        schema = str(getattr(torch.ops.NNPOpsCFConv, name).default._schema)
        args = schema[schema.index("(") + 1:schema.index(") ->")]
        assert sum(a.strip().startswith("Tensor ") for a in args.split(",")) == tensors - 2, schema       # (holder and neighbours: classes)
        assert len(args.split(",")) == tensors, schema


def _module(**kw):
    from NNPOps.CFConv import CFConv
    G, W = 7, 5
    rng = np.random.default_rng(3)
    t = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32))
    return CFConv(0.4, "ssp", t(G, W), t(W), t(W, W), t(W), **kw), (G, W)


class _Layer(torch.nn.Module):
    """a convolution behind its own list (a module cannot be an argument of a scripted method)"""

    def __init__(self, conv):
        super().__init__()
        from NNPOps.CFConvNeighbors import CFConvNeighbors
        self.neighbors = CFConvNeighbors(3.0)
        self.conv = conv

    def forward(self, positions, x, box: Optional[torch.Tensor] = None):
        self.neighbors.build(positions, box)
        return self.conv(self.neighbors, positions, x, box)


def test_trainable_module_has_four_parameters_and_scripts():
    conv, (G, W) = _module(trainable=True)
    shapes = {n: tuple(p.shape) for n, p in conv.named_parameters()}
    assert shapes == dict(weights1=(G, W), biases1=(W,), weights2=(W, W), biases2=(W,))
    assert all(p.requires_grad and p.dtype == torch.float32 for p in conv.parameters())
    assert sorted(conv.state_dict()) == ["biases1", "biases2", "weights1", "weights2"]
    assert conv.holder.uploads() == 0
    scripted = torch.jit.script(_Layer(conv))
    assert "operation_weights" in scripted.conv.code and "operation_periodic_weights" in scripted.conv.code
    assert sorted(n for n, _ in scripted.named_parameters()) == ["conv.biases1", "conv.biases2", "conv.weights1", "conv.weights2"]


def test_default_module_has_no_parameters():
    conv, _ = _module()
    assert list(conv.parameters()) == [] and list(conv.buffers()) == [] and len(conv.state_dict()) == 0
    assert list(_module(twice_differentiable=True)[0].parameters()) == []
    assert list(torch.jit.script(_Layer(conv)).parameters()) == []


def test_trainable_with_twice_differentiable_raises():
    with pytest.raises(ValueError, match="mixed second derivatives with respect to the filter network's weights"):
        _module(trainable=True, twice_differentiable=True)
