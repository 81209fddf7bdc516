"""The weight gradients of a CFConv force loss, without a GPU: the float64 judge of tests/cfconv_force_weights_float64.py against its
closed form and against central differences of M (evaluated by first-order autograd only), the float32 witness inside half of the bar
on every case of the table, every case's kernel from the LDS formula written out by hand, and the surface:
    the library exports nnpops_cfconv_double_backward_weights and it reports a NULL handle with a message; the two ops
    operation_weights_twice / operation_periodic_weights_twice are registered with eight and nine arguments;
    CFConv(..., force_trainable=True) has the four parameters of trainable=True; force_trainable with either other flag raises
    ValueError, and so does trainable with twice_differentiable, as before.
"""
import numpy as np
import pytest
import torch

import cfconv_force_weights_float64 as ff

IDS = [c.name for c in ff.CASES]


def _case(name):
    return next(c for c in ff.CASES if c.name == name)


@pytest.mark.parametrize("case", ff.CASES, ids=IDS)
def test_autograd_equals_the_closed_form(case):
    ref = ff.reference(case)
    _, _, _, _, x, g, V, Q = ff.inputs(case)
    closed = ff.closed_form(ref["J"], ref["i"], ref["j"], ref["d"], x, g, V, Q)
    for n, e in ff.errors(closed, ref["judge"]).items():
        assert e <= 1e-11, (n, e)


@pytest.mark.parametrize("name", ["w8_g10-ssp", "w16_g8-tanh", "w32_g50_Q_only-ssp", "w24_g10_V_only-tanh", "chain17_w24_g10-tanh"])
def test_autograd_equals_central_differences(name):
    case = _case(name)
    ref = ff.reference(case)
    J = ref["J"]
    _, _, _, _, x, g, V, Q = ff.inputs(case)
    base = [t.numpy().copy() for t in (J.w1, J.b1, J.w2, J.b2)]
    rng = np.random.default_rng(17)
    h = 1e-5
    M = lambda ws: ff.M_value(J, ws, ref["i"], ref["j"], ref["d"], x, g, V, Q)
    for k, n in enumerate(ff.NAMES):
        top = np.abs(ref["judge"][n]).max()
        for _ in range(4):
            idx = tuple(int(rng.integers(s)) for s in base[k].shape)
            plus, minus = [w.copy() for w in base], [w.copy() for w in base]
            plus[k][idx] += h
            minus[k][idx] -= h
            fd = (M(plus) - M(minus)) / (2 * h)
            # central differences of a smooth function: truncation h^2 M''' / 6 and rounding 1e-16 |M| / h, both far below 1e-6 of the top
            assert abs(fd - ref["judge"][n][idx]) <= 1e-6 * top, (n, idx, fd, ref["judge"][n][idx])


@pytest.mark.parametrize("case", ff.CASES, ids=IDS)
def test_float32_witness_sits_inside_half_of_the_bar(case):
    ref = ff.reference(case)
    err = ff.errors(ref["witness"], ref["judge"])
    print(f"\n{case.name}: witness {ff.figures(err)}")
    for n, e in err.items():
        assert e <= 0.5 * ff.BAR, (n, e)
    if len(ref["i"]) == 0:
        assert not any(np.any(ref["judge"][n]) for n in ff.NAMES)
    else:
        assert all(np.any(ref["judge"][n]) for n in ff.NAMES)            # (every cotangent combination reaches every array)


def test_without_Q_the_sums_are_the_first_order_ones_with_V_for_the_input():
    import cfconv_weights_float64 as wf
    case = _case("w24_g10_V_only-tanh")
    ref = ff.reference(case)
    _, _, _, _, x, g, V, Q = ff.inputs(case)
    assert Q is None
    r = np.sqrt((ref["d"] ** 2).sum(1))
    first = wf.judge(ref["J"], ref["i"], ref["j"], r, V, g)
    for n, e in ff.errors(first, ref["judge"]).items():
        assert e <= 1e-12, (n, e)


def test_the_table_covers_both_kernels_and_their_edges():
    for c in ff.CASES:
        assert ff.expected_kernel(c.W, c.G) == c.kernel, c.name
    for kernel, tile in (("mfma", ff.TILE), ("vector", ff.TILE), ("vector", ff.VECTOR_TILE)):
        counts = {len(ff.reference(c)["i"]) for c in ff.CASES if c.kernel == kernel}
        assert {0, 1, tile - 1, tile, tile + 1} <= counts, kernel
        assert max(counts) > 256 * ff.TILE                               # more pairs than one sweep of 256 workgroups
        assert {c.act for c in ff.CASES if c.kernel == kernel} == {"ssp", "tanh"}
        assert {c.cot for c in ff.CASES if c.kernel == kernel} == {"VQ", "V", "Q"}
    # the SchNet layer takes the matrix-core kernel: 16384 + 52 * 128 + 6 * 16 * 144 + 2 * 16 * 64 + 96 floats = 152.4 KiB
    assert 4 * (16384 + 52 * 128 + 6 * 16 * 144 + 2 * 16 * 64 + 96) == 156032 <= 160 * 1024
    assert ff.expected_kernel(128, 50) == "mfma"
    assert ff.expected_kernel(128, 64) == "mfma" and ff.expected_kernel(128, 65) == "vector"
    assert ff.expected_kernel(112, 65) == "mfma"                          # (sixteen Gaussian blocks fit below W = 128)


# ---------------------------------------------------------------------------------------------- the surface, without a GPU
def test_library_exports_the_symbol_and_reports_a_null_handle():
    from nnpops_amd import capi
    L = capi.lib()
    assert "nnpops_cfconv_double_backward_weights" in capi.SIGNATURES
    assert L.nnpops_cfconv_double_backward_weights(None, None, None, None, None, None, None, None, None, None) < 0
    assert b"NULL handle" in L.nnpops_last_error()
    assert hasattr(capi.CFConv, "double_backward_weights")


def test_both_ops_are_registered():
    from nnpops_amd import torch_binding
    torch_binding.load()
    for name, old, count in (("operation_weights_twice", "operation_weights", 8),
                             ("operation_periodic_weights_twice", "operation_periodic_weights", 9)):
        schema = str(getattr(torch.ops.NNPOpsCFConv, name).default._schema)
        args = schema[schema.index("(") + 1:schema.index(") ->")]
        assert sum(a.strip().startswith("Tensor ") for a in args.split(",")) == count - 2, schema       # (holder and neighbours: classes)
        assert len(args.split(",")) == count, schema
        theirs = str(getattr(torch.ops.NNPOpsCFConv, old).default._schema)
        assert schema.replace(name, old) == theirs                        # the schema of the first-order op


HOLDER = "__torch__.torch.classes.NNPOpsCFConv.Holder? _0, Any _1"
SCHEMAS = [        # the eight ops as scripted modules saved before the nodes behind them were merged know them
    f"NNPOpsCFConv::operation({HOLDER}, Tensor _2, Tensor _3) -> Tensor _0",
    f"NNPOpsCFConv::operation_periodic({HOLDER}, Tensor _2, Tensor _3, Tensor _4) -> Tensor _0",
    f"NNPOpsCFConv::operation_twice({HOLDER}, Tensor _2, Tensor _3) -> Tensor _0",
    f"NNPOpsCFConv::operation_periodic_twice({HOLDER}, Tensor _2, Tensor _3, Tensor _4) -> Tensor _0",
    f"NNPOpsCFConv::operation_weights({HOLDER}, Tensor _2, Tensor _3, Tensor _4, Tensor _5, Tensor _6, Tensor _7) -> Tensor _0",
    f"NNPOpsCFConv::operation_periodic_weights({HOLDER}, Tensor _2, Tensor _3, Tensor _4, Tensor _5, Tensor _6, Tensor _7, Tensor _8) -> Tensor _0",
    f"NNPOpsCFConv::operation_weights_twice({HOLDER}, Tensor _2, Tensor _3, Tensor _4, Tensor _5, Tensor _6, Tensor _7) -> Tensor _0",
    f"NNPOpsCFConv::operation_periodic_weights_twice({HOLDER}, Tensor _2, Tensor _3, Tensor _4, Tensor _5, Tensor _6, Tensor _7, Tensor _8) "
    "-> Tensor _0",
]


def test_all_eight_schemas_are_the_recorded_ones():
    from nnpops_amd import torch_binding
    torch_binding.load()
    for want in SCHEMAS:
        name = want[len("NNPOpsCFConv::"):want.index("(")]
        assert str(getattr(torch.ops.NNPOpsCFConv, name).default._schema) == want
    registered = [str(s) for s in torch._C._jit_get_all_schemas() if s.name.startswith("NNPOpsCFConv::")]
    assert sorted(registered) == sorted(SCHEMAS)                          # and no ninth


def _module(**kw):
    from NNPOps.CFConv import CFConv
    G, W = 7, 5
    rng = np.random.default_rng(3)
    t = lambda *s: torch.tensor(rng.standard_normal(s).astype(np.float32))
    return CFConv(0.4, "ssp", t(G, W), t(W), t(W, W), t(W), **kw), (G, W)


def test_force_trainable_module_has_the_four_parameters_of_trainable():
    conv, (G, W) = _module(force_trainable=True)
    shapes = {n: tuple(p.shape) for n, p in conv.named_parameters()}
    assert shapes == dict(weights1=(G, W), biases1=(W,), weights2=(W, W), biases2=(W,))
    assert all(p.dtype == torch.float32 and p.requires_grad for p in conv.parameters())
    other, _ = _module(trainable=True)
    assert sorted(other.state_dict()) == sorted(conv.state_dict())
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    conv.load_state_dict(other.state_dict())                              # state dicts interchange, both ways
    other.load_state_dict(conv.state_dict())
    for a, b in zip(conv.parameters(), other.parameters()):
        assert torch.equal(a, b)
    assert conv.force_trainable and not conv.trainable and not conv.twice_differentiable


@pytest.mark.parametrize("kw", [dict(trainable=True), dict(twice_differentiable=True), dict(trainable=True, twice_differentiable=True)],
                         ids=["trainable", "twice_differentiable", "both"])
def test_force_trainable_stands_alone(kw):
    with pytest.raises(ValueError, match="force_trainable=True stands alone"):
        _module(force_trainable=True, **kw)


def test_trainable_with_twice_differentiable_still_raises_and_names_the_flag():
    with pytest.raises(ValueError, match="mixed second derivatives with respect to the filter network's weights") as e:
        _module(trainable=True, twice_differentiable=True)
    assert "force_trainable" in str(e.value)
