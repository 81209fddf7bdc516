"""Every kernel nnpops_gemm_split can launch (csrc/batched_nn.hip: 36 instantiations of gemm_h2), rows_dot and split_planes against
float64 at their dispatch edges: the table, the judge and the bars are tests/gemm_split_float64.py's (pinned without a GPU by
test_gemm_split_reference_cpu.py).  Every row goes through capi.gemm_split_strided on buffers whose filler -- NaN around the operands,
a sentinel around the output -- would show a load or a store outside the operands, and states the kernel it must have run
(capi.gemm_split_last).  Then the op and the module that use the GEMM, at widths the fused kernels do not take.

Measured on an MI355X (docs/LAB_NOTEBOOK_gemm_split.md has the worst figure per kernel): rows 1.1e-7 ... 4.4e-7 of max |C| against
the bar of 4e-6, rows_dot 9.4e-8 of sum |a w|, GroupedMLP 4.4e-7 / 7.4e-7 of its bars' scales."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gemm_split_float64 as J
import mlp_float64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def fast_env(value):
    """NNPOPS_GEMM_FAST as a row wants it (read at every call): `value`, or unset"""
    before = os.environ.pop("NNPOPS_GEMM_FAST", None)
    if value is not None:
        os.environ["NNPOPS_GEMM_FAST"] = value
    try:
        yield
    finally:
        os.environ.pop("NNPOPS_GEMM_FAST", None)
        if before is not None:
            os.environ["NNPOPS_GEMM_FAST"] = before


def _dev(t):
    return None if t is None else t.to(DEV)


def launch(name, env="row"):
    """one call of a row on fresh buffers -> (the whole C buffer on the host, the launch record)"""
    from nnpops_amd import capi
    c, ops, buf = J.CASES[name], J.operands(name), J.buffers(name)
    a_like = _dev(buf.A if c.pro == 0 else buf.PY)[c.a_off:]
    pv = _dev(buf.pv)[c.pv_off:] if c.pro == 1 else None
    C = _dev(buf.C)
    with fast_env(c.fast_env if env == "row" else env):
        capi.gemm_split_strided(c.M, c.N, c.K, c.batch,
                                a_like if c.pro == 0 else None, c.lda if c.pro == 0 else 0, c.strideA if c.pro == 0 else 0,
                                _dev(buf.Bh), _dev(buf.Bl), c.ldb, c.strideB, C, c.ldc, c.strideC,
                                epilogue=c.epi, bias=_dev(buf.bias), strideBias=c.strideBias, Y=_dev(buf.Y), ldy=c.ldy, strideY=c.strideY,
                                prologue=c.pro, PY=a_like if c.pro == 1 else None, ldpy=c.lda if c.pro == 1 else 0,
                                stridePY=c.strideA if c.pro == 1 else 0, pv=pv, stridePv=c.stridePv, alpha=c.alpha, a_scale=c.a_scale,
                                a_rows=_dev(ops.a_rows), c_rows=_dev(ops.c_rows))
        record = capi.gemm_split_last()
    return C.cpu(), record, buf.c_index


@pytest.mark.parametrize("name", J.names())
def test_row_matches_float64(name):
    c, ref = J.CASES[name], J.judge(name)
    whole, record, c_index = launch(name)
    out = whole[c_index].numpy()
    err, scale = J.figure(out, ref)
    werr, _ = J.figure(J.witness(name), ref)
    print(f"{name}: kernel {record}  error {err / scale:.2e} of max |C| = {scale:.3g}  (witness {werr / scale:.2e})")
    assert record == c.expect
    assert not np.isnan(out).any()
    outside = ~J.written(c_index, whole.numel())
    assert bool((whole[outside] == J.SENTINEL).all()), "a store outside C"
    assert err <= J.BAR * scale, (err / scale, werr / scale)
    again, record2, _ = launch(name)
    assert record2 == record and torch.equal(again.view(torch.int32), whole.view(torch.int32)), "two calls differ"
    if c.replicas:
        assert all(np.array_equal(out[b].view(np.int32), out[0].view(np.int32)) for b in range(1, c.batch)), "replicas differ"


FAST_ROWS = [f"a-e{e}p{p}-s{s}-f1" for e, p in J.COMBOS for s in (0, 1, 2)] + ["b-N129-e0p0-s0", "c-K96-e1p0", "e-layer2-w8", "e-back4-w8"]


@pytest.mark.parametrize("name", FAST_ROWS)
def test_fast_staging_off_gives_the_same_bits(name):
    """NNPOPS_GEMM_FAST=0 on a FAST-eligible row: the same arithmetic with different loads"""
    c = J.CASES[name]
    assert c.expect[2] == 1
    fast, record, c_index = launch(name)
    slow, record0, _ = launch(name, env="0")
    assert record == c.expect and record0 == c.expect[:2] + (0,)
    assert torch.equal(fast.view(torch.int32), slow.view(torch.int32))
    one, record1, _ = launch(name, env="1")
    assert record1 == c.expect and torch.equal(fast.view(torch.int32), one.view(torch.int32))


@pytest.mark.parametrize("K,a_scale", [(40, 1.0), (33, 1.0), (40, 1.0 / 16)])
def test_zero_rows_give_celu_of_the_bias_exactly(K, a_scale):
    from nnpops_amd import capi
    M, N = 129, 65
    gen = torch.Generator().manual_seed(77)
    a = torch.randn((M, K), generator=gen)
    zero = [0, 5, 63, 64, 128]
    a[zero] = 0.0
    w = torch.randn((N, K), generator=gen) / np.sqrt(K)
    bias = 0.3 * torch.randn((N,), generator=gen)
    bias[:3] = torch.tensor([0.0, 0.25, -4.0])
    out = capi.gemm_split(a.to(DEV), capi.split_planes(w.to(DEV)), bias=bias.to(DEV), a_scale=a_scale).cpu()
    rows = out[zero]
    assert all(torch.equal(rows[i].view(torch.int32), rows[0].view(torch.int32)) for i in range(1, len(zero)))
    up = bias > 0
    assert torch.equal(rows[0][up], bias[up]) and float(rows[0][0]) == 0.0
    ref = J.celu(bias.double(), 0.1)
    err = float((rows[0].double() - ref).abs().max())
    print(f"zero rows, K {K}, a_scale {a_scale}: {err:.2e} of CELU(bias), max {float(ref.abs().max()):.3g}")
    assert err <= J.BAR * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------- rows_dot, split_planes
@pytest.mark.parametrize("name", list(J.DOT_CASES))
def test_rows_dot_matches_float64(name):
    from nnpops_amd import capi
    c = J.DOT_CASES[name]
    A, w, bias, out_rows, ref, scale, wit = J.dot_operands(name)
    a_buf = J.place(A.unsqueeze(0), c.lda, 0, 0, float("nan"))
    size = 2 * c.M + 3
    for rows in (None, out_rows):
        out = torch.full((size,), J.SENTINEL, device=DEV)
        capi.rows_dot(c.M, c.K, a_buf.to(DEV), c.lda, w.to(DEV), bias, out, out_rows=_dev(rows))
        out = out.cpu()
        where = torch.arange(c.M) if rows is None else rows.long()
        err = float(np.abs(out[where].double().numpy() - ref).max())
        print(f"rows_dot {name}{' mapped' if rows is not None else ''}: {err / scale:.2e} of max sum |a w| = {scale:.3g} "
              f"(witness {np.abs(wit.astype(np.float64) - ref).max() / scale:.2e})")
        assert err <= J.ROWS_DOT_BAR * scale
        rest = torch.ones(size, dtype=torch.bool)
        rest[where] = False
        assert bool((out[rest] == J.SENTINEL).all())


@pytest.mark.parametrize("name", list(J.PLANE_CASES))
def test_split_planes_writes_the_planes_of_the_module(name):
    from nnpops_amd import capi
    from nnpops_amd.BatchedNN import _planes
    c = J.PLANE_CASES[name]
    src = J.plane_source(name)
    w = src[:, :c.cols].contiguous()
    for transpose in (False, True):
        want_hi, want_lo = _planes(w.t().contiguous() if transpose else w)
        ldp = c.ldp if not transpose else J.up32(c.rows) + 32
        hi, lo = capi.split_planes(src.to(DEV), transpose=transpose, src_cols=c.cols, ldp=ldp)
        hi, lo = hi.cpu(), lo.cpu()
        width = want_hi.shape[1]
        assert hi.shape == (want_hi.shape[0], ldp) and ldp >= width
        for got, want in ((hi, want_hi), (lo, want_lo)):
            assert torch.equal(got[:, :width].view(torch.int16), want.view(torch.int16))
            assert not got[:, width:].view(torch.int16).any(), "the padding is not +0"
    dense = capi.split_planes(w.to(DEV))                    # (the form every other test uses)
    assert torch.equal(dense[0].cpu().view(torch.int16), _planes(w)[0].view(torch.int16))


# ---------------------------------------------------------------------------------------------- the op and the module
@pytest.mark.parametrize("name", list(J.MLP_CASES))
def test_grouped_mlp_op_matches_float64(name):
    from nnpops_amd import capi
    from nnpops_amd.BatchedNN import _planes                # (importing the module registers the op)
    c = J.MLP_CASES[name]
    kinds, x, order = J.mlp_frame(name)
    judged = mlp_float64.judge([kd for kd in kinds if len(kd["atoms"])], x)
    fh, fl, bh, bl, biases, last_w, last_b = J.pack_grouped(kinds, _planes)
    xg = x.to(DEV).requires_grad_(True)
    e = torch.ops.NNPOpsBatchedNN.GroupedMLP(xg, order.to(DEV), list(c.counts), c.members, *c.widths, fh.to(DEV), fl.to(DEV), bh.to(DEV),
                                             bl.to(DEV), biases.to(DEV), last_w.to(DEV), last_b)
    after_forward = capi.gemm_split_last()
    seen = []                                               # (the record is per thread: ask on the thread the backward pass ran on)
    xg.register_hook(lambda g: seen.append(capi.gemm_split_last()))
    e.sum().backward()
    e_ref = np.zeros(len(order))
    e_ref[order.long().numpy()] = judged.e.sum(1)
    g_ref = judged.G.sum(0)
    e_err, e_scale = J.figure(e.detach().cpu().numpy(), e_ref)
    g_err, g_scale = J.figure(xg.grad.cpu().numpy(), g_ref)
    print(f"GroupedMLP {name}: energies {e_err / e_scale:.2e} of max |e| = {e_scale:.3g}, dE/dx {g_err / g_scale:.2e} of max |g| = "
          f"{g_scale:.3g}; kernels {after_forward} / {seen}")
    assert after_forward == c.forward_last and seen == [c.backward_last]
    assert e_err <= J.E_BAR * e_scale and g_err <= J.G_BAR * g_scale


def test_gemm_module_on_widths_the_fused_kernels_do_not_take():
    from nnpops_amd import capi
    from NNPOps.BatchedNN import TorchANIBatchedNN
    numbers_of = (1, 6, 8)
    table = torch.full((10,), -1, dtype=torch.long)
    for s, z in enumerate(numbers_of):
        table[z] = s

    class Converter(torch.nn.Module):
        def forward(self, inp):
            return SimpleNamespace(species=table.to(inp[0].device)[inp[0]], coordinates=inp[1])
    F, members = 50, 3
    widths = ((30, 22, 18), (26, 22, 17), (30, 22, 18))      # (padded to the widest of a layer: 30, 22, 18)
    gen = torch.Generator().manual_seed(41)
    ensemble = []
    for _ in range(members):
        nets = []
        for h1, h2, h3 in widths:
            net = torch.nn.Sequential(torch.nn.Linear(F, h1), torch.nn.CELU(0.1), torch.nn.Linear(h1, h2), torch.nn.CELU(0.1),
                                      torch.nn.Linear(h2, h3), torch.nn.CELU(0.1), torch.nn.Linear(h3, 1))
            for layer in net:
                if isinstance(layer, torch.nn.Linear):
                    layer.weight.data = torch.randn(layer.weight.shape, generator=gen) / np.sqrt(layer.in_features)
                    layer.bias.data = 0.1 * torch.randn(layer.bias.shape, generator=gen)
            nets.append(net)
        ensemble.append(torch.nn.ModuleList(nets))
    ensemble = torch.nn.ModuleList(ensemble)
    species = torch.tensor([0] * 64 + [1] + [2] * 65)[torch.randperm(130, generator=gen)]
    numbers = torch.tensor(numbers_of)[species].unsqueeze(0)
    gemm = TorchANIBatchedNN(Converter(), ensemble, numbers, layout="gemm").to(DEV)
    exact = TorchANIBatchedNN(Converter(), ensemble, numbers, layout="grouped").double().to(DEV)
    assert gemm[0].fused_ok and (gemm[0].h1, gemm[0].h2, gemm[0].h3) == (30, 22, 18)
    sp = species.to(DEV).unsqueeze(0)
    aev = torch.randn((1, 130, F), generator=gen).abs().to(DEV)
    # a FAST launch first: the module's last forward GEMM (K = 22) is not, so the record shows that it ran
    capi.gemm_split(aev[0, :, :48].contiguous(), capi.split_planes(torch.zeros((8, 48), device=DEV)))
    assert capi.gemm_split_last() == (64, 2, 1)
    a1, a2 = aev.clone().requires_grad_(True), aev.double().requires_grad_(True)
    e1 = gemm((sp, a1)).energies
    assert capi.gemm_split_last() == (64, 2, 0), "the split GEMM did not run (library fallback?)"
    e2 = exact((sp, a2)).energies
    e1.sum().backward()
    e2.sum().backward()
    g_err, g_scale = J.figure(a1.grad.cpu().numpy(), a2.grad.cpu().numpy())
    v1, v2 = float(e1.detach()), float(e2.detach())
    print(f"layout='gemm': energy {abs(v1 - v2):.2e} of {abs(v2):.3g}, dE/dAEV {g_err / g_scale:.2e} of max {g_scale:.3g}")
    assert e1.dtype == torch.float32 and abs(v1 - v2) <= 1e-5 * abs(v2) + 1e-4
    assert g_err <= J.G_BAR * g_scale


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from nnpops_amd import capi
    M, N, K = 8, 8, 32
    a = torch.ones((M, K), device=DEV)
    hi, lo = capi.split_planes(torch.ones((N, K), device=DEV))
    out = torch.zeros((M, N), device=DEV)
    vec = torch.ones((max(N, K),), device=DEV)
    rows = torch.arange(M, dtype=torch.int32, device=DEV)
    capi.gemm_split(a, (hi, lo), out=out)
    record = capi.gemm_split_last()

    def call(M=M, N=N, K=K, batch=1, ldb=K, **kw):
        return capi.gemm_split_strided(M, N, K, batch, a, K, 0, hi, lo, ldb, 0, out, N, 0, **kw)
    for message, kw in (
            ("row maps are for single problems", dict(batch=2, a_rows=rows)),
            ("row maps are for single problems", dict(batch=2, c_rows=rows)),
            ("planes need ldb >= K rounded up to 32", dict(ldb=36)),
            ("planes need ldb >= K rounded up to 32", dict(K=33, ldb=40)),
            ("unknown epilogue / prologue", dict(epilogue=3, bias=vec, Y=out, ldy=N)),
            ("unknown epilogue / prologue", dict(prologue=2, PY=a, ldpy=K, pv=vec)),
            ("bias \\+ CELU epilogue needs a bias", dict(epilogue=1)),
            ("CELU' epilogue needs the saved activation", dict(epilogue=2)),
            ("alpha and a_scale must be positive", dict(alpha=0.0)),
            ("alpha and a_scale must be positive", dict(alpha=-0.1)),
            ("alpha and a_scale must be positive", dict(a_scale=0.0)),
            ("empty GEMM", dict(M=0)),
            ("empty GEMM", dict(N=0)),
            ("empty GEMM", dict(K=0)),
            ("empty GEMM", dict(batch=0))):
        with pytest.raises(capi.NNPOpsHipError, match=message):
            call(**kw)
        assert capi.gemm_split_last() == record             # (a refused call launches nothing and leaves the record)
    with pytest.raises(capi.NNPOpsHipError, match="empty problem or NULL device pointer"):
        capi.rows_dot(0, K, a, K, vec, 0.0, out)
    torch.cuda.synchronize()
    assert float(out.sum()) == M * N * K                    # (nothing was written since the one good call)
