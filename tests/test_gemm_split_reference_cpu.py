"""Pins tests/gemm_split_float64.py (the judge, the witness and the table test_gemm_split_gpu.py runs) without a GPU: the judge against
an independent formulation (torch.nn.functional.celu, autograd for CELU', one numpy product per batch entry), every row's stated
kernel against a restatement of the dispatch rule of nnpops_gemm_split, the table's coverage of every reachable kernel and every
listed edge by set comparison, the witness (the split-fp16 algorithm in float32 on the CPU) inside HALF the bar on every row, and the
exported symbols and argument tables of the wrappers."""
import inspect
import itertools
import os
import re
import threading

import numpy as np
import pytest
import torch

import gemm_split_float64 as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the dispatch rule, restated
def rule(M, N, batch):
    """-> shape 0 / 1 / 2 of a problem (batched_nn.hip: choose_launch)"""
    tiles_m = -(-M // 64)
    if -(-N // 128) * tiles_m * batch >= 512:
        return 0
    if -(-N // 64) * tiles_m * batch >= 600:
        return 1
    return 2


CAUSES = ("K % 8", "lda % 4", "base", "strideA % 4", "pv base", "stridePv % 4", "NNPOPS_GEMM_FAST=0")


def causes_of_non_fast(c):
    """which of the seven conditions of the FAST staging a row breaks (buffers come 16-byte aligned from the allocator: a base is
    aligned iff its offset is a multiple of 4 floats)"""
    out = []
    if c.K % 8:
        out.append("K % 8")
    if c.lda % 4:
        out.append("lda % 4")
    if c.a_off % 4:
        out.append("base")
    if c.batch > 1 and c.strideA % 4:
        out.append("strideA % 4")
    if c.pro == 1 and c.pv_off % 4:
        out.append("pv base")
    if c.pro == 1 and c.stridePv % 4:
        out.append("stridePv % 4")
    if c.fast_env is not None and int(c.fast_env) == 0:
        out.append("NNPOPS_GEMM_FAST=0")
    return out


@pytest.mark.parametrize("name", J.names())
def test_every_row_states_the_kernel_the_rule_gives(name):
    c = J.CASES[name]
    shape = rule(c.M, c.N, c.batch)
    assert c.expect == (128 if shape == 0 else 64, 2 if shape == 2 else 1, int(not causes_of_non_fast(c))), (shape, causes_of_non_fast(c))
    # what the entry point refuses, and what the loads need that it does not check
    assert c.ldb % 8 == 0 and c.ldb >= J.up32(c.K) and c.strideB % 8 == 0
    assert c.batch == 1 or not (c.a_rows or c.c_rows)
    assert c.M * c.N * c.K * c.batch <= 3.0e8, "a row is a GEMM of at most a few million multiply-adds per problem"


def test_the_table_holds_every_reachable_kernel():
    have = {(c.epi, c.pro, J.shape_of(c), c.expect[2]) for c in J.CASES.values()}
    every = set(itertools.product((0, 1, 2), (0, 1), (0, 1, 2), (0, 1)))
    assert len(every) == 36 and have == every - set(J.UNREACHABLE_KERNELS)
    assert J.UNREACHABLE_KERNELS == ()
    # ... each of them also on dense operands (section a) and, but for the two combined kernels, at the edges
    assert {(c.epi, c.pro, J.shape_of(c), c.expect[2]) for c in J.CASES.values() if c.section == "a"} == every


def test_the_unreachable_cells_are_exactly_the_listed_ones():
    """(shape 1, N <= 64): searched over every M up to 40 tiles and every batch up to 1200"""
    cells = {(s, n) for s in (0, 1, 2) for n in set(J.N_EDGES[0]) | set(J.N_EDGES[2])}
    reachable = set()
    for s, n in cells:
        if any(rule(M, n, b) == s for M in (1, 64, 65, 640, 2560) for b in range(1, 1201)):
            reachable.add((s, n))
    assert cells - reachable == set(J.UNREACHABLE)


def test_the_table_holds_every_listed_edge():
    rows = list(J.CASES.values())
    plain = [c for c in rows if (c.epi, c.pro) == (0, 0)]
    for s in (0, 1, 2):
        mine = [c for c in plain if J.shape_of(c) == s]
        assert {c.M for c in mine} >= set(J.M_EDGES)
        assert {c.K for c in mine if c.expect[2] == 1} >= set(J.K_FAST)
        assert {c.K for c in mine if c.expect[2] == 0} >= set(J.K_SLOW)
    assert {c.N for c in plain if J.shape_of(c) == 0} >= {1, 63, 64, 65, 127, 128, 129}
    assert {c.N for c in plain if J.shape_of(c) == 2} >= {1, 15, 16, 17, 63, 64, 65}
    wanted = {(1, n) for n in (1, 15, 16, 17, 63, 64, 65)} - set(J.UNREACHABLE)
    assert {(1, c.N) for c in plain if J.shape_of(c) == 1} >= wanted == {(1, 65)}
    # what shape 1 cannot have as N it has as the width of its last tile
    assert {(c.N - 1) % 64 + 1 for c in plain if J.shape_of(c) == 1} >= {1, 15, 16, 17, 63, 64}
    for epi, pro in J.VARIANTS[1:]:                        # once with each fused epilogue and the prologue, in every shape
        mine = [c for c in rows if (c.epi, c.pro) == (epi, pro) and c.section.startswith("b")]
        assert {c.M for c in mine} >= set(J.M_EDGES)
        assert {(c.N - 1) % 64 + 1 for c in mine if J.shape_of(c) != 0} >= {1, 15, 16, 17, 63, 64}
        assert {c.N for c in mine if J.shape_of(c) == 0} >= {1, 63, 64, 65, 127, 128, 129}
        assert {c.K for c in mine if c.expect[2] == 1} >= set(J.K_FAST)
        assert {c.K for c in mine if c.expect[2] == 0} >= set(J.K_SLOW)
        assert {J.shape_of(c) for c in mine} == {0, 1, 2}
    for epi, pro in J.VARIANTS:                            # K under the K-splitting kernel
        assert {c.K for c in rows if (c.epi, c.pro) == (epi, pro) and c.expect[:2] == (64, 2) and c.M > 64 and c.N > 64} >= set(J.K_SPLIT)
    # both staging branches of the non-FAST kernels: 16-byte loads for whole groups (lda % 4 == 0) and scalar loads
    slow = [c for c in rows if c.expect[2] == 0]
    assert any(c.lda % 4 == 0 and c.K > 8 for c in slow) and any(c.lda % 4 for c in slow)


def test_every_cause_of_non_fast_stands_alone():
    alone = {}
    for c in J.CASES.values():
        if c.section == "d" and c.expect[2] == 0:
            why = causes_of_non_fast(c)
            assert len(why) == 1, (c.name, why)
            assert (c.epi or c.pro) and c.batch > 1, c.name
            alone.setdefault(why[0], []).append(c.name)
    assert set(alone) == set(CAUSES), alone
    assert J.CASES["d-batch1-strideA"].expect[2] == 1      # (a stride that would break FAST does not count with batch 1)


def test_layouts_scales_and_replicas_are_in_the_table():
    rows = list(J.CASES.values())
    # members interleaved in a row: the stride of a member is its width, the leading dimension all members' widths
    inter = [c for c in rows if c.batch > 1 and c.strideA == c.K and c.lda == c.batch * c.K and c.strideC == c.N and c.ldc == c.batch * c.N]
    assert {(c.epi, c.pro) for c in inter} >= {(1, 0), (2, 0), (2, 1)} and {c.expect[2] for c in inter} == {0, 1}
    assert all(c.strideBias == c.N for c in inter if c.epi == 1)
    assert any(c.a_rows and c.epi == 1 for c in rows) and any(c.c_rows and c.epi == 0 for c in rows)
    assert {c.a_scale for c in rows} == {1.0, 1.0 / 16, 2.0 ** -6}
    assert all(c.amp == 3.0e4 for c in rows if c.a_scale == 2.0 ** -6) and {J.shape_of(c) for c in rows if c.amp == 3.0e4} == {0, 1, 2}
    assert {c.alpha for c in rows} == {0.1, 0.5}
    assert {J.shape_of(c) for c in rows if c.replicas} == {0, 1, 2}
    assert all(c.strideA == 0 and c.strideB == 0 and c.strideC >= c.M * c.ldc for c in rows if c.replicas)
    # leading dimensions beyond the widths on most rows, the widths themselves on the dense ones
    assert sum(c.lda > c.K and c.ldc > c.N and c.ldb > J.up32(c.K) for c in rows) >= 150
    assert sum(c.lda == c.K and c.ldc == c.N and c.ldb == J.up32(c.K) for c in rows) >= 36


# ---------------------------------------------------------------------------------------------- the judge
def test_celu_and_its_derivative_from_the_output_match_torch():
    gen = torch.Generator().manual_seed(1)
    for alpha in (0.1, 0.5, 1.0):
        u = (2.0 * torch.randn(4000, generator=gen, dtype=torch.float64)).requires_grad_(True)
        y = torch.nn.functional.celu(u, alpha=alpha)
        y.sum().backward()
        assert float((J.celu(u.detach(), alpha) - y.detach()).abs().max()) <= 1e-15
        # (autograd's CELU' carries a float32 rounding of alpha, 1.5e-8 relative, even in float64; the bar is 4e-6)
        assert float((J.celu_grad_from_output(y.detach(), alpha) - u.grad).abs().max()) <= 1e-7
    # continuous at 0: the two branches agree there
    assert float(J.celu_grad_from_output(torch.zeros(1, dtype=torch.float64), 0.1)) == 1.0


def _independent(name):
    """C_b = epi(pro(A_b) B_b^T), one numpy product per batch entry, torch's own CELU, CELU' by autograd at the pre-activation the
    saved output came from (u = y for y > 0, alpha log1p(y / alpha) otherwise)"""
    c, ops = J.CASES[name], J.operands(name)

    def grad_of(y):
        y = y.double()
        # (a saturated activation is float32(-alpha), a hair below -alpha: its pre-activation is -inf, its CELU' 0 instead of -1.5e-8)
        u = torch.where(y > 0, y, c.alpha * torch.log((y.clamp(max=0.0) / c.alpha + 1.0).clamp(min=0.0))).requires_grad_(True)
        torch.nn.functional.celu(u, alpha=c.alpha).sum().backward()
        return u.grad.numpy()
    out = np.zeros((c.batch, c.M, c.N))
    for b in range(c.batch):
        s = 0 if c.replicas else b
        rows = np.arange(c.M) if ops.a_rows is None else ops.a_rows.numpy()
        if c.pro == 0:
            A = ops.A[s].double().numpy()[rows]
        else:
            A = ops.pv[s].double().numpy()[None, :] * grad_of(ops.PY[s])[rows]
        v = A @ ops.W[s].double().numpy().T
        if c.epi == 1:
            v = torch.nn.functional.celu(torch.from_numpy(v + ops.bias[s].double().numpy()[None, :]), alpha=c.alpha).numpy()
        elif c.epi == 2:
            v = v * grad_of(ops.Y[s])
        out[b] = v
    return out


@pytest.mark.parametrize("name", [n for n in J.names() if J.CASES[n].section in "adefg" and J.CASES[n].batch <= 128])
def test_the_judge_matches_an_independent_formulation(name):
    ref = J.judge(name)
    other = _independent(name)
    assert ref.shape == other.shape and np.isfinite(ref).all()
    # (nothing differs but CELU' of saturated activations, by 1.5e-8 of the factor it scales: forty times below the bar)
    assert np.abs(ref - other).max() <= 1e-7 * np.abs(ref).max()


@pytest.mark.parametrize("name", J.names())
def test_the_witness_is_inside_half_the_bar(name):
    ref, wit = J.judge(name), J.witness(name)
    err, scale = J.figure(wit, ref)
    print(f"{name}: witness {err / scale:.2e} of max |C| = {scale:.3g}")
    assert wit.dtype == np.float32 and np.isfinite(wit).all() and scale > 0.05
    assert err <= 0.5 * J.BAR * scale


def test_split_is_what_the_module_splits():
    from nnpops_amd.BatchedNN import _planes
    w = J.plane_source("70x50")[:, :50].contiguous()
    hi, lo = _planes(w)
    mine = J.split(w)
    assert torch.equal(hi[:, :50], mine[0]) and torch.equal(lo[:, :50], mine[1])
    assert not hi[:, 50:].any() and not lo[:, 50:].any() and hi.shape == (70, 64)
    p_hi, p_lo = J.planes(w.unsqueeze(0), 72)
    assert torch.equal(p_hi[0, :, :64], hi) and torch.equal(p_lo[0, :, :64], lo) and torch.isnan(p_hi[0, :, 64:]).all()
    # values of the source: fp16 subnormals, normals, zeros; nothing overflows
    v = w.abs()
    assert (v == 0).any() and ((v > 0) & (v < 6.0e-8)).any() and ((v > 6.0e-8) & (v < 6.1e-5)).any() and (v > 1.0e3).any()
    assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()
    big = J.PLANE_CASES["1100x1000"]
    assert big.rows * J.up32(big.cols) > 4096 * 256 and big.cols * J.up32(big.rows) > 4096 * 256


@pytest.mark.parametrize("name", ["a-e1p0-s2-f1", "d-base-off1", "e-layer2-odd", "e-back4-w8", "e-both-maps", "g-e2p1-s2"])
def test_buffers_hold_the_operands_where_the_row_says(name):
    c, ops, buf = J.CASES[name], J.operands(name), J.buffers(name)
    nb = 1 if c.replicas else c.batch
    a_like, a_buf = (ops.A, buf.A) if c.pro == 0 else (ops.PY, buf.PY)
    idx = J.index(nb, a_like.shape[1], c.K, c.lda, c.strideA, c.a_off)
    assert torch.equal(a_buf[idx], a_like)
    mask = J.written(idx, a_buf.numel())
    assert torch.isnan(a_buf[~mask]).all() and int((~mask).sum()) >= J.TAIL_ROWS * c.lda
    assert (buf.C == J.SENTINEL).all() and buf.c_index.shape == (c.batch, c.M, c.N) and int(buf.c_index.max()) < buf.C.numel()
    kpad = J.up32(c.K)
    planes = buf.Bh[:(nb - 1) * c.strideB + c.N * c.ldb]
    first = planes[:c.N * c.ldb].view(c.N, c.ldb)
    assert torch.equal(first[:, :c.K], J.split(ops.W[0])[0]) and not first[:, c.K:kpad].any() and torch.isnan(first[:, kpad:]).all()


@pytest.mark.parametrize("section", sorted({c.section for c in J.CASES.values()}))
def test_every_access_of_a_call_lies_inside_its_buffers(section):
    """the farthest element each operand's addressing reaches (batch, stride, leading dimension, row maps, the planes' padding)
    against the buffer the GPU file passes: the kernels read nothing beyond it on either staging path"""
    for name in J.names(section):
        c, ops, buf = J.CASES[name], J.operands(name), J.buffers(name)
        last = c.batch - 1
        rows_a = c.rows if c.a_rows else c.M
        a_buf = buf.A if c.pro == 0 else buf.PY
        assert c.a_off + last * c.strideA + (rows_a - 1) * c.lda + c.K <= a_buf.numel(), name
        for planes in (buf.Bh, buf.Bl):
            assert last * c.strideB + (c.N - 1) * c.ldb + J.up32(c.K) <= planes.numel(), name
        if c.pro == 1:
            assert c.pv_off + last * c.stridePv + c.K <= buf.pv.numel(), name
        if c.epi == 1:
            assert last * c.strideBias + c.N <= buf.bias.numel(), name
        if c.epi == 2:
            assert last * c.strideY + (c.M - 1) * c.ldy + c.N <= buf.Y.numel(), name
        rows_c = c.rows if c.c_rows else c.M
        assert last * c.strideC + (rows_c - 1) * c.ldc + c.N <= buf.C.numel(), name
        for rows in (ops.a_rows, ops.c_rows):
            assert rows is None or (len(rows) == c.M and 0 <= int(rows.min()) and int(rows.max()) < c.rows)


# ---------------------------------------------------------------------------------------------- rows_dot
@pytest.mark.parametrize("name", list(J.DOT_CASES))
def test_rows_dot_witness_is_inside_half_the_bar(name):
    c = J.DOT_CASES[name]
    A, w, bias, out_rows, ref, scale, wit = J.dot_operands(name)
    assert c.vector == (c.K % 4 == 0 and c.lda % 4 == 0)
    assert len(set(out_rows.tolist())) == c.M and int(out_rows.max()) < 2 * c.M + 3
    assert np.abs(wit.astype(np.float64) - ref).max() <= 0.5 * J.ROWS_DOT_BAR * scale


def test_rows_dot_cases_cover_the_listed_sizes():
    cases = list(J.DOT_CASES.values())
    assert {c.M for c in cases} == {1, 3, 4, 5, 9}
    assert {c.K for c in cases if c.vector} == {4, 252, 256, 260, 1280}
    assert {c.K for c in cases if not c.vector} >= {1, 63, 65, 130}
    assert any(c.K % 4 == 0 and c.lda % 4 for c in cases)
    assert all(c.lda > c.K for c in cases)


# ---------------------------------------------------------------------------------------------- the exported surface
def _c_arguments(entry):
    header = open(os.path.join(ROOT, "include", "nnpops_hip.h")).read()
    m = re.search(r"\bint " + entry + r"\(([^;]*)\);", header)
    assert m, entry
    return [re.split(r"[\s*]+", a.strip())[-1] for a in m.group(1).replace("\n", " ").split(",")]


def test_exported_symbols_and_wrapper_arguments():
    from nnpops_amd import capi
    handle = capi.lib()
    for name in ("nnpops_gemm_split", "nnpops_gemm_split_last", "nnpops_rows_dot", "nnpops_split_planes"):
        assert hasattr(handle, name) and name in capi.SIGNATURES
        assert len(capi.SIGNATURES[name][1]) == len(_c_arguments(name)), name
    # the wrappers take the C entries' arguments, in their order, without the stream (C is capi's name for ctypes: C_out)
    want = [a if a != "C" else "C_out" for a in _c_arguments("nnpops_gemm_split")[1:]]
    assert list(inspect.signature(capi.gemm_split_strided).parameters) == want and len(want) == 30
    assert list(inspect.signature(capi.rows_dot).parameters) == _c_arguments("nnpops_rows_dot")[1:]
    assert _c_arguments("nnpops_gemm_split_last") == ["bn", "k_split", "fast"]
    assert list(inspect.signature(capi.gemm_split).parameters) == ["a", "planes", "bias", "celu_of", "alpha", "a_scale", "out", "a_rows",
                                                                   "c_rows", "rows"]


def test_the_launch_record_is_an_error_before_a_threads_first_launch():
    from nnpops_amd import capi
    seen = []

    def ask():
        try:
            seen.append(capi.gemm_split_last())
        except capi.NNPOpsHipError as e:
            seen.append(str(e))
    t = threading.Thread(target=ask)
    t.start()
    t.join()
    assert len(seen) == 1 and isinstance(seen[0], str) and "no nnpops_gemm_split launch on this thread yet" in seen[0], seen


def test_grouped_mlp_cases_are_widths_the_fused_kernels_do_not_take():
    import mlp_float64
    for c in J.MLP_CASES.values():
        assert c.F % 8 or any(h % 8 for h in c.widths)
        assert 0 in c.counts and {1, 64, 65} <= set(c.counts) and c.members == 3
        kinds, x, order = J.mlp_frame(c.name)
        assert sorted(order.tolist()) == list(range(sum(c.counts))) and x.shape == (sum(c.counts), c.F)
        judged = mlp_float64.judge([kd for kd in kinds if len(kd["atoms"])], x)
        r = mlp_float64.check_frame(judged)
        assert r.e_scale > 0.1
        # the kernels the op's last GEMMs run, from the rule: forward layer 4 (members interleaved), backward dx = d1 W0
        h1, h2, h3 = c.widths
        last = [n for n in c.counts if n][-1]
        fwd_fast = h2 % 8 == 0 and (c.members * h2) % 4 == 0 and h2 % 4 == 0
        bwd_fast = (c.members * h1) % 8 == 0
        assert c.forward_last == (64, 2, int(fwd_fast)) and rule(last, h3, c.members) == 2
        assert c.backward_last == (64, 2, int(bwd_fast)) and rule(last, c.F, 1) == 2
