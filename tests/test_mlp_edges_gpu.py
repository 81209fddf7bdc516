"""The fused atomic networks (mlp_fused.hip, through capi.FusedMLP and the C ABI only) against tests/mlp_float64.py's float64 judge
where their loops change phase ("The fused networks at their edges"):

  a  layer 0: every K-step count modulo the four rotating weight sets, the clamped prologue (one and two steps), input tails of 8, 16
     and 24 columns, the last entry of the column-block table (F = 1024), gradient chunks filled exactly and by half a row block;
  b  the resident layers: every step count 1..8 in every layer position, every row-block count, waves that own no block;
  c  the gradient's K loop over members: one step in all, a weighted fold at every step, 128 members and the refusal of 129, weights
     per molecule with three molecules in one tile -- by the separate launch and by the launch that adds up the forward's shares;
  d  leading dimensions beyond the widths with NaN behind x and a sentinel behind dx, the device scalar `upstream` times `scale`, in all
     four gradient writers;
  e  CELU driven into both ends for three alphas at the smallest and the largest activation scale;
  f  eight kinds with empty ones first and last, nine refused, a frame with no atom at all.

Every judged case: finite; energies within 1e-5 of max |e|, gradients within 1e-4 of the (weighted) magnitude -- the project's bars;
the energy-only launch gives the same bits; a second forward + input_grad gives the same bits; and the WITNESS bar
err <= C * err_float32 + 1e-7 * scale, err_float32 the error of the same sums in float32 torch on the CPU (the form of
test_batched_nn_gpu.py), which is what notices a product the split arithmetic dropped: the fixed bars are loose enough to let one pass.
C per section: WITNESS below, next to the measured worst ratios (docs/LAB_NOTEBOOK_mlp_edges.md).  `pytest -s` prints a line per case.
"""
import numpy as np
import pytest
import torch

import mlp_float64 as f64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.25

# section -> C of the witness bar.  3 is test_batched_nn_gpu.py's; a section measured above 3 gets twice its worst ratio, rounded up,
# never more than 16.  Worst ratios measured on the MI355X, (err - 1e-7 scale) / err_float32, energies / gradients:
#   a 0.95 / 1.43   b 1.80 / 3.22 (8-40-17: sums of 8 and 17 terms)   c 0.94 / 1.85   d 0.77 / 0.98   e 0.81 / 3.79 (act_scale_log2 = 12:
#   gradients scaled into fp16's subnormals)   f 0.85 / 1.69
WITNESS = {"a": 3, "b": 7, "c": 3, "d": 3, "e": 8, "f": 3}


def _mlp(fr, kinds=None):
    from nnpops_amd.capi import FusedMLP
    c = fr.case
    kinds_dev = [{k: v.to(DEV) for k, v in kd.items()} for kd in (kinds or fr.kinds)]
    return FusedMLP(kinds_dev, c.x_width or c.F, alpha=c.alpha, live_groups=c.live, act_scale_log2=c.k)


def _weights(fr, variant):
    """-> (member_weights [B][M] float32 numpy or None, molecule of every row of x or None, offsets or None)"""
    c = fr.case
    if variant == "plain":
        return None, None, None
    if variant == "weighted":
        return f64.random_weights(1, c.M, c.seed), None, None
    mol = f64.molecule_of_rows(f64.MOLECULES, np.minimum(np.arange(fr.x.shape[0]), f64.MOLECULES[-1] - 1))       # (rows 70.. hold no atom)
    return f64.random_weights(3, c.M, c.seed), mol, f64.MOLECULES


def _judged(name, variants=("plain",), padded=False, upstream=None, scale=1.0):
    """one case of the table through forward and every gradient `variant`, all assertions of the module's docstring"""
    fr = f64.frame(name)
    c, J = fr.case, fr.J
    mlp = _mlp(fr)
    rows, x_width = fr.x.shape
    if padded:                                   # NaN behind every row of x -- and in the column blocks no network reads
        x = torch.full((rows, x_width + 12), float("nan"))
        x[:, fr.columns] = fr.x[:, fr.columns]
        x = x.to(DEV)
    else:
        x = fr.x.to(DEV).contiguous()
    up = torch.tensor([upstream], dtype=torch.float32, device=DEV) if upstream is not None else None
    factor = (1.0 if upstream is None else upstream) * scale

    def gradient(variant):
        w, mol, offsets = _weights(fr, variant)
        out = torch.full((rows, x_width + 20), SENTINEL, device=DEV) if padded else None
        return mlp.input_grad(x, upstream=up, out=out, scale=scale,
                              member_weights=None if w is None else torch.tensor(w, device=DEV),
                              molecule_offsets=None if offsets is None else torch.tensor(offsets, dtype=torch.int32, device=DEV)).clone()

    e = mlp.forward(x, with_gradient=True).clone()
    dx = {v: gradient(v) for v in variants}
    assert torch.equal(mlp.forward(x, with_gradient=False), e)                 # the energy-only launch
    assert torch.equal(mlp.forward(x, with_gradient=True), e)                  # and everything once more: the same bits
    for v in variants:
        assert torch.equal(gradient(v), dx[v]), v
    torch.cuda.synchronize()

    C = WITNESS[c.section]
    e = e.cpu().double().numpy()
    assert np.isfinite(e).all()
    atoms = np.concatenate([kd["atoms"].numpy() for kd in fr.kinds])
    no_kind = np.setdiff1d(np.arange(rows), atoms)
    columns = fr.columns.numpy()
    other = np.setdiff1d(np.arange(x_width), columns)
    for v in variants:
        w, mol, _ = _weights(fr, v)
        r = f64.reference(J, None if w is None else (w[0] if mol is None else w), mol)
        got = dx[v].cpu().double().numpy()
        err_e = float(np.abs(e - J.e).max())
        err_g = float(np.abs(got[atoms][:, columns] - factor * r.g_ref[atoms]).max())       # (the other rows: below)
        g_scale, g32 = abs(factor) * r.g_scale, abs(factor) * r.g32
        e32, g32 = max(r.e32, 1e-300), max(g32, 1e-300)
        need_e, need_g = max(err_e - 1e-7 * r.e_scale, 0.0) / e32, max(err_g - 1e-7 * g_scale, 0.0) / g32
        print(f"\n[{c.section}] {name} {v}: energy err {err_e / r.e_scale:.2e} (float32 {r.e32 / r.e_scale:.2e}, ratio {err_e / e32:.2f}, C needed {need_e:.2f})"
              f"  gradient err {err_g / g_scale:.2e} (float32 {g32 / g_scale:.2e}, ratio {err_g / g32:.2f}, C needed {need_g:.2f})", end="")
        assert np.isfinite(got[atoms][:, :x_width]).all()
        assert err_e <= f64.E_BAR * r.e_scale, (err_e, r.e_scale)
        assert err_g <= f64.G_BAR * g_scale, (err_g, g_scale)
        assert err_e <= C * r.e32 + 1e-7 * r.e_scale, ("witness, energies", err_e / e32)
        assert err_g <= C * g32 + 1e-7 * g_scale, ("witness, gradient", err_g / g32)
        raw = dx[v].cpu()
        fill = SENTINEL if padded else 0.0
        assert bool((raw[no_kind] == fill).all())                              # rows of no kind: as they were
        assert bool((raw[:, x_width:] == fill).all())                          # behind the row: as it was
        assert bool((raw[atoms][:, other] == 0).all())                         # column blocks no network reads: zero


# ------------------------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("name", f64.section("a"))
def test_layer0_k_loop_and_input_tail(name):
    _judged(name)


def test_eight_features_in_eight_columns_read_nothing_outside_x():
    """F = 8 on an x of 8 columns: the pieces of layer 0's only K step that lie past F re-read columns 0..7 of their own row (times 0) --
    with NaN right behind the 8 columns (ldx = 20) every output stays finite and judged as in the 8-column x of section a."""
    _judged("a-F8", padded=True)


# ------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("name", f64.section("b"))
def test_hidden_widths(name):
    _judged(name)


# ------------------------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("name", f64.section("c"))
def test_members_and_the_gradient_k_loop(name):
    M = f64.CASES[name].M
    _judged(name, variants=("weighted", "molecules") if M == 128 else ("plain", "weighted", "molecules"))


def test_more_than_128_weighted_members_are_refused():
    from nnpops_amd.capi import NNPOpsHipError
    fr = f64.frame("c-M128-h32")
    mlp = _mlp(fr)
    x = fr.x.to(DEV)
    mlp.forward(x, with_gradient=True)
    out = torch.full((x.shape[0], 64), SENTINEL, device=DEV)
    mlp.frame.num_members = mlp.M = 129                     # (the same object: its planes hold 128; refused before anything reads them)
    with pytest.raises(NNPOpsHipError, match="at most 128 members"):
        mlp.input_grad(x, out=out, member_weights=torch.ones((1, 129), device=DEV))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    mlp.frame.num_members = mlp.M = 128
    mlp.input_grad(x, out=out, member_weights=torch.ones((1, 128), device=DEV))
    assert bool((out != SENTINEL).any())


# ------------------------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("variant", ["plain", "weighted"])
@pytest.mark.parametrize("name", f64.section("d"))
def test_leading_dimensions_sentinels_and_scalars(name, variant):
    """x [80][width + 12] with NaN behind the rows (and in the dead column blocks), dx [80][width + 20] of -7.25, upstream = -0.375 on the
    device times scale = 2.5: mlp_input_grad<false/true> (d-separate) and mlp_sum_members<false/true> (d-live)."""
    _judged(name, variants=(variant,), padded=True, upstream=-0.375, scale=2.5)


# ------------------------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("name", f64.section("e"))
def test_celu_in_saturation(name):
    _judged(name)


# ------------------------------------------------------------------------------------------------------------------ f
def test_eight_kinds_with_empty_ones_first_and_last():
    _judged("f-eight-kinds", variants=("plain", "weighted"))


def test_nine_kinds_are_refused():
    from nnpops_amd.capi import NNPOpsHipError
    fr = f64.frame("f-eight-kinds")
    mlp = _mlp(fr)
    x = fr.x.to(DEV)
    mlp.frame.num_kinds = 9
    with pytest.raises(NNPOpsHipError, match="kinds per launch"):
        mlp.forward(x, with_gradient=False)
    with pytest.raises(NNPOpsHipError, match="kinds per launch"):
        mlp.input_grad(x)
    mlp.frame.num_kinds = 8
    mlp.forward(x, with_gradient=False)


def test_a_frame_without_atoms_launches_nothing():
    fr = f64.frame("f-eight-kinds")
    empty = [dict(kd, atoms=kd["atoms"][:0]) for kd in fr.kinds[:3]]
    mlp = _mlp(fr, kinds=empty)
    assert mlp.energies.numel() == 0
    x = fr.x.to(DEV)
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    energies = torch.full((4, fr.case.M), SENTINEL, device=DEV)
    mlp.frame.rows, mlp.frame.energies = rows.data_ptr(), energies.data_ptr()      # (the C ABI asks for pointers, not for atoms)
    out = torch.full((x.shape[0], fr.case.F), SENTINEL, device=DEV)
    for with_gradient in (True, False):
        mlp.forward(x, with_gradient=with_gradient)
    for w in (None, torch.ones((1, fr.case.M), device=DEV)):
        assert mlp.input_grad(x, out=out, member_weights=w) is out
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((energies == SENTINEL).all())
