"""Pins the float64 judge of the AEV tangent (tests/ani_tangent_float64.py) without a GPU, and checks the surface the feature adds.

The judge J.v -- two reverse passes of autograd over ani_float64.Restatement -- is held against
  * central differences (aev(x + h v) - aev(x - h v)) / 2h of the restatement's own forward, h = 1e-5: their truncation error is
    h^2/6 |d3 aev| ~ 1e-10 |J.v| x (the cube of the largest logarithmic derivative, ~30 / A), their rounding error 1e-16 / h: 1e-6 of
    the largest entry is a bar both sides meet with two decades to spare;
  * the adjoint identity <w, J.v> = <J^T w, v> against Restatement.evaluate(...)['g'], the judge of the forces: two independent
    routes through autograd, 1e-10 of the sum of the absolute terms;
  * the closed form of the per-pair and per-triple tangents, 1e-10 of the largest entry of each block.
The float32 witness (the kernel's formulas on float32 displacements, on the CPU) has to sit inside HALF the bar of the GPU test,
5e-5 of the largest entry of each block, on every case: the bar is one float32 arithmetic can meet.
"""
import ctypes
import os

import numpy as np
import pytest

import ani_tangent_float64 as T
from ani_float64 import Restatement, weights

CASES = [("conformer60", "ani2x", True), ("conformer60", "ani2x", False), ("triclinic60", "ani2x", True), ("cubic100", "ani2x", False),
         ("cubic100", "two_eta_two_zeta", True), ("conformer60", "no_grid", True), ("two_atoms", "ani2x", True), ("lone_angular", "ani2x", True),
         ("one_atom", "ani2x", True)]
IDS = [f"{t}-{f}-{'torchani' if ta else 'paper'}" for t, f, ta in CASES]

_JUDGED = {}


def _judged(tag, fset, torchani):
    key = (tag, fset, torchani)
    if key not in _JUDGED:
        rest = T.restatement(tag, fset, torchani)
        _, _, _, species, pos, box = T.frame(tag)
        v = T.tangent_field(len(species), 5)
        _JUDGED[key] = (rest, pos, box, v, T.judge(rest, pos, box, v))
    return _JUDGED[key]


@pytest.mark.parametrize("tag,fset,torchani", CASES, ids=IDS)
def test_judge_against_central_differences(tag, fset, torchani):
    rest, pos, box, v, (jr, ja) = _judged(tag, fset, torchani)
    b = T.VACUUM if box is None else box
    h = 1e-5
    x = np.asarray(pos, dtype=np.float32).astype(np.float64)

    class Wide(Restatement):                     # the restatement at float64 positions (evaluate() rounds its input to float32)
        def evaluate64(self, p):
            import torch
            box64 = np.asarray(b, dtype=np.float32).astype(np.float64).reshape(3, 3)
            pairs, triples = self.lists(x, box64)             # the lists of the unmoved frame, held fixed
            tx, tB = torch.tensor(p), torch.tensor(box64)
            r = torch.zeros(self.N * self.S, self.nR, dtype=torch.float64)
            a = torch.zeros(self.N * self.NB, self.nA, dtype=torch.float64)
            terms, rows = self._radial_terms(tx, tB, pairs)
            r.index_add_(0, rows, terms)
            if len(triples[0]):
                terms, rows = self._angular_terms(tx, tB, triples)
                a.index_add_(0, rows, terms)
            return r.reshape(self.N, -1).numpy(), a.reshape(self.N, -1).numpy()

    wide = Wide(rest.S, rest.rcr, rest.rca, rest.species, rest.rf.numpy(), rest.af.numpy(), rest.torchani)
    v64 = np.asarray(v, dtype=np.float64)
    rp, ap = wide.evaluate64(x + h * v64)
    rm, am = wide.evaluate64(x - h * v64)
    er, ea = T.block_errors(((rp - rm) / (2 * h), (ap - am) / (2 * h)), (jr, ja))
    print(f"[ani-tangent-ref] {tag} {fset} torchani={torchani}: judge vs central differences radial {er:.2e} angular {ea:.2e}")
    assert er <= 1e-6 and ea <= 1e-6, (er, ea)


@pytest.mark.parametrize("tag,fset,torchani", CASES, ids=IDS)
def test_judge_is_the_adjoint_of_the_force_judge(tag, fset, torchani):
    rest, pos, box, v, (jr, ja) = _judged(tag, fset, torchani)
    wr, wa = weights(jr.shape, ja.shape, seed=11)
    g = rest.evaluate(pos, T.VACUUM if box is None else box, wr, wa)["g"]
    left = float((wr.astype(np.float64) * jr).sum() + (wa.astype(np.float64) * ja).sum())
    right = float((g * np.asarray(v, dtype=np.float64)).sum())
    size = float(np.abs(wr * jr).sum() + np.abs(wa * ja).sum() + np.abs(g * v).sum())
    print(f"[ani-tangent-ref] {tag} {fset} torchani={torchani}: <w, J v> = {left:.12e}, <J^T w, v> = {right:.12e}")
    assert abs(left - right) <= 1e-10 * max(size, 1e-300), (left, right, size)


@pytest.mark.parametrize("tag,fset,torchani", CASES, ids=IDS)
def test_closed_form_and_witness(tag, fset, torchani):
    rest, pos, box, v, ref = _judged(tag, fset, torchani)
    er, ea = T.block_errors(T.closed_form(rest, pos, box, v), ref)
    wr, wa = T.block_errors(T.witness(rest, pos, box, v), ref)
    print(f"[ani-tangent-ref] {tag} {fset} torchani={torchani}: closed form radial {er:.2e} angular {ea:.2e}; "
          f"float32 witness radial {wr:.2e} angular {wa:.2e} (half the bar: {0.5 * T.BAR:.0e})")
    assert er <= 1e-10 and ea <= 1e-10, (er, ea)
    assert wr <= 0.5 * T.BAR and wa <= 0.5 * T.BAR, (wr, wa)


def test_zero_field_and_translation_have_no_tangent():
    rest, pos, box, _, _ = _judged("triclinic60", "ani2x", True)
    zr, za = T.judge(rest, pos, box, np.zeros_like(pos))
    assert not zr.any() and not za.any()
    tr, ta = T.judge(rest, pos, box, np.tile(np.float32([0.3, -1.1, 0.7]), (len(pos), 1)))
    assert np.abs(tr).max() <= 1e-12 and np.abs(ta).max() <= 1e-12


# ---------------------------------------------------------------------------------------------- the surface
def test_symbol_is_exported_and_declared():
    from nnpops_amd import build, capi
    assert "nnpops_ani_tangent_strided" in capi.SIGNATURES
    assert os.path.exists(build.LIB), "the library is built by build()"
    assert hasattr(ctypes.CDLL(build.LIB), "nnpops_ani_tangent_strided")
    assert callable(getattr(capi.AniSymmetryFunctions, "tangent"))
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "nnpops_hip.h")).read()
    assert "int nnpops_ani_tangent_strided(nnpops_ani_t h, const float* position_tangent" in header


def test_holder_schema():
    import torch
    from nnpops_amd import torch_binding
    torch_binding.load()
    cls = "__torch__.torch.classes.NNPOpsANISymmetryFunctions.Holder"
    holder = torch.classes.NNPOpsANISymmetryFunctions.Holder(1, 5.0, 3.0, [1.0], [1.0], [1.0], [1.0], [1.0], [1.0], [0])
    assert str(holder._get_method("tangent").schema) == f"tangent({cls} _0, Tensor _1) -> Tensor _0"
    assert str(holder._get_method("tangent_split").schema) == f"tangent_split({cls} _0, Tensor _1) -> Tensor[] _0"
    assert str(holder._get_method("build_count").schema) == f"build_count({cls} _0) -> int _0"
    assert holder.build_count() == 0
    with pytest.raises(RuntimeError, match="before forward"):
        holder.tangent(torch.zeros(1, 3))
