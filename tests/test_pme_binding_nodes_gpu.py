"""The autograd nodes of the PME torch binding (the PME section of nnpops_amd/csrc/torch_binding.cpp): every node differentiates the
tensors of its own forward pass, whatever the same PME object, the same frames table and the other ops have been called with since.
All 13 ops share one state struct (PmeState: save and load) and the five _twice ops one recorded chain; a piece saved or loaded in
the wrong place, or a chain serving the wrong term, shows here and nowhere else: no other PME test takes a backward after another
forward pass of the same op, or interleaves the flavours on one object.

The kernels are not under test (the float64 files judge them), so the shapes are the smallest at which two pieces of equal shape
still differ in value: 3 frames of 5, 9 and 7 atoms in triclinic boxes with bonded-like exclusions in every frame, 24 atoms for the
single system, grid 6 x 8 x 10 (three moduli of different lengths, a grid transform="lds" serves) with order 5, cutoff 1.0 below
half the narrowest box width, charges that differ, and every gradient the op gives (positions, charges, and the box where it has one).

BAR: torch.equal.  A gradient taken after other passes is the result of the same kernels on the same inputs as the gradient of that
call made alone on a fresh PME object, and the kernels are deterministic (the "bit for bit" tests of the neighbouring files).
14 tests, 7 s on an MI355X when they are the process's first launches (2.5 s of it in the first reciprocal case).
"""
import functools

import numpy as np
import pytest
import torch

import pme_float64 as f64
import pme_frames_float64 as frames64
from pme_frames_float64 import ALPHA, COULOMB, CUTOFF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID, ORDER = (6, 8, 10), 5
SIZES, ATOMS = (5, 9, 7), 24

# op -> (the method's term, frames or single system, the options that select the op, whether the box takes a gradient)
OPS = {
    "pme_direct": ("direct", False, {}, False),
    "pme_direct_box": ("direct", False, {}, True),
    "pme_direct_twice": ("direct", False, dict(twice_differentiable=True), False),
    "pme_reciprocal": ("reciprocal", False, {}, True),
    "pme_reciprocal_twice": ("reciprocal", False, dict(twice_differentiable=True), False),
    "pme_direct_frames": ("direct", True, {}, False),
    "pme_direct_frames_box": ("direct", True, dict(box_gradient=True), True),
    "pme_direct_frames_twice": ("direct", True, dict(twice_differentiable=True), False),
    "pme_reciprocal_frames": ("reciprocal", True, {}, False),
    "pme_reciprocal_frames_box": ("reciprocal", True, dict(box_gradient=True), True),
    "pme_reciprocal_frames_lds": ("reciprocal", True, dict(transform="lds"), False),
    "pme_reciprocal_frames_lds_box": ("reciprocal", True, dict(transform="lds", box_gradient=True), True),
    "pme_reciprocal_frames_twice": ("reciprocal", True, dict(twice_differentiable=True), False),
}
TWICE = [op for op in OPS if op.endswith("_twice")]


@functools.lru_cache(maxsize=None)
def _inputs(frames, which):
    """inputs "A" or "B" (other positions, charges and boxes of the same shapes) -> positions, charges, box(es), offsets, exclusions"""
    seed, scale = (300, 1.0) if which == "A" else (400, 1.125)
    if frames:
        pos, q, boxes, offsets, _ = frames64.batch(SIZES, seed, scales=(scale,))
        excl = frames64.batch(SIZES, 300)[4]                  # (A's: the exclusions are the object's)
        assert all((excl[a:b] >= 0).any() for a, b in zip(offsets, offsets[1:])), "every frame has an exclusion pair"
        return pos, q, boxes, offsets, excl
    pos, q, box = f64.system(True, n=ATOMS, seed=seed)
    return pos * np.float32(scale), q, box * np.float32(scale), None, f64.exclusion_table(ATOMS, seed=4).numpy()


def _pme(frames, options):
    from NNPOps.pme import PME
    excl = torch.tensor(_inputs(frames, "A")[4])              # (A and B share the exclusions: one object serves both)
    twice = bool(options.get("twice_differentiable")) and not frames        # (the frames methods take it per call)
    return PME(*GRID, ORDER, ALPHA, COULOMB, excl, reciprocal=True, twice_differentiable=twice)


class Call:
    """one forward pass of `op` on leaves of its own; the energies of frames are weighted, every frame differently, into one number"""

    def __init__(self, pme, op, which):
        term, frames, options, box_grad = OPS[op]
        pos, q, box, offsets, _ = _inputs(frames, which)
        self.pos, self.q = (torch.tensor(a, device=DEV, requires_grad=True) for a in (pos, q))
        self.box = torch.tensor(box, device=DEV, requires_grad=box_grad)
        self.leaves = (self.pos, self.q) + ((self.box,) if box_grad else ())
        assert len(set(q.tolist())) > 1
        if frames and term == "direct":
            e = pme.compute_direct_frames(self.pos, self.q, CUTOFF, self.box, offsets, **options)
        elif frames:
            e = pme.compute_reciprocal_frames(self.pos, self.q, self.box, offsets, **options)
        elif term == "direct":
            e = pme.compute_direct(self.pos, self.q, CUTOFF, self.box)
        else:
            e = pme.compute_reciprocal(self.pos, self.q, self.box)
        self.energy = (e * torch.tensor([1.0, -0.5, 2.0], device=DEV)).sum() if frames else e

    def gradients(self):
        return torch.autograd.grad(self.energy, self.leaves)

    def forces(self):
        """the first backward, recorded"""
        self.fx, self.fq = torch.autograd.grad(self.energy, (self.pos, self.q), create_graph=True)

    def force_loss_gradients(self):
        rng = np.random.default_rng(7)
        cx, cq = (torch.tensor(rng.standard_normal(tuple(t.shape)).astype(np.float32), device=DEV) for t in (self.fx, self.fq))
        return torch.autograd.grad((self.fx * cx).sum() + (self.fq * cq).sum(), (self.pos, self.q))


def _same(got, alone):
    assert len(got) == len(alone)
    for g, a in zip(got, alone):
        assert torch.isfinite(a).all() and bool((a != 0).any())
        assert torch.equal(g, a)


@pytest.mark.parametrize("op", list(OPS))
def test_first_backward_after_a_second_forward(op):
    _, frames, options, _ = OPS[op]
    pme = _pme(frames, options)
    a = Call(pme, op, "A")
    Call(pme, op, "B")
    _same(a.gradients(), Call(_pme(frames, options), op, "A").gradients())
    if op not in TWICE:
        return
    # one order up: the gradient of a force loss on A after B's forward and first backward
    a = Call(pme, op, "A")
    b = Call(pme, op, "B")
    b.forces()
    a.forces()
    b.force_loss_gradients()
    alone = Call(_pme(frames, options), op, "A")
    alone.forces()
    _same((a.fx, a.fq) + a.force_loss_gradients(), (alone.fx, alone.fq) + alone.force_loss_gradients())


def test_recorded_and_default_ops_interleaved():
    """one PME object and one offsets list, so one frames table: the four flavours of compute_reciprocal_frames forward, then
    backward in reverse order"""
    flavours = ["pme_reciprocal_frames", "pme_reciprocal_frames_box", "pme_reciprocal_frames_lds", "pme_reciprocal_frames_twice"]
    pme = _pme(True, {})
    calls = [Call(pme, op, which) for op, which in zip(flavours, "ABAB")]
    got = {}
    for op, call in reversed(list(zip(flavours, calls))):
        if op.endswith("_twice"):
            call.forces()
            got[op] = (call.fx, call.fq) + call.force_loss_gradients()
        else:
            got[op] = call.gradients()
    for op, which in zip(flavours, "ABAB"):
        alone = Call(_pme(True, {}), op, which)
        if op.endswith("_twice"):
            alone.forces()
            _same(got[op], (alone.fx, alone.fq) + alone.force_loss_gradients())
        else:
            _same(got[op], alone.gradients())
