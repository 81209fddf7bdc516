"""Second derivatives of the CFConv: nnpops_cfconv_double_backward and the twice-differentiable torch surface above it.

The judge is `SecondOrder` of tests/cfconv_float64.py (pinned by tests/test_cfconv_second_order_reference_cpu.py to the float32 oracle,
to the closed-form expressions and to finite differences): with seeded float32 weights, inputs and cotangents V, Q it gives the gradients
of M = <V, gx> + <Q, gp> with respect to (output gradient, input, positions) over a fixed pair list.  Every comparison first takes
the pair set from the device (nnpops_cfconv_neighbors_export) and asserts that it is the restatement's: both then sum the same
pairs, and no pair sits inside the jump of F'' at the cutoff.  One float64 evaluation per (system, layer), kept for the module.

Figure: max |device - reference| / max |reference| per output.  Every bar below (BAR for the three outputs, SUM_BAR, STEP_BAR,
HESSIAN_BAR) is ten times the worst figure measured on an MI355X, per kernel family where the kernels differ, rounded to one digit
(DESIGN 3.7c holds the measured values):
    matrix (cfconv_second_mfma)     W a multiple of 16 up to 128, weights in LDS
    vector (cfconv_second_vector)   every other shape
Shapes: W 16 G 8 (one column block), W 32 G 16 ssp and tanh, W 48 G 12 (odd block count), W 32 G 70 (more Gaussians than a K tile of
the split kernels), W 128 G 50 (largest LDS footprint), W 24 G 10 (vector), W 130 G 20 tanh (vector, streamed weights); beyond the issue's table, on the small
frame only, the instantiations those do not reach: W 64 (256 registers on eight waves), W 96 (four waves per workgroup), W 100 with
G 12 and G 256 (two channels per lane, weights in LDS and streamed), W 260 (eight channels per lane).  Frames:
triclinic350 (all-pairs build), liquid1500 (cell-ordered walk), dense1100 (rows of 89-120 entries: more than a wave, no multiple of
16), and a 60-atom molecule in vacuum with one atom far away (an empty row: exact zeros).
"""
import numpy as np
import pytest
import torch

from cfconv_float64 import Restatement, SecondOrder, cotangents, frame, handles, layer, sigma_of, weights

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CUTOFF = 5.0
BAR = {"matrix": 8e-5, "vector": 4e-5}
SUM_BAR = {"matrix": 1e-5, "vector": 2e-5}         # |sum_i dM/dpos_i| of the largest entry
STEP_BAR = {"matrix": 7e-6, "vector": 1e-5}        # the force-loss step through two layers
HESSIAN_BAR = 3e-6                                 # |u.Hv - v.Hu| / |u.Hv|

SHAPES = {                     # name: (family, W, G, activation, frames)
    "matrix-one-block": ("matrix", 16, 8, "ssp", ["triclinic350", "dense1100", "molecule"]),
    "matrix-ssp": ("matrix", 32, 16, "ssp", ["triclinic350", "liquid1500", "dense1100", "molecule"]),
    "matrix-tanh": ("matrix", 32, 16, "tanh", ["triclinic350", "liquid1500"]),
    "matrix-odd-blocks": ("matrix", 48, 12, "ssp", ["triclinic350", "liquid1500"]),
    "matrix-many-gaussians": ("matrix", 32, 70, "ssp", ["triclinic350", "liquid1500"]),
    "matrix-config3": ("matrix", 128, 50, "ssp", ["triclinic350", "liquid1500", "dense1100"]),
    "matrix-four-blocks": ("matrix", 64, 16, "tanh", ["triclinic350"]),          # the widest on eight waves per workgroup
    "matrix-six-blocks": ("matrix", 96, 20, "ssp", ["triclinic350"]),            # four waves per workgroup, below the widest
    "vector": ("vector", 24, 10, "ssp", ["triclinic350", "liquid1500", "dense1100", "molecule"]),
    "vector-streamed": ("vector", 130, 20, "tanh", ["triclinic350", "liquid1500"]),
    "vector-two-channels": ("vector", 100, 12, "ssp", ["triclinic350"]),         # two channels per lane, weights in LDS
    "vector-two-channels-streamed": ("vector", 100, 256, "ssp", ["triclinic350"]),      # ... and weights that do not fit
    "vector-eight-channels": ("vector", 260, 8, "tanh", ["triclinic350"]),       # W > 256, streamed
}
CASES = [(name, tag) for name, (_, _, _, _, tags) in SHAPES.items() for tag in tags]

_REFERENCES = {}


def _layer(tag, W, G):
    """-> (w1, b1, w2, b2, x, gout, V, Q) of a layer on a frame, seeded by the shape"""
    return layer(tag, W, G) + cotangents(len(frame(tag)[0]), W, 2000 * W + G)


def _second_order(tag, W, G, act):
    pos, box = frame(tag)
    w1, b1, w2, b2 = _layer(tag, W, G)[:4]
    judge = Restatement(W, G, CUTOFF, sigma_of(G), act, w1, b1, w2, b2)
    return SecondOrder.open(judge, pos) if box is None else SecondOrder.periodic(judge, pos, box)


def _reference(tag, W, G, act):
    """float64: (SecondOrder, its dict for both cotangents), once per (system, layer)"""
    key = (tag, W, G, act)
    if key not in _REFERENCES:
        so = _second_order(tag, W, G, act)
        _, _, _, _, x, gy, V, Q = _layer(tag, W, G)
        _REFERENCES[key] = (so, so.second(frame(tag)[0], x, gy, V, Q))
    return _REFERENCES[key]


def _dev(*arrays):
    return [None if a is None else torch.tensor(a, device=DEV) for a in arrays]


def _built(tag, W, G, act, so):
    """handles with the list built on the frame; asserts that the device's pair set is the restatement's"""
    nb, cf = handles(tag, W, G, act, CUTOFF)
    tpos, tbox = _dev(*frame(tag))
    nb.build(tpos, tbox)
    atoms, _ = nb.export()
    assert np.array_equal(atoms[0], so.i.numpy()) and np.array_equal(atoms[1], so.j.numpy()), \
        f"{tag}: the device's pair set differs from the restatement's ({atoms.shape[1]} against {len(so.i)} pairs)"
    return nb, cf, tpos, tbox


def _errors(got, ref):
    out = {}
    for name, t in zip(("dg", "dx", "dp"), got):
        top = float(np.abs(ref[name]).max())
        assert top > 0
        out[name] = float(np.abs(t.cpu().numpy().astype(np.float64) - ref[name]).max()) / top
    return out


# ---------------------------------------------------------------------------------------------- every kernel, through the C entry
@pytest.mark.parametrize("shape,tag", CASES, ids=[f"{s}-{t}" for s, t in CASES])
def test_double_backward_against_float64(shape, tag):
    family, W, G, act, _ = SHAPES[shape]
    so, ref = _reference(tag, W, G, act)
    nb, cf, tpos, tbox = _built(tag, W, G, act, so)
    if tag in ("liquid1500", "dense1100"):
        assert nb.read_grid()["ok"], nb.read_grid()            # the cell grid built these rows
    counts = np.bincount(np.concatenate([so.i.numpy(), so.j.numpy()]), minlength=len(tpos))
    if tag == "dense1100":
        assert counts.min() > 64 and (counts % 16 != 0).any(), (counts.min(), counts.max())
    x, gy, V, Q = _dev(*_layer(tag, W, G)[4:])
    first = [t.clone() for t in cf.double_backward(nb, tpos, x, gy, V, Q)]
    again = cf.double_backward(nb, tpos, x, gy, V, Q)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b), "two calls give different bits"
    err = _errors(first, ref)
    print(f"\n[cfconv-second] {shape} W={W} G={G} {act} {tag} ({family}): dM/dg {err['dg']:.2e}  dM/dx {err['dx']:.2e}  dM/dpos {err['dp']:.2e} "
          f"of max; rows {counts.min()}..{counts.max()}, margin to the cutoff {so.margin(frame(tag)[0]):.1e}")
    for t in first:
        assert bool(torch.isfinite(t).all())
    if tag == "molecule":
        assert counts[-1] == 0
        for t in first:
            assert torch.equal(t[-1], torch.zeros_like(t[-1])), "the isolated atom's outputs are not exact zeros"
    # the pair terms of dM/dpos are antisymmetric, each end evaluating its own in float32: the rows sum to rounding of the largest
    total = first[2].double().sum(dim=0).abs().max().item()
    top = float(np.abs(ref["dp"]).max())
    print(f"[cfconv-second] {shape} {tag}: |sum_i dM/dpos_i| {total / top:.2e} of the largest entry")
    assert total <= SUM_BAR[family] * top
    for name in ("dg", "dx", "dp"):
        assert err[name] <= BAR[family], (shape, tag, name, err[name])


# ---------------------------------------------------------------------------------------------- exact and structural cases
@pytest.mark.parametrize("shape", ["matrix-one-block", "vector"])
def test_two_atoms_one_pair(shape):
    from nnpops_amd.capi import CFConv, CFConvNeighbors
    family, W, G, act, _ = SHAPES[shape]
    pos = np.array([[0.4, 5.0, 5.1], [2.1, 5.9, 4.2]], dtype=np.float32)
    w1, b1, w2, b2, x, gy = weights(W, G, 2, 7)
    V, Q = cotangents(2, W, 8)
    so = SecondOrder.open(Restatement(W, G, 3.0, 0.4, act, w1, b1, w2, b2), pos)
    assert len(so.i) == 1
    ref = so.second(pos, x, gy, V, Q)
    nb, cf = CFConvNeighbors(2, 3.0, False), CFConv(2, W, G, 3.0, 0.4, act, w1, b1, w2, b2)
    tpos, tx, tg, tV, tQ = _dev(pos, x, gy, V, Q)
    nb.build(tpos)
    got = cf.double_backward(nb, tpos, tx, tg, tV, tQ)
    err = _errors(got, ref)
    print(f"\n[cfconv-second] two atoms {shape}: dM/dg {err['dg']:.2e}  dM/dx {err['dx']:.2e}  dM/dpos {err['dp']:.2e}")
    assert max(err.values()) <= BAR[family]
    assert torch.equal(got[2][0], -got[2][1]) or float((got[2][0] + got[2][1]).abs().max()) <= BAR[family] * float(got[2].abs().max())


@pytest.mark.parametrize("shape", ["matrix-ssp", "vector"])
def test_rigid_translation_gives_exact_zeros(shape):
    """V = 0 and every Q_i the same vector: a = u.(Q_j - Q_i) = 0 and A = 0 in every pair"""
    family, W, G, act, _ = SHAPES[shape]
    tag = "triclinic350"
    so, _ = _reference(tag, W, G, act)
    nb, cf, tpos, tbox = _built(tag, W, G, act, so)
    x, gy = _dev(*_layer(tag, W, G)[4:6])
    V = torch.zeros_like(x)
    Q = torch.tensor([0.3, -1.7, 0.9], device=DEV).repeat(len(tpos), 1).contiguous()
    for t in cf.double_backward(nb, tpos, x, gy, V, Q):
        assert torch.equal(t, torch.zeros_like(t))
    for t in cf.double_backward(nb, tpos, x, gy, None, Q):
        assert torch.equal(t, torch.zeros_like(t))


@pytest.mark.parametrize("shape", ["matrix-ssp", "matrix-config3", "vector"])
def test_input_cotangent_alone_is_the_forward_and_the_backward_of_it(shape):
    """Q = NULL: dM/dx = 0 exactly, dM/dg = compute(input = V), dM/dpos = the position gradient of backprop(input = V)"""
    family, W, G, act, _ = SHAPES[shape]
    tag = "triclinic350"
    so, _ = _reference(tag, W, G, act)
    nb, cf, tpos, tbox = _built(tag, W, G, act, so)
    x, gy, V, _ = _dev(*_layer(tag, W, G)[4:])
    dg, dx, dp = cf.double_backward(nb, tpos, x, gy, V, None)
    assert torch.equal(dx, torch.zeros_like(dx))
    fwd = cf.compute(nb, tpos, V, tbox)
    _, gp = cf.backprop(nb, tpos, V, gy, tbox)
    e_g = float((dg - fwd).abs().max() / fwd.abs().max())
    e_p = float((dp - gp).abs().max() / gp.abs().max())
    print(f"\n[cfconv-second] {shape}: V alone: dM/dg vs compute(V) {e_g:.2e}, dM/dpos vs backprop(V) {e_p:.2e}")
    assert e_g <= BAR[family] and e_p <= BAR[family]


@pytest.mark.parametrize("shape", ["matrix-ssp", "matrix-config3", "vector"])
def test_forward_and_backward_keep_their_bits(shape):
    """compute() and backprop() around a double-backward call return what they return without it (the backward reads the forward
    call's filter rows back: the new kernel must leave them and their bookkeeping alone)"""
    family, W, G, act, _ = SHAPES[shape]
    tag = "liquid1500"
    so, _ = _reference(tag, W, G, act)
    x, gy, V, Q = _dev(*_layer(tag, W, G)[4:])

    def run(between):
        nb, cf, tpos, tbox = _built(tag, W, G, act, so)
        out = cf.compute(nb, tpos, x, tbox).clone()
        if between:
            cf.double_backward(nb, tpos, x, gy, V, Q)
        gx, gp = [t.clone() for t in cf.backprop(nb, tpos, x, gy, tbox)]
        if between:
            cf.double_backward(nb, tpos, x, gy, V, Q)
        out2 = cf.compute(nb, tpos, x, tbox).clone()
        gx2, gp2 = [t.clone() for t in cf.backprop(nb, tpos, x, gy, tbox)]
        torch.cuda.synchronize()
        return out, gx, gp, out2, gx2, gp2

    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


def test_refused_without_a_cotangent_or_a_list():
    from nnpops_amd.capi import NNPOpsHipError
    _, W, G, act, _ = SHAPES["matrix-ssp"]
    tag = "triclinic350"
    nb, cf = handles(tag, W, G, act, CUTOFF)
    tpos, tbox = _dev(*frame(tag))
    x, gy, V, Q = _dev(*_layer(tag, W, G)[4:])
    with pytest.raises(NNPOpsHipError, match="not been built"):
        cf.double_backward(nb, tpos, x, gy, V, Q)
    nb.build(tpos, tbox)
    with pytest.raises(NNPOpsHipError, match="both NULL"):
        cf.double_backward(nb, tpos, x, gy, None, None)
    assert all(bool(torch.isfinite(t).all()) for t in cf.double_backward(nb, tpos, x, gy, V, Q))      # the handles are still good


# ---------------------------------------------------------------------------------------------- the torch surface
def _model(tag, W, G, act, twice, seed=0):
    """a trainable linear layer in front of two stacked convolutions on one list (scriptable)"""
    from typing import Optional
    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    la, lb = weights(W, G, 1, 31 + seed)[:4], weights(W, G, 1, 32 + seed)[:4]
    as_module = lambda w1, b1, w2, b2: CFConv(sigma_of(G), act, torch.tensor(w1).reshape(G, W), torch.tensor(b1), torch.tensor(w2),
                                              torch.tensor(b2), twice_differentiable=twice)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.neighbors = CFConvNeighbors(CUTOFF)
            self.linear = torch.nn.Linear(W, W, bias=False)
            self.conv1 = as_module(*la)
            self.conv2 = as_module(*lb)

        def forward(self, positions: torch.Tensor, x: torch.Tensor, box: Optional[torch.Tensor]) -> torch.Tensor:
            self.neighbors.build(positions, box)
            h = self.conv1(self.neighbors, positions, self.linear(x), box)
            return self.conv2(self.neighbors, positions, 0.1 * h, box)

    torch.manual_seed(5)
    return Model().to(DEV), (la, lb)


def _force_loss_step(model, pos, x, box, readout, f_ref):
    """E -> F = dE/dpos (create_graph) -> |F - F_ref|^2 -> its gradients with respect to (linear weight, positions, input)"""
    energy = (model(pos, x, box) * readout).sum()
    force, = torch.autograd.grad(energy, pos, create_graph=True)
    loss = ((force - f_ref) ** 2).sum()
    return torch.autograd.grad(loss, [model.linear.weight, pos, x]), force.detach(), energy.detach()


def _step_inputs(tag, W, G):
    pos, box = frame(tag)
    _, _, _, _, x, gy, _, Q = _layer(tag, W, G)
    return pos, box, x, (0.1 * gy).astype(np.float32), (0.1 * Q).astype(np.float32)


@pytest.mark.parametrize("tag", ["triclinic350", "molecule"])
def test_twice_ops_give_the_bits_of_the_plain_ops(tag):
    _, W, G, act, _ = SHAPES["matrix-ssp"]
    pos, box, x, readout, _ = _step_inputs(tag, W, G)

    def run(twice):
        model, _ = _model(tag, W, G, act, twice)
        tpos, tx = (t.requires_grad_(True) for t in _dev(pos, x))
        tbox, tr = _dev(box, readout)
        out = model(tpos, tx, tbox)
        (out * tr).sum().backward()
        return out.detach(), tx.grad, tpos.grad, model.linear.weight.grad

    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", ["matrix-ssp", "vector"])
def test_force_loss_step_against_float64(shape):
    """Two stacked twice-differentiable convolutions behind a trainable linear layer: the gradient of a force loss with respect to the
    layer's weight and to the positions, against the restatement's autograd, each as max |device - reference| / max |reference| (STEP_BAR)."""
    family, W, G, act, _ = SHAPES[shape]
    tag = "triclinic350"
    pos, box, x, readout, f_ref = _step_inputs(tag, W, G)
    model, (la, lb) = _model(tag, W, G, act, True)
    tpos, tx = (t.requires_grad_(True) for t in _dev(pos, x))
    tbox, tr, tf = _dev(box, readout, f_ref)
    (gw, gp, gx), force, _ = _force_loss_step(model, tpos, tx, tbox, tr, tf)
    scripted = torch.jit.script(_model(tag, W, G, act, True)[0])
    (sw, sp, sx), _, _ = _force_loss_step(scripted, tpos, tx, tbox, tr, tf)
    assert torch.equal(sw, gw) and torch.equal(sp, gp) and torch.equal(sx, gx), "the scripted module gives other numbers"
    # float64
    so1 = SecondOrder.periodic(Restatement(W, G, CUTOFF, sigma_of(G), act, *la), pos, box)
    so2 = SecondOrder(Restatement(W, G, CUTOFF, sigma_of(G), act, *lb), so1.i, so1.j, so1.shift)
    wide = lambda a: torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))
    w = wide(model.linear.weight.detach().cpu().numpy()).requires_grad_(True)
    p, xin = wide(pos).requires_grad_(True), wide(x).requires_grad_(True)
    energy = (so2.forward(p, 0.1 * so1.forward(p, xin @ w.T)) * wide(readout)).sum()
    f64, = torch.autograd.grad(energy, p, create_graph=True)
    rw, rp, rx = torch.autograd.grad(((f64 - wide(f_ref)) ** 2).sum(), [w, p, xin])
    rel = lambda got, ref: float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    e_f, e_w, e_p, e_x = rel(force, f64.detach()), rel(gw, rw), rel(gp, rp), rel(gx, rx)
    print(f"\n[cfconv-second] force-loss step {shape}: force {e_f:.2e}, d/dweight {e_w:.2e}, d/dpositions {e_p:.2e}, d/dinput {e_x:.2e} of max")
    assert float(rw.abs().max()) > 0 and float(rp.abs().max()) > 0
    assert max(e_w, e_p, e_x) <= STEP_BAR[family]


def test_default_module_does_not_train_on_forces():
    """What the default CFConv does under create_graph=True on this commit: its backward returns plain tensors, so the force carries no
    graph and a loss made of it alone cannot be differentiated; next to another differentiable term the convolution's share of the
    gradient is dropped without a word.  twice_differentiable=True is the remedy (the test above)."""
    _, W, G, act, _ = SHAPES["matrix-ssp"]
    tag = "triclinic350"
    pos, box, x, readout, f_ref = _step_inputs(tag, W, G)
    model, _ = _model(tag, W, G, act, False)
    tpos, tx = (t.requires_grad_(True) for t in _dev(pos, x))
    tbox, tr, tf = _dev(box, readout, f_ref)
    energy = (model(tpos, tx, tbox) * tr).sum()
    force, = torch.autograd.grad(energy, tpos, create_graph=True)
    assert not force.requires_grad and force.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        ((force - tf) ** 2).sum().backward()
    # with a differentiable term beside it: runs, and the weight gets nothing from the force
    energy = (model(tpos, tx, tbox) * tr).sum() + (tpos ** 2).sum()
    force, = torch.autograd.grad(energy, tpos, create_graph=True)
    ((force - tf) ** 2).sum().backward()
    assert model.linear.weight.grad is None or not bool(model.linear.weight.grad.abs().max() > 0)


def test_hessian_vector_products_are_symmetric():
    """u^T (H v) = v^T (H u) for the Hessian of E in the positions, to HESSIAN_BAR of the value"""
    family, W, G, act, _ = SHAPES["matrix-ssp"]
    tag = "triclinic350"
    pos, box, x, readout, _ = _step_inputs(tag, W, G)
    model, _ = _model(tag, W, G, act, True)
    tpos = _dev(pos)[0].requires_grad_(True)
    tx, tbox, tr = _dev(x, box, readout)
    rng = np.random.default_rng(9)
    u, v = _dev(rng.standard_normal(pos.shape).astype(np.float32), rng.standard_normal(pos.shape).astype(np.float32))
    energy = (model(tpos, tx, tbox) * tr).sum()
    force, = torch.autograd.grad(energy, tpos, create_graph=True)
    hv, = torch.autograd.grad((force * v).sum(), tpos, retain_graph=True)
    hu, = torch.autograd.grad((force * u).sum(), tpos, retain_graph=True)
    a, b = float((u.double() * hv.double()).sum()), float((v.double() * hu.double()).sum())
    print(f"\n[cfconv-second] u.Hv {a:.6e}  v.Hu {b:.6e}  difference {abs(a - b) / abs(a):.2e} of the value")
    assert float(hv.abs().max()) > 0 and abs(a) > 1.0 and abs(a - b) <= HESSIAN_BAR * abs(a)
    # a third derivative raises
    hv2, = torch.autograd.grad((force * v).sum(), tpos, create_graph=True)
    with pytest.raises(RuntimeError, match="third derivatives are not implemented"):
        torch.autograd.grad(hv2.sum(), tpos)


def test_torch_refusals():
    _, W, G, act, _ = SHAPES["matrix-ssp"]
    tag = "triclinic350"
    pos, box, x, readout, _ = _step_inputs(tag, W, G)
    model, _ = _model(tag, W, G, act, True)
    tpos = _dev(pos)[0].requires_grad_(True)
    tx, tbox, tr = _dev(x, box, readout)
    with pytest.raises(RuntimeError, match="operation_periodic"):
        model(tpos, tx, tbox.clone().requires_grad_(True))             # a box that requires a gradient
    # a list rebuilt between the forward pass and a derivative
    energy = (model(tpos, tx, tbox) * tr).sum()
    model.neighbors.build(tpos.detach() + 0.01, tbox)
    with pytest.raises(RuntimeError, match="rebuilt"):
        torch.autograd.grad(energy, tpos)
    energy = (model(tpos, tx, tbox) * tr).sum()
    force, = torch.autograd.grad(energy, tpos, create_graph=True)
    model.neighbors.build(tpos.detach() + 0.01, tbox)
    with pytest.raises(RuntimeError, match="rebuilt"):
        (force ** 2).sum().backward()
    energy = (model(tpos, tx, tbox) * tr).sum()                         # ... and the module is still good
    assert bool(torch.isfinite(torch.autograd.grad(energy, tpos)[0]).all())


def test_force_loss_step_replays_in_a_captured_graph():
    """Build + energy + force + force loss + its gradients captured once (after warm-up steps) and replayed after positions and input
    were written in place gives the eager result, bit for bit."""
    _, W, G, act, _ = SHAPES["matrix-ssp"]
    tag = "liquid1500"
    pos, box, x, readout, f_ref = _step_inputs(tag, W, G)
    model, _ = _model(tag, W, G, act, True)
    static_pos, static_x = (t.requires_grad_(True) for t in _dev(pos, x))
    tbox, tr, tf = _dev(box, readout, f_ref)

    def step(p, xin):
        return _force_loss_step(model, p, xin, tbox, tr, tf)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                              # calibrates neighbour capacities, sizes the filter rows
            step(static_pos, static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_w, g_pos, g_x = step(static_pos, static_x)
    rng = np.random.default_rng(1)
    for _ in range(2):
        new_pos = (pos + rng.normal(0, 0.05, pos.shape)).astype(np.float32)
        new_x = (x + rng.normal(0, 0.1, x.shape)).astype(np.float32)
        with torch.no_grad():
            static_pos.copy_(torch.tensor(new_pos, device=DEV))
            static_x.copy_(torch.tensor(new_x, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        e_w, e_pos, e_x = step(static_pos.detach().clone().requires_grad_(True), static_x.detach().clone().requires_grad_(True))
        assert torch.equal(g_w, e_w) and torch.equal(g_pos, e_pos) and torch.equal(g_x, e_x)
        assert float(e_w.abs().max()) > 0 and float(e_pos.abs().max()) > 0
