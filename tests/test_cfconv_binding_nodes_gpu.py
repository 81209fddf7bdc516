"""The autograd nodes of the CFConv torch binding (namespace NNPOps::CFConv of nnpops_amd/csrc/torch_binding.cpp): every node differentiates
the tensors of its own forward pass, whatever the same CFConv has been called with since.

The kernels are not under test here (the float64 files judge them), so the shapes are the smallest the neighbouring files use: W = 16,
G = 8 on conformer90 (90 atoms, open, cutoff 5.0) and on triclinic80 (80 atoms, periodic, cutoff 4.0: below half its narrowest width).

BAR: torch.equal.  A gradient taken after another forward pass of the same module is the result of the same kernels on the same
inputs as the gradient of that call made alone on a fresh module, and two such calls agree bit for bit
(test_cfconv_weights_gpu.py::test_weight_gradients_against_float64 asserts it for the weight gradients, the "bit for bit" tests of the
neighbouring files for the others).  Parameter gradients accumulated over two backward passes are compared with the float32 sum of the
two single-call gradients, formed in the same order: the same add of the same two tensors.

Before the nodes kept their own tensors the default and the trainable flavours failed test_first_backward_after_a_second_forward: their
backward read what the holder had last been called with.  10 tests, 4 s on an MI355X.
"""
import pytest
import torch

import cfconv_dispatch_float64 as dispatch
import cfconv_float64
from box_gradient_judge import clean_env
from cfconv_float64 import sigma_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, G, ACT = 16, 8, "ssp"
PARAMS = ("weights1", "biases1", "weights2", "biases2")
FLAVOURS = {"default": {}, "twice_differentiable": dict(twice_differentiable=True), "trainable": dict(trainable=True),
            "force_trainable": dict(force_trainable=True)}


def _frame(periodic):
    """-> (pos, box or None, cutoff)"""
    if periodic:
        pos, box = cfconv_float64.frame("triclinic80")
        return pos, box, 4.0
    pos, _, cutoff = dispatch.frame("conformer90")
    assert cutoff == dispatch.CUTOFF
    return pos, None, cutoff


def _module(weights, **kw):
    from NNPOps.CFConv import CFConv
    w1, b1, w2, b2 = (torch.tensor(w) for w in weights)
    return CFConv(sigma_of(G), ACT, w1.reshape(G, W), b1, w2, b2, **kw).to(DEV)      # weights1: the core's [W][G] buffer seen as [G, W]


def _neighbors(pos, box, cutoff):
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    nb = CFConvNeighbors(cutoff)
    nb.build(torch.tensor(pos, device=DEV), None if box is None else torch.tensor(box, device=DEV))
    return nb


def _leaf(a, requires_grad=True):
    return None if a is None else torch.tensor(a, device=DEV, requires_grad=requires_grad)


class Call:
    """one forward pass on leaves of its own (the positions and the box hold the frame's values in every call)"""

    def __init__(self, conv, nb, pos, box, x, g, box_grad):
        self.pos, self.x, self.box, self.g = _leaf(pos), _leaf(x), _leaf(box, box_grad), torch.tensor(g, device=DEV)
        self.out = conv(nb, self.pos, self.x, self.box)

    def backward(self):
        self.out.backward(self.g)
        return dict(out=self.out.detach(), positions=self.pos.grad, input=self.x.grad,
                    box=self.box.grad if self.box is not None and self.box.requires_grad else None)


def _param_grads(conv):
    """copies of the four parameters' gradients, in PARAMS' order; none for a layer with fixed filters"""
    assert [n for n, _ in conv.named_parameters()] in ([], list(PARAMS))
    return [p.grad.clone() for p in conv.parameters()]


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert torch.equal(got[k], want[k]), (what, k)


# ---------------------------------------------------------------------------------------------- 1. two forward passes, then the first one's backward
@pytest.mark.parametrize("periodic", [False, True], ids=["open", "periodic"])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_first_backward_after_a_second_forward(monkeypatch, flavour, periodic):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    kw = FLAVOURS[flavour]
    pos, box, cutoff = _frame(periodic)
    box_grad = periodic and flavour in ("default", "trainable")          # (the recorded flavours refuse a box that wants a gradient)
    *weights, xa, ga = cfconv_float64.weights(W, G, len(pos), 4101)
    xb, gb = cfconv_float64.weights(W, G, len(pos), 4102)[4:]
    nb = _neighbors(pos, box, cutoff)                                     # one build for every call below

    alone, alone_params = [], []
    for x, g in ((xa, ga), (xb, gb)):                                     # each call alone, on a fresh module
        conv = _module(weights, **kw)
        alone.append(Call(conv, nb, pos, box, x, g, box_grad).backward())
        alone_params.append(_param_grads(conv))
    assert not torch.equal(alone[0]["input"], alone[1]["input"]) and not torch.equal(alone[0]["positions"], alone[1]["positions"])
    assert (alone[0]["box"] is not None) == box_grad

    conv = _module(weights, **kw)
    a = Call(conv, nb, pos, box, xa, ga, box_grad)
    b = Call(conv, nb, pos, box, xb, gb, box_grad)
    _same(a.backward(), alone[0], "first call")
    after_first = _param_grads(conv)
    _same(b.backward(), alone[1], "second call")
    after_second = _param_grads(conv)
    assert len(after_first) == (4 if flavour in ("trainable", "force_trainable") else 0)
    for name, first, second, pa, pb in zip(PARAMS, after_first, after_second, *alone_params):
        assert bool(pa.any()) and bool(pb.any()), name
        assert torch.equal(first, pa), name
        assert torch.equal(second, pa + pb), name                         # accumulated in the order of the two backward passes
    assert conv.holder.uploads() == (1 if after_first else 0)             # (the second forward pass found the weights in place)


# ---------------------------------------------------------------------------------------------- 2. the scripted surface
def test_scripted_forward_and_backward_of_the_holder(monkeypatch):
    """Holder.forward, then Holder.backward: {none, none, positionsGrad, inputGrad}, the bits of operation through autograd"""
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    pos, box, cutoff = _frame(False)
    w1, b1, w2, b2, x, g = cfconv_float64.weights(W, G, len(pos), 4103)
    nb = _neighbors(pos, None, cutoff)
    new = lambda: torch.classes.NNPOpsCFConv.Holder(sigma_of(G), ACT, torch.tensor(w1).reshape(G, W), torch.tensor(b1), torch.tensor(w2),
                                                    torch.tensor(b2))
    tpos, tx, tg = _leaf(pos), _leaf(x), torch.tensor(g, device=DEV)
    out = torch.ops.NNPOpsCFConv.operation(new(), nb.holder, tpos, tx)
    out.backward(tg)

    holder = new()
    direct = holder.forward(nb.holder, tpos.detach(), tx.detach())
    grads = holder.backward([tg])
    assert torch.equal(direct, out.detach())
    assert len(grads) == 4 and grads[0] is None and grads[1] is None
    assert torch.equal(grads[2], tpos.grad) and torch.equal(grads[3], tx.grad)
    assert holder.uploads() == 0


# ---------------------------------------------------------------------------------------------- 3. two flavours on one list
def test_a_force_trainable_and_a_default_layer_interleaved_on_one_list(monkeypatch):
    """forward A, forward B, grad(E_A, positions, create_graph=True), then the loss's backward: each layer's results are those of its
    own run, and so are the upload counters"""
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    pos, box, cutoff = _frame(False)
    *wa, xa, ra = cfconv_float64.weights(W, G, len(pos), 4104)
    *wb, xb, rb = cfconv_float64.weights(W, G, len(pos), 4105)
    nb = _neighbors(pos, None, cutoff)
    dev = lambda a: torch.tensor(a, device=DEV)

    def forward_a(conv):
        p = _leaf(pos)
        return p, (conv(nb, p, dev(xa)) * dev(ra)).sum()

    def finish_a(conv, p, E):
        F, = torch.autograd.grad(E, p, create_graph=True)
        return (F ** 2).sum() + E

    def forward_b(conv):
        p, x = _leaf(pos), _leaf(xb)
        return p, x, (conv(nb, p, x) * dev(rb)).sum()

    conv_a, conv_b = _module(wa, force_trainable=True), _module(wb)      # each alone
    pa, E = forward_a(conv_a)
    finish_a(conv_a, pa, E).backward()
    pb, x, E = forward_b(conv_b)
    E.backward()
    want = dict(pa=pa.grad, pb=pb.grad, xb=x.grad, **dict(zip(PARAMS, _param_grads(conv_a))))
    want_uploads = (conv_a.holder.uploads(), conv_b.holder.uploads())
    assert want_uploads == (1, 0)

    conv_a, conv_b = _module(wa, force_trainable=True), _module(wb)      # interleaved
    pa, E_a = forward_a(conv_a)
    pb, x, E_b = forward_b(conv_b)
    (finish_a(conv_a, pa, E_a) + E_b).backward()
    got = dict(pa=pa.grad, pb=pb.grad, xb=x.grad, **dict(zip(PARAMS, _param_grads(conv_a))))
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert (conv_a.holder.uploads(), conv_b.holder.uploads()) == want_uploads
