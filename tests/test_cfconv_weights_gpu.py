"""The gradients of the CFConv filter network's weights (nnpops_cfconv_backprop_weights, nnpops_cfconv_set_weights and
CFConv(..., trainable=True)) on the GPU, against float64.

The judge, its closed form, the float32 witness and the table of cases are in tests/cfconv_weights_float64.py;
tests/test_cfconv_weights_reference_cpu.py pins them without a GPU and shows that the witness sits inside half of the bar on every case.

BAR: each of the four gradients within FORCE_RTOL = 1e-4 (cfconv_float64.py) of the judge, as a fraction of that gradient's largest
entry -- the project's bar for CFConv gradients, widened for no case.  Every judged case prints its four errors and the witness's on
the same case (pytest -s).  Measured on an MI355X (docs/LAB_NOTEBOOK_cfconv_weights.md has the table): the worst error over the table
is 9.4e-7 of the largest entry (w128_g104_last_mfma-tanh, w1), 0.0094 of the bar; the worst ratio to the witness on the same case is
2.48 (chain1_w16_g8-ssp: one pair, 2.1e-7 against 8.4e-8).  60 tests, 5 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cfconv_weights_float64 as wf
from box_gradient_judge import clean_env
from cfconv_float64 import sigma_of
from nnpops_amd import capi, workloads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_WORDS = {wf.REG: "split_registers", wf.PLANES: "split_planes", wf.MATRIX: "matrix", wf.VECTOR: "vector"}


def _env(monkeypatch, case=None):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")
    for k, v in (case.env if case is not None else ()):
        monkeypatch.setenv(k, v)


def _handles(case, weights=None):
    pos, box, cutoff = wf.frame(case.frame)
    w1, b1, w2, b2, x, g = wf.layer(case.frame, case.W, case.G)
    if weights is not None:
        w1, b1, w2, b2 = weights
    periodic = box is not None
    nb = capi.CFConvNeighbors(len(pos), cutoff, periodic)
    cf = capi.CFConv(len(pos), case.W, case.G, cutoff, sigma_of(case.G), case.act, w1, b1, w2, b2, periodic=periodic)
    tpos = torch.tensor(pos, device=DEV)
    tbox = torch.tensor(box, device=DEV) if periodic else None
    nb.build(tpos, tbox)
    return nb, cf, tpos, tbox, torch.tensor(x, device=DEV), torch.tensor(g, device=DEV)


def _numpy(grads):
    return {n: t.cpu().numpy() for n, t in zip(wf.NAMES, grads)}


def _case(name):
    return next(c for c in wf.CASES if c.name == name)


# ---------------------------------------------------------------------------------------------- every case of the table
@pytest.mark.parametrize("case", wf.CASES, ids=[c.name for c in wf.CASES])
def test_weight_gradients_against_float64(monkeypatch, case):
    _env(monkeypatch, case)
    ref = wf.reference(case)
    nb, cf, tpos, tbox, tx, tg = _handles(case)
    assert cf.describe()["path"] == PATH_WORDS[case.path]              # the forward path the row names
    assert wf.expected_kernel(case.W, case.G) == case.kernel
    assert nb.num_pairs() == len(ref["i"])
    first = cf.backprop_weights(nb, tx, tg)
    second = cf.backprop_weights(nb, tx, tg)
    torch.cuda.synchronize()
    got = _numpy(first)
    for n, a, b in zip(wf.NAMES, first, second):
        assert torch.equal(a, b), n                                     # two calls agree bit for bit
        assert np.all(np.isfinite(got[n])), n
    err, wit = wf.errors(got, ref["judge"]), wf.errors(ref["witness"], ref["judge"])
    print(f"\n{case.name} [{case.kernel}] pairs {len(ref['i'])}: {wf.figures(err)} | witness {wf.figures(wit)}")
    if len(ref["i"]) == 0:
        for n in wf.NAMES:
            assert not np.any(got[n]), n                                # no pair: exact zeros
    for n in wf.NAMES:
        assert err[n] <= wf.BAR, (n, err[n])


def test_batched_molecules_sum_the_molecules_own_gradients(monkeypatch):
    """three molecules whose coordinates overlap behind one list: the gradients are the sum of the molecules' own"""
    _env(monkeypatch)
    sizes = (30, 17, 25)
    pos = np.concatenate([workloads.conformer(n, seed=20 + k)[0] for k, n in enumerate(sizes)]).astype(np.float32)
    offsets = [0, 30, 47, 72]
    for W, G, act in ((16, 8, "ssp"), (24, 10, "tanh")):
        w1, b1, w2, b2, x, g = wf.cfconv_float64.weights(W, G, len(pos), 7000 + W)
        J = wf.judge_of(W, G, 5.0, act, w1, b1, w2, b2)
        i, j, r = wf.pair_list(J, pos, offsets=offsets)
        whole = wf.pair_list(J, pos)
        assert len(whole[0]) > len(i)                                   # (the molecules do overlap: one list of all atoms has more pairs)
        ref = wf.judge(J, i, j, r, x, g)
        nb = capi.CFConvNeighbors(len(pos), 5.0, False)
        nb.set_molecules(offsets)
        cf = capi.CFConv(len(pos), W, G, 5.0, sigma_of(G), act, w1, b1, w2, b2)
        tpos = torch.tensor(pos, device=DEV)
        nb.build(tpos)
        assert nb.num_pairs() == len(i)
        got = _numpy(cf.backprop_weights(nb, torch.tensor(x, device=DEV), torch.tensor(g, device=DEV)))
        err = wf.errors(got, ref)
        print(f"\nbatched W={W} G={G}: {wf.figures(err)}")
        assert max(err.values()) <= wf.BAR, err


# ---------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("name", ["w64_g50-ssp", "w136_g10-tanh"])
def test_zero_output_gradient_gives_exact_zeros(monkeypatch, name):
    _env(monkeypatch)
    nb, cf, tpos, tbox, tx, tg = _handles(_case(name))
    for t in cf.backprop_weights(nb, tx, torch.zeros_like(tg)):
        assert not bool(t.any())


@pytest.mark.parametrize("name", ["w64_g50-ssp", "w16_g8-tanh", "w136_g10-tanh"])
def test_compute_and_backprop_keep_their_bits_around_a_weight_gradient_call(monkeypatch, name):
    _env(monkeypatch)
    nb, cf, tpos, tbox, tx, tg = _handles(_case(name))
    out0 = cf.compute(nb, tpos, tx, tbox)
    gx0, gp0 = cf.backprop(nb, tpos, tx, tg, tbox)
    cf.backprop_weights(nb, tx, tg)
    gx1, gp1 = cf.backprop(nb, tpos, tx, tg, tbox)
    out1 = cf.compute(nb, tpos, tx, tbox)
    assert torch.equal(out0, out1) and torch.equal(gx0, gx1) and torch.equal(gp0, gp1)


@pytest.mark.parametrize("name", ["w48_g7-ssp", "w8_g10-tanh"])
def test_sentinels_behind_the_four_outputs_survive(monkeypatch, name):
    _env(monkeypatch)
    case = _case(name)
    nb, cf, tpos, tbox, tx, tg = _handles(case)
    W, G, pad = case.W, case.G, 64
    sizes = [W * G, W, W * W, W]
    buf = torch.full((sum(sizes) + pad * 5,), 12345.0, device=DEV)
    starts = np.cumsum([pad] + [s + pad for s in sizes[:-1]])
    ptrs = [C.c_void_p(buf.data_ptr() + 4 * int(s)) for s in starts]
    L = capi.lib()
    assert L.nnpops_cfconv_backprop_weights(cf._h, nb._h, C.c_void_p(tx.data_ptr()), C.c_void_p(tg.data_ptr()), *ptrs) == 0
    host = buf.cpu().numpy()
    want = _numpy(cf.backprop_weights(nb, tx, tg))
    inside = np.zeros(len(host), bool)
    for n, s, size in zip(wf.NAMES, starts, sizes):
        inside[s:s + size] = True
        assert np.array_equal(host[s:s + size], want[n].reshape(-1)), n       # fully overwritten, the same bits
    assert np.all(host[~inside] == 12345.0)


def test_errors_are_reported_with_a_message(monkeypatch):
    _env(monkeypatch)
    case = _case("w16_g8-ssp")
    nb, cf, tpos, tbox, tx, tg = _handles(case)
    L = capi.lib()
    out = [torch.empty(n, device=DEV) for n in (16 * 8, 16, 256, 16)]
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.nnpops_cfconv_backprop_weights(cf._h, nb._h, p(tx), p(tg), p(out[0]), None, p(out[2]), p(out[3])) < 0
    assert b"NULL" in L.nnpops_last_error()
    assert L.nnpops_cfconv_backprop_weights(cf._h, nb._h, None, p(tg), *map(p, out)) < 0
    assert b"NULL" in L.nnpops_last_error()
    unbuilt = capi.CFConvNeighbors(len(tpos), 5.0, False)
    assert L.nnpops_cfconv_backprop_weights(cf._h, unbuilt._h, p(tx), p(tg), *map(p, out)) < 0
    assert b"not been built" in L.nnpops_last_error()
    other = capi.CFConvNeighbors(len(tpos) + 1, 5.0, False)
    other.build(torch.cat([tpos, tpos[:1] + 50.0]))
    assert L.nnpops_cfconv_backprop_weights(cf._h, other._h, p(tx), p(tg), *map(p, out)) < 0
    assert b"atoms" in L.nnpops_last_error()
    assert L.nnpops_cfconv_set_weights(cf._h, None, None, None, None) < 0
    assert b"NULL" in L.nnpops_last_error()


# ---------------------------------------------------------------------------------------------- set_weights
def _results(nb, cf, tpos, tbox, tx, tg):
    out = cf.compute(nb, tpos, tx, tbox)
    gx, gp = cf.backprop(nb, tpos, tx, tg, tbox)
    grads = cf.backprop_weights(nb, tx, tg)
    return [out, gx, gp, *grads]


@pytest.mark.parametrize("name", ["w64_g50-ssp", "w64_g50-tanh", "w16_g8-ssp", "w136_g10-tanh", "liquid1500_w32_g16-ssp"])
def test_set_weights_gives_the_bits_of_a_fresh_handle(monkeypatch, name):
    """... through a change of weights that moves a W = 64 layer from the split-fp16 plan to the fp32 plan and back"""
    _env(monkeypatch)
    case = _case(name)
    base = wf.layer(case.frame, case.W, case.G)[:4]
    rng = np.random.default_rng(99)
    moved = [(w + 0.05 * rng.standard_normal(w.shape)).astype(np.float32) for w in base]
    wide = [w.copy() for w in moved]
    wide[2][3, 5] = 6.0e4                                               # one entry of W2 outside the fp16 planes' range: no split kernels
    nb, cf, tpos, tbox, tx, tg = _handles(case)
    _results(nb, cf, tpos, tbox, tx, tg)                                # (the handle has run, and keeps filter rows of the old weights)
    plans = []
    for weights in (moved, wide, base):
        cf.set_weights(*weights)
        nb2, fresh, *_ = _handles(case, weights)
        assert cf.describe() == fresh.describe()
        plans.append(cf.describe()["path"])
        for k, (a, b) in enumerate(zip(_results(nb, cf, tpos, tbox, tx, tg), _results(nb2, fresh, tpos, tbox, tx, tg))):
            assert torch.equal(a, b), (k, plans)
    if case.W == 64:
        assert plans == ["split_registers", "matrix", "split_registers"]


# ---------------------------------------------------------------------------------------------- the torch surface
def _modules(W, G, act, weights, **kw):
    from NNPOps.CFConv import CFConv
    w1, b1, w2, b2 = (torch.tensor(w) for w in weights)
    return CFConv(sigma_of(G), act, w1.reshape(G, W), b1, w2, b2, **kw)      # weights1: the core's [W][G] buffer seen as [G, W]


def _neighbors(pos, box, cutoff):
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    nb = CFConvNeighbors(cutoff)
    nb.build(pos, box)
    return nb


@pytest.mark.parametrize("periodic", [False, True], ids=["open", "periodic"])
def test_module_gradients(monkeypatch, periodic):
    """the four parameter gradients against the judge; positions, input and box gradients bit-equal to the default ops'"""
    _env(monkeypatch)
    W, G, act = 32, 16, "ssp"
    if periodic:
        pos, box = wf.cfconv_float64.frame("cubic100")
        cutoff = 4.5
    else:
        (pos, box, cutoff) = wf.frame("conformer90")
    w1, b1, w2, b2, x, g = wf.cfconv_float64.weights(W, G, len(pos), 555)
    J = wf.judge_of(W, G, cutoff, act, w1, b1, w2, b2)
    i, j, r = wf.pair_list(J, pos, box)
    ref = wf.judge(J, i, j, r, x, g)
    leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
    results = []
    for trainable in (True, False):
        conv = _modules(W, G, act, (w1, b1, w2, b2), trainable=trainable).to(DEV)
        tpos, tx = leaf(pos), leaf(x)
        tbox = leaf(box) if periodic else None
        nb = _neighbors(tpos.detach(), None if tbox is None else tbox.detach(), cutoff)
        out = conv(nb, tpos, tx, tbox)
        (out * torch.tensor(g, device=DEV)).sum().backward()
        results.append((out.detach(), tpos.grad, tx.grad, None if tbox is None else tbox.grad))
        if trainable:
            got = dict(w1=conv.weights1.grad.cpu().numpy().reshape(W, G), b1=conv.biases1.grad.cpu().numpy(),
                       w2=conv.weights2.grad.cpu().numpy(), b2=conv.biases2.grad.cpu().numpy())
            assert conv.weights1.grad.shape == (G, W)
            err = wf.errors(got, ref)
            print(f"\nmodule periodic={periodic}: {wf.figures(err)}")
            assert max(err.values()) <= wf.BAR, err
    for a, b in zip(*results):
        assert (a is None and b is None) or torch.equal(a, b)


def test_three_sgd_steps_on_a_two_layer_stack(monkeypatch):
    """... lower a float64-judged loss and match the same three steps taken in the judge; the upload counter moves once per step"""
    _env(monkeypatch)
    W, G, act, lr = 16, 8, "tanh", 3e-4          # (the judge descends 36.3 -> 26.6 -> 20.7 -> 16.7 at this rate; updates ~1e-2)
    pos, box, cutoff = wf.frame("conformer90")
    n = len(pos)
    la = wf.cfconv_float64.weights(W, G, n, 811)
    lb = wf.cfconv_float64.weights(W, G, n, 812)
    x, target = la[4], 0.1 * lb[5]
    J = wf.judge_of(W, G, cutoff, act, *la[:4])
    i, j, r = wf.pair_list(J, pos)
    r64 = torch.tensor(r)

    def judged_loss(params):
        h = wf.layer_output(J, *params[:4], i, j, r64, wf._wide(x))
        out = wf.layer_output(J, *params[4:], i, j, r64, h)
        return ((out - wf._wide(target)) ** 2).mean()

    start = [wf._wide(w) for w in (*la[:4], *lb[:4])]
    params = [p.clone().requires_grad_(True) for p in start]
    losses = []
    for _ in range(3):
        L = judged_loss(params)
        losses.append(float(L.detach()))
        grads = torch.autograd.grad(L, params)
        params = [(p - lr * gr).detach().requires_grad_(True) for p, gr in zip(params, grads)]
    losses.append(float(judged_loss(params).detach()))
    assert losses[3] < losses[2] < losses[1] < losses[0], losses

    conv1 = _modules(W, G, act, la[:4], trainable=True).to(DEV)
    conv2 = _modules(W, G, act, lb[:4], trainable=True).to(DEV)
    tpos, tx, tt = torch.tensor(pos, device=DEV), torch.tensor(x, device=DEV), torch.tensor(target, device=DEV)
    nb = _neighbors(tpos, None, cutoff)
    opt = torch.optim.SGD(list(conv1.parameters()) + list(conv2.parameters()), lr=lr)
    assert len(opt.param_groups[0]["params"]) == 8
    for step in range(3):
        opt.zero_grad()
        loss = ((conv2(nb, tpos, conv1(nb, tpos, tx)) - tt) ** 2).mean()
        assert conv1.holder.uploads() == step + 1 and conv2.holder.uploads() == step + 1
        with torch.no_grad():                                           # a second forward pass on unchanged weights uploads nothing
            conv1(nb, tpos, tx)
        assert conv1.holder.uploads() == step + 1
        loss.backward()
        opt.step()
    mine = [p.detach().cpu().numpy().astype(np.float64) for p in (*conv1.parameters(), *conv2.parameters())]
    names = ["weights1", "biases1", "weights2", "biases2"]
    assert [n for n, _ in conv1.named_parameters()] == names
    # the judged loss at the GPU's weights is lower than at the start, and the accumulated updates are the judge's to the bar
    at_mine = [torch.tensor(m.reshape(s.shape)) for m, s in zip(mine, start)]
    assert float(judged_loss(at_mine)) < losses[0]
    assert abs(float(judged_loss(at_mine)) - losses[3]) <= wf.BAR * losses[0]
    for k, (m, p, s) in enumerate(zip(mine, params, start)):
        step_ref = (p.detach() - s).numpy()
        step_got = m.reshape(step_ref.shape) - s.numpy()
        # (bar on the update, plus the rounding of three float32 parameter updates: 3 x 2^-24 of the largest weight)
        bound = wf.BAR * np.abs(step_ref).max() + 3 * 2.0 ** -24 * np.abs(s.numpy()).max()
        assert np.abs(step_got - step_ref).max() <= bound, (k, np.abs(step_got - step_ref).max(), bound)


def test_state_dict_round_trip_and_scripting(monkeypatch, tmp_path):
    _env(monkeypatch)
    W, G, act = 16, 8, "ssp"
    pos, box, cutoff = wf.frame("conformer90")
    w1, b1, w2, b2, x, g = wf.cfconv_float64.weights(W, G, len(pos), 901)
    other = wf.cfconv_float64.weights(W, G, len(pos), 902)[:4]
    tpos, tx = torch.tensor(pos, device=DEV), torch.tensor(x, device=DEV)
    nb = _neighbors(tpos, None, cutoff)
    src = _modules(W, G, act, (w1, b1, w2, b2), trainable=True).to(DEV)
    dst = _modules(W, G, act, other, trainable=True).to(DEV)
    before = dst(nb, tpos, tx)
    assert sorted(src.state_dict()) == ["biases1", "biases2", "weights1", "weights2"]
    dst.load_state_dict(src.state_dict())
    want = src(nb, tpos, tx)
    after = dst(nb, tpos, tx)                                            # the live handle was given the loaded weights
    assert torch.equal(after, want) and not torch.equal(before, want)
    assert dst.holder.uploads() == 2
    assert torch.equal(_modules(W, G, act, (w1, b1, w2, b2)).to(DEV)(nb, tpos, tx), want)      # the default layer's bits

    class Layer(torch.nn.Module):                                        # (a module cannot be an argument of a scripted method)
        def __init__(self):
            super().__init__()
            from NNPOps.CFConvNeighbors import CFConvNeighbors
            self.neighbors = CFConvNeighbors(cutoff)
            self.conv = _modules(W, G, act, (w1, b1, w2, b2), trainable=True)

        def forward(self, positions, x):
            self.neighbors.build(positions)
            return self.conv(self.neighbors, positions, x)

    scripted = torch.jit.script(Layer().to(DEV))
    out = scripted(tpos, tx.clone().requires_grad_(True))
    assert torch.equal(out, want)
    out.sum().backward()
    assert scripted.conv.weights2.grad is not None and scripted.conv.weights2.grad.shape == (W, W)
    torch.jit.save(scripted, str(tmp_path / "layer.pt"))
    loaded = torch.jit.load(str(tmp_path / "layer.pt"))
    assert torch.equal(loaded(tpos, tx), want)


def test_refusals(monkeypatch):
    _env(monkeypatch)
    W, G, act = 16, 8, "ssp"
    pos, box, cutoff = wf.frame("conformer90")
    w1, b1, w2, b2, x, g = wf.cfconv_float64.weights(W, G, len(pos), 903)
    tpos = torch.tensor(pos, device=DEV, requires_grad=True)
    tx = torch.tensor(x, device=DEV, requires_grad=True)
    nb = _neighbors(tpos.detach(), None, cutoff)
    conv = _modules(W, G, act, (w1, b1, w2, b2), trainable=True).to(DEV)
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(conv(nb, tpos, tx).sum(), tpos, create_graph=True)
    out = conv(nb, tpos, tx)
    nb.build(tpos.detach())
    with pytest.raises(RuntimeError, match="rebuilt since the forward pass"):
        out.sum().backward()
    op = torch.ops.NNPOpsCFConv.operation_weights
    good = [conv.weights1, conv.biases1, conv.weights2, conv.biases2]
    for k, bad, what in [(0, conv.weights1.detach().reshape(W, G)[:, :G - 1], "shape of \"weights1\""),
                         (1, conv.biases1.detach()[:W - 1], "shape of \"biases1\""),
                         (2, conv.weights2.detach().double(), "type of \"weights2\""),
                         (3, conv.biases2.detach().half(), "type of \"biases2\"")]:
        args = list(good)
        args[k] = bad
        with pytest.raises(RuntimeError, match=what):
            op(conv.holder, nb.holder, tpos, tx, *args)
