"""Box-vector gradient (virial) of the periodic CFConv: nnpops_cfconv_backprop_box and the torch surface above it.

The judge is the float64 restatement of tests/cfconv_float64.py (pinned by tests/test_cfconv_box_gradient_reference_cpu.py to the
float32 oracle and to finite differences of itself): L = <gout, CFConv(x)> with seeded float32 weights and inputs, dL/dB with the
minimum-image shifts held fixed, all nine entries.  One float64 evaluation per (system, layer), kept for the module.

Bar (the project's force tolerance, FORCE_RTOL of test_cfconv_gpu.py): max |gB - gB_ref| <= 1e-4 max |gB_ref|.
Every evaluation also asserts: gB finite and non-trivial; the input and position gradients are the plain backprop()'s, bit for
bit; two calls give equal bits; the stress is symmetric -- the antisymmetric part of W = sum_i x_i (x) dL/dx_i + B^T dL/dB
(rotation invariance of the convolution) stays below 1e-4 of the largest entry of W.  Every evaluation prints its measured figures
(pytest -s).

Which kernels a layer runs follows the selection rule of nnpops_cfconv_create (cfconv.hip, ConvPath):
    W 32, G 16          both layers split-fp16, register-fed (cfconv_filters_h2b)        ssp and tanh
    W 32, G 70          layer 2 split through LDS planes (cfconv_filters_h2)
    W 16, G 8           fp32 matrix instruction (cfconv_filters_mfma)
    W 24, G 10          vector kernel, weights in LDS (cfconv_kernel, and its ROW_S walk for the pair scalars)
    W 130, G 20         vector kernel, weights streamed
    W 128, G 50         the config-3 kernel
and $NNPOPS_CFCONV_VALU=1 / $NNPOPS_CFCONV_SPLIT=0 (read when the convolution is created) put W 32 on the vector and the fp32
matrix kernels.  Systems: a 350-atom triclinic frame (all-pairs build), 1 500 atoms (cell-grid build, cell-ordered walk), 1 100
atoms at twice the density (rows longer than a wave), and the 600-atom frame moved 0.37 box lengths along x, then wrapped back by
one box vector (other shifts, another dL/dB, each judged on its own).

Measured on an MI355X (worst box-gradient error per path, of the largest entry): register-fed split 1.9e-6 (ssp) / 1.8e-6 (tanh), LDS
planes 3.3e-6, fp32 matrix 1.5e-6, vector 1.4e-6, vector with streamed weights 2.9e-6, config-3 kernel 1.4e-5, NNPOPS_CFCONV_VALU=1
1.6e-6, NNPOPS_CFCONV_SPLIT=0 1.9e-6; antisymmetric stress at most 2.2e-6 of its largest entry.
"""
import numpy as np
import pytest
import torch

from box_gradient_judge import clean_env, judge
from cfconv_float64 import Restatement, frame, handles, layer as _layer, sigma_of, weights      # (tests here call their module layer)
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu

FORCE_RTOL = 1e-4
DEV = torch.device("cuda:0")
CUTOFF = 5.0

_REFERENCES = {}


def _reference(tag, W, G, act):
    """float64: the judge's dict, once per (system, layer)"""
    key = (tag, W, G, act)
    if key not in _REFERENCES:
        pos, box = frame(tag)
        w1, b1, w2, b2, x, gy = _layer(tag, W, G)
        _REFERENCES[key] = Restatement(W, G, CUTOFF, sigma_of(G), act, w1, b1, w2, b2).evaluate(pos, box, x, gy)
    return _REFERENCES[key]


def _evaluate(nb, cf, tag, W, G, forward_first=True, pos=None):
    """build(), [compute()], the plain backprop(), two backprop_box() -> (position gradient, box gradient) as float64 numpy arrays"""
    if pos is None:
        pos, box = frame(tag)
    else:
        box = frame(tag)[1]
    _, _, _, _, x, gy = _layer(tag, W, G)
    tpos, tbox, tx, tg = (torch.tensor(a, device=DEV) for a in (pos, box, x, gy))
    nb.build(tpos, tbox)
    if forward_first:
        cf.compute(nb, tpos, tx, tbox)
    plain = [t.clone() for t in cf.backprop(nb, tpos, tx, tg, tbox)]
    first = [t.clone() for t in cf.backprop_box(nb, tpos, tx, tg, tbox)]
    second = cf.backprop_box(nb, tpos, tx, tg, tbox)
    torch.cuda.synchronize()
    assert torch.equal(first[2], second[2]), "two calls give different box gradients"
    for k, name in enumerate(("input", "position")):
        assert torch.equal(first[k], plain[k]) and torch.equal(second[k], plain[k]), f"the {name} gradient is not the plain backprop()'s"
    assert first[2].shape == (3, 3) and first[2].dtype == torch.float32
    return first[1].cpu().numpy().astype(np.float64), first[2].cpu().numpy().astype(np.float64)


def _judge(label, tag, ref, g, gbox, pos=None):
    judge("cfconv-box", label, frame(tag)[0] if pos is None else pos, frame(tag)[1], ref, g, gbox, FORCE_RTOL)


def _clean_env(monkeypatch):
    clean_env(monkeypatch, "NNPOPS_CFCONV_")


# ---------------------------------------------------------------------------------------------- every kernel path
PATHS = {                      # name: (W, G, activation, systems)
    "split-registers-ssp": (32, 16, "ssp", ["triclinic350", "liquid1500", "dense1100", "liquid600_shifted", "liquid600_wrapped"]),
    "split-registers-tanh": (32, 16, "tanh", ["triclinic350", "liquid1500"]),
    "split-planes": (32, 70, "ssp", ["triclinic350", "liquid1500"]),
    "fp32-matrix": (16, 8, "ssp", ["triclinic350", "dense1100"]),
    "vector": (24, 10, "ssp", ["triclinic350", "liquid1500", "dense1100", "liquid600_wrapped"]),
    "vector-streamed": (130, 20, "tanh", ["triclinic350", "liquid1500"]),
    "config3": (128, 50, "ssp", ["triclinic350", "liquid1500", "dense1100"]),
}
CASES = [(name, tag) for name, (_, _, _, tags) in PATHS.items() for tag in tags]


@pytest.mark.parametrize("path,tag", CASES, ids=[f"{p}-{t}" for p, t in CASES])
def test_box_gradient_against_float64(monkeypatch, path, tag):
    _clean_env(monkeypatch)
    W, G, act, _ = PATHS[path]
    ref = _reference(tag, W, G, act)
    nb, cf = handles(tag, W, G, act, CUTOFF)
    g, gbox = _evaluate(nb, cf, tag, W, G)
    if tag in ("liquid1500", "dense1100"):
        assert nb.read_grid()["ok"], nb.read_grid()            # the cell grid built these rows
    if tag == "dense1100":
        assert int(np.bincount(np.concatenate([ref["i"], ref["j"]])).max()) > 64       # rows longer than a wave
    _judge(f"{path} W={W} G={G} {act} {tag}", tag, ref, g, gbox)
    if tag == "liquid600_wrapped":
        # the same atoms, a third of them one box vector away: other shifts, and a dL/dB that differs far beyond the bar
        other = _reference("liquid600_shifted", W, G, act)
        assert np.abs(other["gbox"] - ref["gbox"]).max() > 100 * FORCE_RTOL * np.abs(ref["gbox"]).max()
        assert not np.array_equal(other["n"], ref["n"])


@pytest.mark.parametrize("switch,value", [("VALU", "1"), ("SPLIT", "0")])
@pytest.mark.parametrize("tag", ["triclinic350", "liquid1500"])
def test_box_gradient_on_the_forced_paths(monkeypatch, switch, value, tag):
    """W = 32 on the vector kernel ($NNPOPS_CFCONV_VALU=1) and on the fp32 matrix kernel ($NNPOPS_CFCONV_SPLIT=0)"""
    _clean_env(monkeypatch)
    monkeypatch.setenv("NNPOPS_CFCONV_" + switch, value)
    W, G, act = 32, 16, "ssp"
    ref = _reference(tag, W, G, act)
    nb, cf = handles(tag, W, G, act, CUTOFF)
    g, gbox = _evaluate(nb, cf, tag, W, G)
    _judge(f"{switch}={value} W={W} G={G} {act} {tag}", tag, ref, g, gbox)


# ---------------------------------------------------------------------------------------------- exact cases
def test_two_atoms_across_the_boundary():
    from nnpops_amd.capi import CFConv, CFConvNeighbors
    pos = np.array([[0.4, 5.0, 5.1], [9.5, 5.3, 4.8]], dtype=np.float32)
    box = (np.eye(3) * 10).astype(np.float32)
    for W, G in ((16, 8), (24, 10)):                       # a matrix-core layer and a vector one
        w1, b1, w2, b2, x, gy = weights(W, G, 2, 7)
        ref = Restatement(W, G, 3.0, 0.4, "ssp", w1, b1, w2, b2).evaluate(pos, box, x, gy)
        assert len(ref["i"]) == 1 and np.array_equal(ref["n"], [[-1.0, 0.0, 0.0]])
        nb, cf = CFConvNeighbors(2, 3.0, True), CFConv(2, W, G, 3.0, 0.4, "ssp", w1, b1, w2, b2, periodic=True)
        tpos, tbox, tx, tg = (torch.tensor(a, device=DEV) for a in (pos, box, x, gy))
        nb.build(tpos, tbox)
        _, pg, gb = cf.backprop_box(nb, tpos, tx, tg, tbox)
        gb = gb.cpu().numpy().astype(np.float64)
        top = np.abs(ref["gbox"]).max()
        print(f"\n[cfconv-box] two atoms W={W}: box gradient {np.abs(gb - ref['gbox']).max() / top:.2e} of max {top:.3e}")
        assert top > 0 and np.abs(gb - ref["gbox"]).max() <= FORCE_RTOL * top
        assert np.array_equal(gb[1:], np.zeros((2, 3)))     # only the a vector carries a shift
        # one pair: dL/dB[0] = n_x dL/dd = -(force on atom 1), in the kernel's own float32 numbers
        assert np.abs(gb[0] + pg[1].cpu().numpy().astype(np.float64)).max() <= FORCE_RTOL * top


def test_nothing_wraps_in_a_large_box():
    from nnpops_amd.capi import CFConv, CFConvNeighbors
    pos, _ = workloads.conformer(60, seed=4)
    box = (np.eye(3) * 100).astype(np.float32)
    for W, G in ((32, 16), (24, 10)):
        w1, b1, w2, b2, x, gy = weights(W, G, 60, 8)
        nb, cf = CFConvNeighbors(60, CUTOFF, True), CFConv(60, W, G, CUTOFF, 0.4, "ssp", w1, b1, w2, b2, periodic=True)
        tpos, tbox, tx, tg = (torch.tensor(a, device=DEV) for a in (pos, box, x, gy))
        nb.build(tpos, tbox)
        _, pg, gb = cf.backprop_box(nb, tpos, tx, tg, tbox)
        assert float(pg.abs().max()) > 0
        assert torch.equal(gb, torch.zeros(3, 3, device=DEV))


# ---------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize("path", ["config3", "vector"])
def test_without_a_preceding_forward_call(monkeypatch, path):
    """backprop_box() on a build no compute() has seen stores its own filter rows (the case above reads the forward call's back)"""
    _clean_env(monkeypatch)
    W, G, act, _ = PATHS[path]
    tag = "liquid1500"
    ref = _reference(tag, W, G, act)
    nb, cf = handles(tag, W, G, act, CUTOFF)
    g, gbox = _evaluate(nb, cf, tag, W, G, forward_first=False)
    _judge(f"{path} {tag} no forward call", tag, ref, g, gbox)


@pytest.mark.parametrize("path", ["split-registers-ssp", "vector"])
def test_follows_a_rebuild(monkeypatch, path):
    """After a rebuild on moved positions (other pairs, other shifts) the same handles give what fresh handles give, bit for bit"""
    _clean_env(monkeypatch)
    W, G, act, _ = PATHS[path]
    tag = "liquid1500"
    pos, box = frame(tag)
    moved = (pos + np.random.default_rng(3).normal(0, 0.3, pos.shape)).astype(np.float32)
    nb, cf = handles(tag, W, G, act, CUTOFF)
    g0, b0 = _evaluate(nb, cf, tag, W, G)
    g1, b1 = _evaluate(nb, cf, tag, W, G, pos=moved)
    g2, b2 = _evaluate(*handles(tag, W, G, act, CUTOFF), tag, W, G, pos=moved)
    assert np.array_equal(b1, b2) and np.array_equal(g1, g2)
    assert np.abs(b1 - b0).max() > 100 * FORCE_RTOL * np.abs(b0).max()
    w1, b1_, w2, b2_, x, gy = _layer(tag, W, G)
    ref = Restatement(W, G, CUTOFF, sigma_of(G), act, w1, b1_, w2, b2_).evaluate(moved, box, x, gy)
    _judge(f"{path} {tag} rebuilt on moved positions", tag, ref, g1, b1, pos=moved)


# ---------------------------------------------------------------------------------------------- errors
def test_refused_without_a_periodic_list_or_a_box():
    from nnpops_amd.capi import NNPOpsHipError
    tag, W, G, act = "triclinic350", 32, 16, "ssp"
    pos, box = frame(tag)
    _, _, _, _, x, gy = _layer(tag, W, G)
    tpos, tbox, tx, tg = (torch.tensor(a, device=DEV) for a in (pos, box, x, gy))
    nb, cf = handles(tag, W, G, act, CUTOFF, periodic=False)
    nb.build(tpos)
    with pytest.raises(NNPOpsHipError, match="periodic"):
        cf.backprop_box(nb, tpos, tx, tg, tbox)
    nb, cf = handles(tag, W, G, act, CUTOFF)
    nb.build(tpos, tbox)
    with pytest.raises(NNPOpsHipError, match="NULL"):
        cf.backprop_box(nb, tpos, tx, tg, None)
    xg, pg, gb = cf.backprop_box(nb, tpos, tx, tg, tbox)      # the handles are still good
    assert bool(torch.isfinite(gb).all()) and float(gb.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- the torch surface
def _torch_layer(tag, W, G, act):
    """-> a module around the neighbour list and the convolution, as a model holds them (scriptable)"""
    from typing import Optional
    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    w1, b1, w2, b2, _, _ = _layer(tag, W, G)

    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.neighbors = CFConvNeighbors(CUTOFF)
            # the module takes weights1 as [G, W], a reinterpretation of the core's [W][G] buffer (CFConv.py, torch_binding.cpp)
            self.conv = CFConv(sigma_of(G), act, torch.tensor(w1).reshape(G, W), torch.tensor(b1), torch.tensor(w2), torch.tensor(b2))

        def forward(self, positions: torch.Tensor, x: torch.Tensor, build_box: Optional[torch.Tensor], box: Optional[torch.Tensor]) -> torch.Tensor:
            self.neighbors.build(positions, build_box)
            return self.conv(self.neighbors, positions, x, box)

    return Layer()


@pytest.mark.parametrize("path", ["split-registers-ssp", "vector"])
def test_torch_box_gradient_is_the_c_abi_result(monkeypatch, path):
    """box.requires_grad_(): box.grad is the C ABI's result bit for bit, positions.grad and input.grad the bits of a call without a
    box; a box that does not require a gradient gets None; a scripted module gives the same numbers."""
    _clean_env(monkeypatch)
    W, G, act, _ = PATHS[path]
    tag = "liquid1500"
    pos, box = frame(tag)
    _, _, _, _, x, gy = _layer(tag, W, G)
    tg = torch.tensor(gy, device=DEV)
    layer = _torch_layer(tag, W, G, act)

    def run(module, with_box, box_grad):
        tpos = torch.tensor(pos, device=DEV).requires_grad_(True)
        tx = torch.tensor(x, device=DEV).requires_grad_(True)
        tbox = torch.tensor(box, device=DEV).requires_grad_(box_grad)
        out = module(tpos, tx, tbox, tbox if with_box else None)
        (out * tg).sum().backward()
        return out.detach(), tpos.grad, tx.grad, tbox.grad

    out0, gp0, gx0, none0 = run(layer, False, False)
    out1, gp1, gx1, none1 = run(layer, True, False)
    out2, gp2, gx2, gb2 = run(layer, True, True)
    out3, gp3, gx3, gb3 = run(torch.jit.script(_torch_layer(tag, W, G, act)), True, True)
    torch.cuda.synchronize()
    assert none0 is None and none1 is None
    assert gb2 is not None and gb2.shape == (3, 3) and gb2.dtype == torch.float32
    for o, p, xg in ((out1, gp1, gx1), (out2, gp2, gx2), (out3, gp3, gx3)):
        assert torch.equal(o, out0) and torch.equal(p, gp0) and torch.equal(xg, gx0)
    assert torch.equal(gb3, gb2)
    ref = _reference(tag, W, G, act)
    g_abi, b_abi = _evaluate(*handles(tag, W, G, act, CUTOFF), tag, W, G)
    assert np.array_equal(gb2.cpu().numpy().astype(np.float64), b_abi)
    assert np.array_equal(gp2.cpu().numpy().astype(np.float64), g_abi)
    _judge(f"torch {path} {tag}", tag, ref, g_abi, b_abi)


def test_torch_box_gradient_replays_in_a_captured_graph(monkeypatch):
    """Build + forward + backward with a box gradient captured once (after warm-up steps: the scratch belongs to the handles) and
    replayed on new positions gives the eager result, bit for bit."""
    _clean_env(monkeypatch)
    tag, W, G, act = "liquid1500", 32, 16, "ssp"
    pos, box = frame(tag)
    _, _, _, _, x, gy = _layer(tag, W, G)
    layer = _torch_layer(tag, W, G, act)
    tbox = torch.tensor(box, device=DEV).requires_grad_(True)
    tx = torch.tensor(x, device=DEV).requires_grad_(True)
    tg = torch.tensor(gy, device=DEV)
    static_pos = torch.tensor(pos, device=DEV).requires_grad_(True)

    def step(p):
        return torch.autograd.grad((layer(p, tx, tbox, tbox) * tg).sum(), [p, tx, tbox])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                              # calibrates neighbour capacities, sizes the scratch
            step(static_pos)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_pos, g_x, g_box = step(static_pos)
    rng = np.random.default_rng(1)
    for _ in range(2):
        new = (pos + rng.normal(0, 0.05, pos.shape)).astype(np.float32)
        with torch.no_grad():
            static_pos.copy_(torch.tensor(new, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        e_pos, e_x, e_box = step(static_pos.detach().clone().requires_grad_(True))
        assert torch.equal(g_box, e_box) and torch.equal(g_pos, e_pos) and torch.equal(g_x, e_x)
        assert float(e_box.abs().max()) > 0


def test_torch_argument_checks():
    tag, W, G, act = "triclinic350", 32, 16, "ssp"
    pos, box = frame(tag)
    _, _, _, _, x, _ = _layer(tag, W, G)
    tpos, tbox, tx = (torch.tensor(a, device=DEV) for a in (pos, box, x))
    layer = _torch_layer(tag, W, G, act)
    with pytest.raises(RuntimeError, match="without a box"):
        layer(tpos, tx, None, tbox)                                     # a non-periodic list
    layer = _torch_layer(tag, W, G, act)
    with pytest.raises(RuntimeError, match='type of "box"'):
        layer(tpos, tx, tbox, tbox.double())
    with pytest.raises(RuntimeError, match='shape of "box"'):
        layer(tpos, tx, tbox, tbox[:2])
    with pytest.raises(RuntimeError, match="box"):
        layer(tpos, tx, tbox, tbox.cpu())
    assert bool(torch.isfinite(layer(tpos, tx, tbox, tbox)).all())
