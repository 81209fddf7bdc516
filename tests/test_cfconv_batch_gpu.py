"""Batched CFConv on the device: B molecules behind one neighbour list (nnpops_cfconv_neighbors_set_molecules / Holder.set_molecules).

Frames and judge: tests/cfconv_batch_float64.py (pinned by tests/test_cfconv_batch_reference_cpu.py).  Every molecule is centred on
the origin, so a builder that forgot the segments would list thousands of pairs between molecules; no intramolecular distance is
within 1e-4 A of the cutoff, so the exact list comparisons are unambiguous.
    ragged     sizes [1, 2, 21, 64, 65, 7], 160 atoms: an empty row, a full wave of candidates, one more than a wave
    frames64   64 x 21 = 1 344 atoms: a total at which the single-system list switches to the cell grid
    crowded    [5, 120, 12] at cutoff 9 A: rows of up to 119 entries, beyond the first row capacity (check() grows, build again)
Tolerances: OUT_RTOL / OUT_ATOL_FRAC / FORCE_RTOL of tests/cfconv_float64.py for compute and backprop, BAR and STEP_BAR of
tests/test_cfconv_second_order_gpu.py for the second derivatives, per kernel family (matrix: W a multiple of 16 up to 128).
"""
import numpy as np
import pytest
import torch

import cfconv_batch_float64 as batch
from cfconv_float64 import FORCE_RTOL, OUT_ATOL_FRAC, OUT_RTOL, Restatement, SecondOrder, sigma_of, weights

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = {"matrix": 8e-5, "vector": 4e-5}             # tests/test_cfconv_second_order_gpu.py
STEP_BAR = {"matrix": 7e-6, "vector": 1e-5}

LAYERS = {                     # name: (family of the second-order kernel, W, G, activation, environment)
    "split-registers-ssp": ("matrix", 128, 50, "ssp", {}),
    "split-registers-tanh": ("matrix", 128, 50, "tanh", {}),
    "split-planes": ("matrix", 128, 80, "ssp", {}),
    "fp32-matrix": ("matrix", 48, 12, "ssp", {}),
    "vector": ("vector", 20, 10, "tanh", {}),
    "valu-at-matrix-width": ("vector", 128, 50, "ssp", {"NNPOPS_CFCONV_VALU": "1"}),
}


def _dev(*arrays):
    return [None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV) for a in arrays]


def _list(n, cutoff, offsets=None):
    from nnpops_amd.capi import CFConvNeighbors
    nb = CFConvNeighbors(n, cutoff, False)
    if offsets is not None:
        nb.set_molecules(offsets)
    return nb


def _conv(tag, W, G, act, n=None, cutoff=None):
    from nnpops_amd.capi import CFConv
    w1, b1, w2, b2 = batch.batch_layer(tag, W, G)[:4]
    pos, _, c = batch.batch_frame(tag)
    return CFConv(len(pos) if n is None else n, W, G, c if cutoff is None else cutoff, sigma_of(G), act, w1, b1, w2, b2)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------- the list
@pytest.mark.parametrize("tag", ["ragged", "frames64", "crowded"])
def test_list_is_the_union_of_the_molecules_lists(tag):
    pos, offsets, cutoff = batch.batch_frame(tag)
    nb = _list(len(pos), cutoff, offsets)
    tpos, = _dev(pos)
    nb.build(tpos)
    atoms, dist = nb.export()
    want_i, want_j, want_d = [], [], []
    for lo, hi in batch.segments(offsets):
        one = _list(hi - lo, cutoff)
        one.build(tpos[lo:hi].contiguous())
        a, d = one.export()
        assert one.num_pairs() == a.shape[1]
        want_i.append(a[0] + lo); want_j.append(a[1] + lo); want_d.append(d)
    want_i, want_j, want_d = np.concatenate(want_i), np.concatenate(want_j), np.concatenate(want_d)
    assert nb.num_pairs() == len(want_i)
    assert np.array_equal(atoms[0], want_i) and np.array_equal(atoms[1], want_j)
    assert np.array_equal(dist.view(np.int32), want_d.view(np.int32)), "distances differ in their bits"
    # ... which is the float64 list
    ri, rj = batch.half_pairs(pos, offsets, cutoff)
    assert np.array_equal(atoms[0], ri) and np.array_equal(atoms[1], rj)
    if tag == "crowded":
        rows = np.bincount(np.concatenate([ri, rj]), minlength=len(pos))
        assert rows.max() > 64                               # the first build overflowed its rows; build() grew them and built again
        assert nb.build_count() > 0


# ---------------------------------------------------------------------------------------------- values
def _check_first(tag, out, gx, gp, ref):
    out, gx, gp = (t.cpu().numpy().astype(np.float64) for t in (out, gx, gp))
    e_out = np.abs(out - ref["out"]).max() / np.abs(ref["out"]).max()
    e_gx = np.abs(gx - ref["gx"]).max() / np.abs(ref["gx"]).max()
    e_gp = np.abs(gp - ref["g"]).max() / np.abs(ref["g"]).max()
    np.testing.assert_allclose(out, ref["out"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(ref["out"]).max())
    np.testing.assert_allclose(gx, ref["gx"], rtol=OUT_RTOL, atol=OUT_ATOL_FRAC * np.abs(ref["gx"]).max())
    assert np.abs(gp - ref["g"]).max() <= FORCE_RTOL * np.abs(ref["g"]).max()
    return e_out, e_gx, e_gp


def _check_second(got, ref, family):
    errs = []
    for name, t in zip(("dg", "dx", "dp"), got):
        top = float(np.abs(ref[name]).max())
        assert top > 0
        errs.append(float(np.abs(t.cpu().numpy().astype(np.float64) - ref[name]).max()) / top)
    assert max(errs) <= BAR[family], errs
    return errs


@pytest.mark.parametrize("tag", ["ragged", "frames64"])
@pytest.mark.parametrize("name", list(LAYERS))
def test_values_against_float64_and_against_a_loop(name, tag, monkeypatch):
    family, W, G, act, env = LAYERS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pos, offsets, cutoff = batch.batch_frame(tag)
    ref = batch.reference(tag, W, G, act)
    nb, cf = _list(len(pos), cutoff, offsets), _conv(tag, W, G, act)
    tpos, = _dev(pos)
    x, gy, V, Q = _dev(*batch.batch_layer(tag, W, G)[4:])
    nb.build(tpos)
    atoms, _ = nb.export()
    assert np.array_equal(atoms[0], ref["i"]) and np.array_equal(atoms[1], ref["j"])
    out = cf.compute(nb, tpos, x).clone()
    gx, gp = [t.clone() for t in cf.backprop(nb, tpos, x, gy)]
    sec = [t.clone() for t in cf.double_backward(nb, tpos, x, gy, V, Q)]
    again = [cf.compute(nb, tpos, x), *cf.backprop(nb, tpos, x, gy), *cf.double_backward(nb, tpos, x, gy, V, Q)]
    torch.cuda.synchronize()
    for a, b in zip([out, gx, gp] + sec, again):
        assert _same_bits(a, b), "two calls give different bits"
    e1 = _check_first(tag, out, gx, gp, ref)
    e2 = _check_second(sec, ref, family)
    assert not out[0].any() if tag == "ragged" else True                    # the single atom: exact zeros
    # the same molecules one by one: handles of the molecule's size (first, middle and last molecules; every one of the ragged frame)
    segs = batch.segments(offsets)
    picked = segs if tag == "ragged" else [segs[0], segs[31], segs[63]]
    same = True
    for lo, hi in picked:
        if hi - lo < 2:
            continue
        one, cf1 = _list(hi - lo, cutoff), _conv(tag, W, G, act, n=hi - lo)
        p1, x1, g1, V1, Q1 = (t[lo:hi].contiguous() for t in (tpos, x, gy, V, Q))
        one.build(p1)
        loop = [cf1.compute(one, p1, x1).clone(), *[t.clone() for t in cf1.backprop(one, p1, x1, g1)], *cf1.double_backward(one, p1, x1, g1, V1, Q1)]
        sub = {k: v[lo:hi] for k, v in ref.items() if k not in ("i", "j")}
        if np.abs(sub["out"]).max() > 0:
            _check_first(tag, *loop[:3], sub)
            _check_second(loop[3:], sub, family)
        same = same and all(_same_bits(a[lo:hi], b) for a, b in zip([out, gx, gp] + sec, loop))
    print(f"\n[cfconv-batch] {name} W={W} G={G} {act} {tag}: out {e1[0]:.2e} gx {e1[1]:.2e} gp {e1[2]:.2e} | dM/dg {e2[0]:.2e} dM/dx {e2[1]:.2e} "
          f"dM/dpos {e2[2]:.2e} of max; batch and loop {'agree bit for bit' if same else 'differ in their bits'}")


# ---------------------------------------------------------------------------------------------- isolation, bit for bit
ISOLATION = ["split-registers-ssp", "vector"]


def _run(nb, cf, pos, x, gy, V, Q):
    tpos, tx, tg, tV, tQ = _dev(pos, x, gy, V, Q)
    nb.build(tpos)
    res = [cf.compute(nb, tpos, tx).clone(), *[t.clone() for t in cf.backprop(nb, tpos, tx, tg)],
           *[t.clone() for t in cf.double_backward(nb, tpos, tx, tg, tV, tQ)]]
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", ISOLATION)
def test_a_molecule_does_not_feel_the_others_coordinates(name):
    """every other molecule replaced by another conformer, then by NaN: output, input gradient, forces and second derivatives of the
    molecule keep their bits"""
    family, W, G, act, _ = LAYERS[name]
    pos, offsets, cutoff = batch.batch_frame("ragged")
    other = batch.batch_frame("ragged_other")[0]
    x, gy, V, Q = batch.batch_layer("ragged", W, G)[4:]
    nb, cf = _list(len(pos), cutoff, offsets), _conv("ragged", W, G, act)
    base = _run(nb, cf, pos, x, gy, V, Q)
    for keep in (2, 3, 4):                                   # the 21-, 64- and 65-atom molecules
        lo, hi = batch.segments(offsets)[keep]
        moved = other.copy(); moved[lo:hi] = pos[lo:hi]
        got = _run(nb, cf, moved, x, gy, V, Q)
        for a, b in zip(base, got):
            assert _same_bits(a[lo:hi], b[lo:hi])
        assert not _same_bits(base[0][hi:], got[0][hi:])     # (the others did move)
        # NaN coordinates in the molecule in front of it and the one behind it
        poisoned = pos.copy()
        for m in (keep - 1, keep + 1):
            plo, phi = batch.segments(offsets)[m]
            poisoned[plo:phi] = np.nan
        got = _run(nb, cf, poisoned, x, gy, V, Q)
        for a, b in zip(base, got):
            assert _same_bits(a[lo:hi], b[lo:hi])
            assert bool(torch.isfinite(b[lo:hi]).all())
        # the poisoned molecules give what a list of their own gives on the same coordinates (no distance to NaN is below the
        # cutoff: empty rows), and nothing of theirs is written outside their rows
        plo, phi = batch.segments(offsets)[keep + 1]
        one, cf1 = _list(phi - plo, cutoff), _conv("ragged", W, G, act, n=phi - plo)
        alone = _run(one, cf1, poisoned[plo:phi], x[plo:phi], gy[plo:phi], V[plo:phi], Q[plo:phi])
        for a, b in zip(got, alone):
            assert _same_bits(a[plo:phi], b)
        untouched = np.ones(len(pos), bool)
        for m in (keep - 1, keep + 1):
            plo, phi = batch.segments(offsets)[m]
            untouched[plo:phi] = False
        for a, b in zip(base, got):
            assert np.array_equal(_bits(a)[untouched], _bits(b)[untouched])


@pytest.mark.parametrize("name", ISOLATION)
def test_permuting_the_molecules_permutes_the_results(name):
    family, W, G, act, _ = LAYERS[name]
    pos, offsets, cutoff = batch.batch_frame("ragged")
    x, gy, V, Q = batch.batch_layer("ragged", W, G)[4:]
    segs = batch.segments(offsets)
    order = [4, 0, 5, 3, 1, 2]
    rows = np.concatenate([np.arange(*segs[m]) for m in order])
    new_offsets = np.concatenate([[0], np.cumsum([segs[m][1] - segs[m][0] for m in order])]).astype(np.int32)
    cf = _conv("ragged", W, G, act)
    base = _run(_list(len(pos), cutoff, offsets), cf, pos, x, gy, V, Q)
    got = _run(_list(len(pos), cutoff, new_offsets), cf, pos[rows], x[rows], gy[rows], V[rows], Q[rows])
    for a, b in zip(base, got):
        assert _same_bits(a[torch.tensor(rows, device=DEV)], b)


# ---------------------------------------------------------------------------------------------- the C ABI's refusals
def test_c_abi_refusals_and_the_way_back():
    from nnpops_amd.capi import CFConvNeighbors, NNPOpsHipError
    pos, offsets, cutoff = batch.batch_frame("ragged")
    n = len(pos)
    tpos, = _dev(pos)
    nb = _list(n, cutoff)
    with pytest.raises(NNPOpsHipError, match="start at 0 and end at num_atoms"):
        nb.set_molecules([1, 50, n])
    with pytest.raises(NNPOpsHipError, match="start at 0 and end at num_atoms"):
        nb.set_molecules([0, 50, n - 1])
    with pytest.raises(NNPOpsHipError, match="empty or offsets are not increasing"):
        nb.set_molecules([0, 50, 50, n])                     # an empty molecule
    with pytest.raises(NNPOpsHipError, match="empty or offsets are not increasing"):
        nb.set_molecules([0, 90, 50, n])
    with pytest.raises(NNPOpsHipError, match="empty or offsets are not increasing"):
        nb.set_molecules([0, n + 5, n])                      # (never indexes beyond the table)
    with pytest.raises(NNPOpsHipError, match="non-periodic"):
        CFConvNeighbors(n, cutoff, True).set_molecules(offsets)
    # a refused call changed nothing: the list is still the single system's
    nb.build(tpos)
    fresh = _list(n, cutoff)
    fresh.build(tpos)
    single, single_d = fresh.export()
    atoms, dist = nb.export()
    assert np.array_equal(atoms, single) and np.array_equal(dist.view(np.int32), single_d.view(np.int32))
    # molecules: the current build is invalidated, a box is refused
    assert nb.build_count() > 0
    nb.set_molecules(offsets)
    assert nb.build_count() == 0
    with pytest.raises(NNPOpsHipError, match="has not been built"):
        _conv("ragged", 20, 10, "ssp").compute(nb, tpos, _dev(batch.batch_layer("ragged", 20, 10)[4])[0])
    with pytest.raises(NNPOpsHipError, match="no box vectors"):
        nb.build(tpos, _dev(batch.FAR_BOX)[0])
    nb.build(tpos)
    assert nb.num_pairs() == len(batch.half_pairs(pos, offsets, cutoff)[0]) < single.shape[1]
    # ... and back: set_molecules(0) restores the single-system list
    nb.set_molecules(None)
    assert nb.build_count() == 0
    nb.build(tpos)
    atoms, dist = nb.export()
    assert np.array_equal(atoms, single) and np.array_equal(dist.view(np.int32), single_d.view(np.int32))
    # the box gradient refuses a batched list as any non-periodic one
    nb.set_molecules(offsets)
    nb.build(tpos)
    W, G = 20, 10
    x, gy = _dev(*batch.batch_layer("ragged", W, G)[4:6])
    with pytest.raises(NNPOpsHipError, match="periodic neighbour list"):
        _conv("ragged", W, G, "ssp").backprop_box(nb, tpos, x, gy, _dev(batch.FAR_BOX)[0])


# ---------------------------------------------------------------------------------------------- the torch surface
def _modules(W, G, act, twice, offsets):
    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    la, lb = weights(W, G, 1, 41)[:4], weights(W, G, 1, 42)[:4]
    as_module = lambda w1, b1, w2, b2: CFConv(sigma_of(G), act, torch.tensor(w1).reshape(G, W), torch.tensor(b1), torch.tensor(w2),
                                              torch.tensor(b2), twice_differentiable=twice)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.neighbors = CFConvNeighbors(batch.CUTOFF)
            self.linear = torch.nn.Linear(W, W, bias=False)
            self.conv1 = as_module(*la)
            self.conv2 = as_module(*lb)

        def forward(self, positions: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
            self.neighbors.build(positions)
            h = self.conv1(self.neighbors, positions, self.linear(x))
            return self.conv2(self.neighbors, positions, 0.1 * h)

    torch.manual_seed(5)
    model = Model().to(DEV)
    model.neighbors.set_molecules([int(v) for v in offsets])
    return model, (la, lb)


@pytest.mark.parametrize("name", ["split-registers-ssp", "vector"])
def test_module_forward_and_backward_against_float64(name):
    from NNPOps.CFConv import CFConv
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    family, W, G, act, _ = LAYERS[name]
    tag = "ragged"
    pos, offsets, cutoff = batch.batch_frame(tag)
    ref = batch.reference(tag, W, G, act)
    w1, b1, w2, b2, x, gy = batch.batch_layer(tag, W, G)[:6]
    nb = CFConvNeighbors(cutoff)
    nb.set_molecules([int(v) for v in offsets])
    # (the module takes weights1 as [G][W] and hands the buffer on as the core's [W][G]: a reshape, not a transpose)
    conv = CFConv(sigma_of(G), act, torch.tensor(w1).reshape(G, W), torch.tensor(b1), torch.tensor(w2), torch.tensor(b2))
    tpos, tx = (t.requires_grad_(True) for t in _dev(pos, x))
    tg, = _dev(gy)
    nb.build(tpos)
    out = conv(nb, tpos, tx)
    (out * tg).sum().backward()
    _check_first(tag, out.detach(), tx.grad, tpos.grad, ref)


@pytest.mark.parametrize("name", ["split-registers-ssp", "vector"])
def test_force_loss_step_on_a_batch_against_float64(name):
    """two stacked twice-differentiable layers behind a linear layer, one batched list: the gradients of a force loss against the SUM
    of the same step molecule by molecule in float64"""
    family, W, G, act, _ = LAYERS[name]
    tag = "ragged"
    pos, offsets, cutoff = batch.batch_frame(tag)
    _, _, _, _, x, gy, _, Q = batch.batch_layer(tag, W, G)
    readout, f_ref = (0.1 * gy).astype(np.float32), (0.1 * Q).astype(np.float32)
    model, (la, lb) = _modules(W, G, act, True, offsets)
    tpos, tx = (t.requires_grad_(True) for t in _dev(pos, x))
    tr, tf = _dev(readout, f_ref)

    def step(m):
        energy = (m(tpos, tx) * tr).sum()
        force, = torch.autograd.grad(energy, tpos, create_graph=True)
        return torch.autograd.grad(((force - tf) ** 2).sum(), [m.linear.weight, tpos, tx]), force.detach()

    (gw, gp, gx), force = step(model)
    # float64, molecule by molecule
    wide = lambda a: torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))
    w = wide(model.linear.weight.detach().cpu().numpy()).requires_grad_(True)
    j1, j2 = Restatement(W, G, cutoff, sigma_of(G), act, *la), Restatement(W, G, cutoff, sigma_of(G), act, *lb)
    rw, rp, rx, rf = torch.zeros_like(w), torch.zeros(len(pos), 3, dtype=torch.float64), torch.zeros(len(pos), W, dtype=torch.float64), \
        torch.zeros(len(pos), 3, dtype=torch.float64)
    for lo, hi in batch.segments(offsets):
        so1 = SecondOrder.open(j1, pos[lo:hi])
        if len(so1.i) == 0:
            continue                                         # no pair: no energy, no force; its share of the loss is constant
        so2 = SecondOrder(j2, so1.i, so1.j, so1.shift)
        p, xin = wide(pos[lo:hi]).requires_grad_(True), wide(x[lo:hi]).requires_grad_(True)
        energy = (so2.forward(p, 0.1 * so1.forward(p, xin @ w.T)) * wide(readout[lo:hi])).sum()
        f64, = torch.autograd.grad(energy, p, create_graph=True)
        dw, dp, dx = torch.autograd.grad(((f64 - wide(f_ref[lo:hi])) ** 2).sum(), [w, p, xin])
        rw += dw; rp[lo:hi] = dp; rx[lo:hi] = dx; rf[lo:hi] = f64.detach()
    rel = lambda got, ref: float((got.double().cpu() - ref).abs().max() / ref.abs().max())
    e_f, e_w, e_p, e_x = rel(force, rf), rel(gw, rw), rel(gp, rp), rel(gx, rx)
    print(f"\n[cfconv-batch] force-loss step {name}: force {e_f:.2e}, d/dweight {e_w:.2e}, d/dpositions {e_p:.2e}, d/dinput {e_x:.2e} of max")
    assert float(rw.abs().max()) > 0 and float(rp.abs().max()) > 0
    assert max(e_w, e_p, e_x) <= STEP_BAR[family]


def test_torch_refusals():
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    _, W, G, act, _ = LAYERS["vector"]
    pos, offsets, cutoff = batch.batch_frame("ragged")
    x = batch.batch_layer("ragged", W, G)[4]
    tpos, tx, tbox = _dev(pos, x, batch.FAR_BOX)
    for twice in (False, True):
        model, _ = _modules(W, G, act, twice, offsets)
        with pytest.raises(RuntimeError, match="batched molecules"):
            model.neighbors.build(tpos, tbox)
        with pytest.raises(RuntimeError, match="batched molecules"):
            model.neighbors.holder.build_periodic(tpos, tbox)
        model.neighbors.build(tpos)
        with pytest.raises(RuntimeError, match="batched molecules"):
            model.conv1(model.neighbors, tpos, tx, tbox)                   # operation_periodic / operation_periodic_twice
        assert bool(torch.isfinite(model(tpos, tx)).all())                  # ... and the modules are still good
    nb = CFConvNeighbors(cutoff)
    nb.set_molecules([0, 100, 161])                                         # offsets that do not fit the positions: refused at the first build
    with pytest.raises(RuntimeError, match="start at 0 and end at num_atoms"):
        nb.build(tpos)
    nb.set_molecules([int(v) for v in offsets])
    nb.build(tpos)
    periodic = CFConvNeighbors(cutoff)
    periodic.build(tpos, tbox)
    with pytest.raises(RuntimeError, match="non-periodic"):
        periodic.set_molecules([int(v) for v in offsets])


def test_scripted_saved_and_reloaded_module_still_batches(tmp_path):
    from NNPOps.CFConvNeighbors import CFConvNeighbors
    _, W, G, act, _ = LAYERS["vector"]
    tag = "ragged"
    pos, offsets, cutoff = batch.batch_frame(tag)
    nb = CFConvNeighbors(cutoff)
    nb.set_molecules([int(v) for v in offsets])
    path = str(tmp_path / "neighbors.pt")
    torch.jit.script(nb).save(path)
    loaded = torch.jit.load(path)
    assert loaded.holder.molecules() == []
    tpos, tx = _dev(pos, batch.batch_layer(tag, W, G)[4])
    loaded.build(tpos)
    assert loaded.holder.molecules() == [int(v) for v in offsets]
    nb.build(tpos)
    model, _ = _modules(W, G, act, False, offsets)
    a = torch.ops.NNPOpsCFConv.operation(model.conv1.holder, loaded.holder, tpos, tx)
    b = torch.ops.NNPOpsCFConv.operation(model.conv1.holder, nb.holder, tpos, tx)
    assert _same_bits(a, b) and not a[0].any() and bool(a[1:].abs().sum() > 0)          # (the lone atom: an empty row)
    # the batched result is not the single-system one
    single = CFConvNeighbors(cutoff)
    single.build(tpos)
    c = torch.ops.NNPOpsCFConv.operation(model.conv1.holder, single.holder, tpos, tx)
    assert float((a - c).abs().max()) > 1e-3 * float(a.abs().max())


def test_build_and_convolution_replay_in_a_captured_graph():
    """build + two convolutions + backward captured after eager steps, replayed on new coordinates: the eager result, bit for bit"""
    _, W, G, act, _ = LAYERS["split-registers-ssp"]
    tag = "frames64"
    pos, offsets, cutoff = batch.batch_frame(tag)
    _, _, _, _, x, gy, _, _ = batch.batch_layer(tag, W, G)
    model, _ = _modules(W, G, act, False, offsets)
    static_pos, static_x = (t.requires_grad_(True) for t in _dev(pos, x))
    tr, = _dev((0.1 * gy).astype(np.float32))

    def step(p, xin):
        out = model(p, xin)
        return (out,) + torch.autograd.grad((out * tr).sum(), [p, xin])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step(static_pos, static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out, g_pos, g_x = step(static_pos, static_x)
    rng = np.random.default_rng(1)
    for _ in range(2):
        new_pos = (pos + rng.normal(0, 0.05, pos.shape)).astype(np.float32)
        with torch.no_grad():
            static_pos.copy_(torch.tensor(new_pos, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        e_out, e_pos, e_x = step(static_pos.detach().clone().requires_grad_(True), static_x.detach().clone().requires_grad_(True))
        assert _same_bits(g_out, e_out) and _same_bits(g_pos, e_pos) and _same_bits(g_x, e_x)
        assert float(e_pos.abs().max()) > 0
