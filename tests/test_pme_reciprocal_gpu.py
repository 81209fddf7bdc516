"""Reciprocal-space PME on the MI355X: torch.ops.pme.pme_reciprocal and capi.pme_reciprocal against the reference-made vectors
(tests/golden/pme_recip_ref.npz), bitwise repeatability, an independent float64 Ewald sum, graph capture and the device's limits."""
import math

import numpy as np
import pytest
import torch

import NNPOps  # noqa: F401  (loads the torch ops)
from nnpops_amd import workloads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cases(golden_dir):
    g = np.load(f"{golden_dir}/pme_recip_ref.npz")
    for k in range(int(g["num_cases"])):
        yield k, {name[len(f"c{k}_"):]: g[name] for name in g.files if name.startswith(f"c{k}_")}


def _args(c, device=DEV):
    gx, gy, gz = (int(v) for v in c["grid"])
    mods = [torch.tensor(c[n], device=device) for n in ("xmoduli", "ymoduli", "zmoduli")]
    return torch.tensor(c["box"], device=device), gx, gy, gz, int(c["order"]), float(c["alpha"]), float(c["coulomb"]), mods


def _run(c, pos=None, q=None, device=DEV):
    box, gx, gy, gz, order, alpha, coulomb, mods = _args(c, device)
    pos = torch.tensor(c["positions"], device=device) if pos is None else pos
    q = torch.tensor(c["charges"], device=device) if q is None else q
    pos = pos.detach().clone().requires_grad_()
    q = q.detach().clone().requires_grad_()
    e = torch.ops.pme.pme_reciprocal(pos, q, box, gx, gy, gz, order, alpha, coulomb, *mods)
    if pos.shape[0]:
        e.backward()
        return e.detach(), pos.grad, q.grad
    return e.detach(), torch.zeros(0, 3, device=device), torch.zeros(0, device=device)


def _close(k, c, e, pg, cg):
    ref = float(c["energy"])
    assert abs(float(e) - ref) <= 1e-5 * max(abs(ref), 1.0), (k, float(e), ref)
    if len(c["positions"]):
        np.testing.assert_allclose(pg, c["pos_grad"], rtol=0, atol=1e-4 * np.abs(c["pos_grad"]).max(), err_msg=str(k))
        np.testing.assert_allclose(cg, c["charge_grad"], rtol=0, atol=1e-4 * np.abs(c["charge_grad"]).max(), err_msg=str(k))


def test_torch_op_matches_the_reference_op(golden_dir):
    orders = set()
    for k, c in _cases(golden_dir):
        e, pg, cg = _run(c)
        assert e.dim() == 0 and e.device.type == "cuda"
        _close(k, c, e.cpu(), pg.cpu().numpy(), cg.cpu().numpy())
        orders.add(int(c["order"]))
    assert orders == {4, 5}


def test_c_abi_matches_the_reference_op(golden_dir):
    from nnpops_amd import capi
    for k, c in _cases(golden_dir):
        box, gx, gy, gz, order, alpha, coulomb, mods = _args(c)
        e, pg, cg = capi.pme_reciprocal(torch.tensor(c["positions"], device=DEV), torch.tensor(c["charges"], device=DEV), box, gx, gy,
                                        gz, order, alpha, coulomb, *mods)
        torch.cuda.synchronize()
        _close(k, c, e.cpu()[0], pg.cpu().numpy(), cg.cpu().numpy())


def test_reference_test_energies_through_the_class(golden_dir):
    from NNPOps.pme import PME
    for k, c in _cases(golden_dir):
        if not np.isfinite(c["openmm_total"]):
            continue
        box, gx, gy, gz, order, alpha, coulomb, _ = _args(c)
        pme = PME(gx, gy, gz, order, alpha, coulomb, torch.zeros(9, 0, dtype=torch.int32), reciprocal=True)
        e = pme.compute_reciprocal(torch.tensor(c["positions"], device=DEV), torch.tensor(c["charges"], device=DEV), box)
        assert np.allclose(float(c["openmm_total"]), float(e), rtol=1e-5), (k, float(e))


def test_bitwise_repeatable(golden_dir):
    for k, c in _cases(golden_dir):
        a = _run(c)
        b = _run(c)
        for x, y in zip(a, b):
            assert torch.equal(x, y), k


def test_atom_permutation(golden_dir):
    c = next(c for k, c in _cases(golden_dir) if k == 6)
    n = len(c["positions"])
    perm = np.random.default_rng(5).permutation(n)
    e0, pg0, cg0 = _run(c)
    p = dict(c, positions=c["positions"][perm], charges=c["charges"][perm])
    e1, pg1, cg1 = _run(p)
    assert abs(float(e1) - float(e0)) <= 2e-6 * abs(float(e0))
    scale = float(pg0.abs().max())
    torch.testing.assert_close(pg1, pg0[torch.tensor(perm, device=DEV)], rtol=0, atol=1e-5 * scale)
    torch.testing.assert_close(cg1, cg0[torch.tensor(perm, device=DEV)], rtol=0, atol=1e-5 * float(cg0.abs().max()))


# ---- an independent float64 Ewald sum (no PME, no grid) -------------------------------------------------------------------
def ewald_kspace(pos, q, box, alpha, coulomb):
    """1/(2 pi V) coulomb sum_{m != 0} exp(-pi^2 m^2 / alpha^2) / m^2 |S(m)|^2 and its derivatives, float64."""
    pos, q, box = np.asarray(pos, np.float64), np.asarray(q, np.float64), np.asarray(box, np.float64)
    recip = np.linalg.inv(box).T                                     # rows: a*, b*, c*
    V = abs(np.linalg.det(box))
    mmax = 8.0 * alpha / np.pi                                       # exp(-pi^2 m^2 / alpha^2) < 1e-27 beyond
    kmax = [int(np.ceil(mmax * np.linalg.norm(box[i]))) + 1 for i in range(3)]     # |k_i| = |m . box_i| <= |m| |box_i|
    ks = np.stack(np.meshgrid(*[np.arange(-k, k + 1) for k in kmax], indexing="ij"), -1).reshape(-1, 3)
    ks = ks[np.any(ks != 0, axis=1)]
    m = ks @ recip
    m2 = (m * m).sum(1)
    keep = m2 <= mmax * mmax
    m, m2 = m[keep], m2[keep]
    f = np.exp(-np.pi ** 2 * m2 / alpha ** 2) / m2
    phase = np.exp(2j * np.pi * (pos @ m.T))                         # [atoms, k]
    S = q @ phase
    pref = coulomb / (2 * np.pi * V)
    e = pref * np.sum(f * np.abs(S) ** 2)
    dq = pref * 2 * np.real(np.conj(S)[None, :] * phase) @ f
    dpos = pref * (2 * np.real(np.conj(S)[None, :] * q[:, None] * 2j * np.pi * phase) * f[None, :]) @ m
    return e, dpos, dq


def ewald_direct(pos, q, box, alpha, coulomb, images=2):
    """Real-space Ewald sum over periodic images (no cutoff), float64."""
    from math import erfc
    pos, q, box = np.asarray(pos, np.float64), np.asarray(q, np.float64), np.asarray(box, np.float64)
    n = len(q)
    e = 0.0
    rng = range(-images, images + 1)
    shifts = np.array([[a, b, c] for a in rng for b in rng for c in rng], np.float64) @ box
    for i in range(n):
        d = pos[i] - pos                                             # [n, 3]
        for s in shifts:
            r = np.linalg.norm(d + s, axis=1)
            same = r < 1e-12
            r[same] = 1.0
            t = np.array([erfc(alpha * x) for x in r]) / r
            t[same] = 0.0
            e += 0.5 * coulomb * q[i] * np.sum(q * t)
    return e


def _system(triclinic, n=24, seed=3):
    rng = np.random.default_rng(seed)
    L = 2.0
    box = np.array([[L, 0, 0], [0.25 * L, 1.05 * L, 0], [-0.2 * L, 0.1 * L, 0.95 * L]]) if triclinic else np.diag([L, 1.1 * L, 0.9 * L])
    pos = rng.random((n, 3)) @ box
    q = rng.normal(0, 0.5, n)
    q -= q.mean()                                                    # neutral: the total Ewald energy needs no background term
    return pos.astype(np.float32), q.astype(np.float32), box.astype(np.float32)


@pytest.mark.parametrize("triclinic", [False, True])
def test_against_an_independent_ewald_sum(triclinic):
    from NNPOps.pme import PME
    pos, q, box = _system(triclinic)
    alpha, coulomb = 4.0, 138.935
    e_ref, dpos_ref, dq_ref = ewald_kspace(pos, q, box, alpha, coulomb)
    errs = []
    for grid in (12, 24, 64):
        pme = PME(grid, grid, grid, 5, alpha, coulomb, torch.zeros(len(q), 0, dtype=torch.int32), reciprocal=True)
        tp = torch.tensor(pos, device=DEV, requires_grad=True)
        tq = torch.tensor(q, device=DEV, requires_grad=True)
        tb = torch.tensor(box, device=DEV)
        self_energy = -coulomb * alpha / math.sqrt(math.pi) * float(np.sum(q.astype(np.float64) ** 2))
        erecip = pme.compute_reciprocal(tp, tq, tb)
        erecip.backward()
        errs.append(abs(float(erecip) - self_energy - e_ref) / abs(e_ref))
    assert errs[2] < 1e-4 and errs[0] > errs[2], errs
    np.testing.assert_allclose(tp.grad.cpu().numpy(), dpos_ref, rtol=0, atol=1e-3 * np.abs(dpos_ref).max())
    self_dq = -2 * coulomb * alpha / math.sqrt(math.pi) * q.astype(np.float64)
    np.testing.assert_allclose(tq.grad.cpu().numpy(), dq_ref + self_dq, rtol=0, atol=1e-3 * np.abs(dq_ref + self_dq).max())
    # direct + reciprocal + self == the full Ewald sum (the cutoff at half the box: erfc(alpha rc) ~ 1e-6)
    edir = pme.compute_direct(tp.detach(), tq.detach(), 0.85, tb)
    total = float(edir) + float(erecip)
    full = ewald_direct(pos, q, box, alpha, coulomb) + e_ref + self_energy
    assert abs(total - full) <= 2e-4 * max(abs(full), 1.0), (total, full)


def test_large_system_against_the_cpu_key():
    pos, _, box = workloads.random_box(20000, density=0.1, seed=8)
    rng = np.random.default_rng(8)
    q = rng.normal(0, 0.4, len(pos)).astype(np.float32)
    from nnpops_amd.pme.pme import bspline_moduli
    mods = [bspline_moduli(64, 5)] * 3
    out = []
    for dev in ("cpu", DEV):
        tp = torch.tensor(pos, device=dev, requires_grad=True)
        tq = torch.tensor(q, device=dev, requires_grad=True)
        e = torch.ops.pme.pme_reciprocal(tp, tq, torch.tensor(box, device=dev), 64, 64, 64, 5, 0.6, 138.935, *[m.to(dev) for m in mods])
        e.backward()
        out.append((float(e), tp.grad.cpu().numpy(), tq.grad.cpu().numpy()))
    (e0, p0, q0), (e1, p1, q1) = out
    assert abs(e1 - e0) <= 1e-5 * abs(e0)
    np.testing.assert_allclose(p1, p0, rtol=0, atol=1e-5 * np.abs(p0).max())
    np.testing.assert_allclose(q1, q0, rtol=0, atol=1e-5 * np.abs(q0).max())


def test_side_stream(golden_dir):
    c = next(c for k, c in _cases(golden_dir) if k == 5)
    ref = _run(c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = _run(c)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for x, y in zip(ref, got):
        assert torch.equal(x, y)


def test_direct_plus_reciprocal_replay_as_a_hip_graph(golden_dir):
    """compute_direct + compute_reciprocal + backward captured after a warm-up and replayed on moved atoms and a new box written
    in place (the reference's test_cuda_graph), compared with eager evaluation."""
    from NNPOps.pme import PME
    c = next(c for k, c in _cases(golden_dir) if k == 1)
    box, gx, gy, gz, order, alpha, coulomb, _ = _args(c)
    pme = PME(gx, gy, gz, order, alpha, coulomb, torch.zeros(9, 0, dtype=torch.int32), reciprocal=True)
    pos = torch.tensor(c["positions"], device=DEV)
    q = torch.tensor(c["charges"], device=DEV)
    static_pos = pos.clone().requires_grad_()
    static_box = box.clone()

    def step():
        e = pme.compute_direct(static_pos, q, 0.5, static_box, max_num_pairs=64) + pme.compute_reciprocal(static_pos, q, static_box)
        e.backward()
        return e

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
            static_pos.grad = None
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        e = step()
    moved = pos + 0.05
    with torch.no_grad():
        static_pos.copy_(moved)
    graph.replay()
    torch.cuda.synchronize()
    ref_pos = moved.clone().requires_grad_()
    e_ref = pme.compute_direct(ref_pos, q, 0.5, box, max_num_pairs=64) + pme.compute_reciprocal(ref_pos, q, box)
    e_ref.backward()
    assert torch.allclose(e, e_ref, rtol=1e-5, atol=1e-5) and torch.allclose(static_pos.grad, ref_pos.grad, rtol=1e-4, atol=1e-4)

    # the reciprocal term alone, replayed with a new box written into the captured tensor: the kernels read the box on the device
    rpos = pos.clone().requires_grad_()
    with torch.cuda.stream(s):
        for _ in range(2):
            pme.compute_reciprocal(rpos, q, static_box).backward()
            rpos.grad = None
    torch.cuda.current_stream().wait_stream(s)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        er = pme.compute_reciprocal(rpos, q, static_box)
        er.backward()
    new_box = box * 1.05
    with torch.no_grad():
        static_box.copy_(new_box)
    g2.replay()
    torch.cuda.synchronize()
    p3 = pos.clone().requires_grad_()
    e3 = pme.compute_reciprocal(p3, q, new_box)
    e3.backward()
    assert torch.allclose(er, e3, rtol=1e-5, atol=1e-5) and torch.allclose(rpos.grad, p3.grad, rtol=1e-4, atol=1e-4)


def test_zero_atoms_and_small_grids(golden_dir):
    seen = set()
    for k, c in _cases(golden_dir):
        if len(c["positions"]) == 0:
            seen.add("empty")
        elif min(int(v) for v in c["grid"]) < int(c["order"]):
            seen.add("small")
        else:
            continue
        _close(k, c, *[t.cpu().numpy() if t.dim() else t.cpu() for t in _run(c)])
    assert seen == {"empty", "small"}


def test_device_refuses_order_6():
    m = torch.ones(8, device=DEV)
    with pytest.raises(RuntimeError, match="Only pmeOrder 4 or 5 is supported"):
        torch.ops.pme.pme_reciprocal(torch.zeros(3, 3, device=DEV), torch.zeros(3, device=DEV), torch.eye(3, device=DEV), 8, 8, 8, 6,
                                     3.0, 1.0, m, m, m)
