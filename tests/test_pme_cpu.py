"""Direct-space PME without a GPU: the numpy oracle and the op's host (CPU-tensor) path against vectors produced by the
reference's own CPU op (tests/golden/pme_ref.npz) and the OpenMM energies the reference's test holds."""
import numpy as np
import pytest
import torch

import pme_float64 as f64
from oracle import pme_direct_oracle


def _cases(golden_dir):
    g = np.load(f"{golden_dir}/pme_ref.npz")
    for k in range(int(g["num_cases"])):
        yield k, {name[len(f"c{k}_"):]: g[name] for name in g.files if name.startswith(f"c{k}_")}


def test_oracle_is_pinned_to_the_reference_op(golden_dir):
    for k, c in _cases(golden_dir):
        e, pd, cd = pme_direct_oracle(c["positions"], c["charges"], c["neighbors"], c["deltas"], c["distances"],
                                      f64.sorted_excl(c["exclusions"]), c["alpha"], c["coulomb"])
        scale = np.abs(c["pos_grad"]).max()
        assert abs(e - float(c["energy"])) <= 2e-6 * max(abs(float(c["energy"])), 1.0), k
        np.testing.assert_allclose(pd, c["pos_grad"], rtol=2e-5, atol=2e-6 * scale)
        np.testing.assert_allclose(cd, c["charge_grad"], rtol=2e-5, atol=2e-6 * np.abs(c["charge_grad"]).max())
        if np.isfinite(c["openmm_energy"]):                  # the reference test's own bar: np.allclose (rtol 1e-5, atol 1e-8)
            assert np.allclose(float(c["openmm_energy"]), e, rtol=1e-5)


def test_pme_class_on_host_tensors(golden_dir):
    """NNPOps.pme.PME.compute_direct end to end on CPU tensors: our getNeighborPairs CPU key + pme_direct host path + autograd."""
    from NNPOps.pme import PME
    for k, c in _cases(golden_dir):
        pme = PME(14, 15, 16, 5, float(c["alpha"]), float(c["coulomb"]), torch.tensor(c["exclusions"].astype(np.int32)).reshape(len(c["positions"]), -1))
        pos = torch.tensor(c["positions"], requires_grad=True)
        q = torch.tensor(c["charges"], requires_grad=True)
        e = pme.compute_direct(pos, q, float(c["cutoff"]), torch.tensor(c["box"]))
        e.backward()
        assert abs(float(e) - float(c["energy"])) <= 1e-5 * max(abs(float(c["energy"])), 1.0)
        np.testing.assert_allclose(pos.grad.numpy(), c["pos_grad"], rtol=1e-4, atol=1e-5 * np.abs(c["pos_grad"]).max())
        np.testing.assert_allclose(q.grad.numpy(), c["charge_grad"], rtol=1e-4, atol=1e-5 * np.abs(c["charge_grad"]).max())


def test_pme_argument_errors_match_the_reference():
    from NNPOps.pme import PME
    with pytest.raises(ValueError, match="alpha must be positive"):
        PME(8, 8, 8, 4, 0.0, 1.0, torch.zeros(3, 0, dtype=torch.int32))
    pme = PME(8, 8, 8, 4, 3.0, 1.0, torch.zeros(3, 0, dtype=torch.int32))
    with pytest.raises(ValueError, match="charges must be 1D"):
        pme.compute_direct(torch.zeros(3, 3), torch.zeros(3, 1), 0.4, torch.eye(3))
    with pytest.raises(ValueError, match="must all have the same length"):
        pme.compute_direct(torch.zeros(4, 3), torch.zeros(4), 0.4, torch.eye(3))
    with pytest.raises(RuntimeError, match="reciprocal-space"):
        pme.compute_reciprocal(torch.zeros(3, 3), torch.zeros(3), torch.eye(3))


def test_ops_run_below_autograd_and_validate_their_arguments(golden_dir):
    """Round-2 advisor findings: (i) getNeighborPairs / pme_direct under torch.inference_mode() (the reference registers
    them under the CPU backend key, getNeighborPairsCPU.cpp:102, pmeCPU.cpp:381); (ii) a pair list whose arrays do not match
    is refused instead of read out of bounds; (iii) a recorded backward pass (create_graph=True) is refused."""
    from NNPOps.neighbors import getNeighborPairs
    k, c = next(_cases(golden_dir))
    pos, q, box = torch.tensor(c["positions"]), torch.tensor(c["charges"]), torch.tensor(c["box"])
    excl = torch.tensor(f64.sorted_excl(c["exclusions"]).astype(np.int32)).reshape(len(c["positions"]), -1)
    with torch.inference_mode():
        nb, dl, ds, n = getNeighborPairs(pos, float(c["cutoff"]), -1, box)
        e = torch.ops.pme.pme_direct(pos, q, nb, dl, ds, excl, float(c["alpha"]), float(c["coulomb"]))
    assert abs(float(e) - float(c["energy"])) <= 1e-5 * max(abs(float(c["energy"])), 1.0)
    nb, dl, ds, n = getNeighborPairs(pos, float(c["cutoff"]), -1, box)
    with pytest.raises(RuntimeError, match="deltas must have shape"):
        torch.ops.pme.pme_direct(pos, q, nb, dl[:-1], ds, excl, 0.5, 1.0)
    with pytest.raises(RuntimeError, match="distances must have shape"):
        torch.ops.pme.pme_direct(pos, q, nb, dl, ds[:-1], excl, 0.5, 1.0)
    with pytest.raises(RuntimeError, match="integer indices"):
        torch.ops.pme.pme_direct(pos, q, nb.float(), dl, ds, excl, 0.5, 1.0)
    bad = nb.clone()
    bad[1, 0] = len(pos) + 5
    bad[0, 0] = 0
    with pytest.raises(RuntimeError, match="out of range"):
        torch.ops.pme.pme_direct(pos, q, bad, dl, ds, excl, 0.5, 1.0)
    p2 = pos.clone().requires_grad_(True)
    e = torch.ops.pme.pme_direct(p2, q, nb, dl, ds, excl, float(c["alpha"]), float(c["coulomb"]))
    torch.autograd.grad(e, p2, retain_graph=True)
    with pytest.raises(RuntimeError, match="second derivatives are not implemented"):
        torch.autograd.grad(e, p2, create_graph=True)


def test_one_sided_exclusion_table_is_refused():
    """The HIP kernel is owner-computes: every atom reads the terms of its excluded pairs from its own row, so the table must be
    symmetric (the reference documents the same requirement, pme.py:66-73).  The wrapper checks it once at construction."""
    import pytest
    import torch
    from NNPOps.pme import PME
    sym = torch.tensor([[1, -1], [0, 2], [1, -1]])
    PME(8, 8, 8, 5, 0.3, 138.9, sym)                                   # 0-1, 1-2 listed from both ends
    with pytest.raises(ValueError, match="symmetric"):
        PME(8, 8, 8, 5, 0.3, 138.9, torch.tensor([[1, -1], [-1, -1], [-1, -1]]))      # 1 in row 0, 0 not in row 1
    with pytest.raises(ValueError, match="atom indices"):
        PME(8, 8, 8, 5, 0.3, 138.9, torch.tensor([[7, -1], [-1, -1], [-1, -1]]))
