#!/usr/bin/env python3
"""Generate reciprocal-space PME golden vectors from the REFERENCE's own CPU op.

Authoring container only (needs the reference checkout; compiles src/pytorch/pme/{pme,pmeCPU}.cpp against the installed libtorch
under /tmp through make_golden_pme.load_reference -- nothing of the reference is written into this repository):

    python tests/golden/make_golden_pme_recip.py

Output: tests/golden/pme_recip_ref.npz.  For each case the inputs (positions, charges, box, grid, order, alpha, coulomb), the
B-spline moduli the reference's PME class computes for that grid and order, and the outputs of torch.ops.pme.pme_reciprocal with
its autograd: energy (without the self energy), dE/dpositions, dE/dcharges.  Cases 0-2 are the three systems of the reference's
own test (src/pytorch/pme/TestPme.py:17-170: rectangular, triclinic, triclinic with exclusions -- exclusions do not change the
reciprocal term); their OpenMM totals of the reciprocal term (with the self energy) are recorded alongside.  The rest: seeded
random systems at orders 4 and 5, odd and non-power-of-two grids, a grid smaller than the order along one axis, positions several
boxes outside the cell and atoms on a cell face, and zero atoms.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_pme as direct  # noqa: E402

R = direct.R


def reference_moduli(gx, gy, gz, order):
    """The moduli of the reference's PME class (src/pytorch/pme/pme.py), computed by that class itself."""
    pkg = types.ModuleType("_refpme")
    pkg.__path__ = []
    nb = types.ModuleType("_refpme.neighbors")
    nb.getNeighborPairs = None
    sub = types.ModuleType("_refpme.pme")
    sub.__path__ = []
    sys.modules.update({"_refpme": pkg, "_refpme.neighbors": nb, "_refpme.pme": sub})
    spec = importlib.util.spec_from_file_location("_refpme.pme.pme", f"{R}/pytorch/pme/pme.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pme = mod.PME(gx, gy, gz, order, 1.0, 1.0, torch.zeros(0, 0, dtype=torch.int32))
    return [m.numpy().astype(np.float32) for m in pme.moduli]


def run(pos, charges, box, grid, order, alpha, coulomb, openmm_total=None):
    gx, gy, gz = grid
    xm, ym, zm = reference_moduli(gx, gy, gz, order)
    positions = torch.tensor(np.asarray(pos, np.float32).reshape(-1, 3), requires_grad=True)
    q = torch.tensor(np.asarray(charges, np.float32), requires_grad=True)
    tb = torch.tensor(np.asarray(box, np.float32))
    e = torch.ops.pme.pme_reciprocal(positions, q, tb, gx, gy, gz, order, alpha, coulomb, torch.tensor(xm), torch.tensor(ym),
                                     torch.tensor(zm))
    if positions.shape[0] > 0:
        e.backward()
        pg, qg = positions.grad.numpy(), q.grad.numpy()
    else:
        pg, qg = np.zeros((0, 3), np.float32), np.zeros((0,), np.float32)
    return {"positions": positions.detach().numpy(), "charges": q.detach().numpy(), "box": tb.numpy(),
            "grid": np.array(grid, np.int64), "order": np.int64(order), "alpha": np.float64(alpha), "coulomb": np.float64(coulomb),
            "xmoduli": xm, "ymoduli": ym, "zmoduli": zm, "energy": np.float64(e.item()), "pos_grad": pg, "charge_grad": qg,
            "openmm_total": np.float64(np.nan if openmm_total is None else openmm_total)}


def random_case(rng, n, grid, order, triclinic=True, spread=1.5, alpha=3.2):
    L = 2.4
    box = np.array([[L, 0, 0], [0.2 * L, 1.05 * L, 0], [-0.1 * L, 0.15 * L, 0.95 * L]]) if triclinic else np.diag([L, 1.1 * L, 0.9 * L])
    pos = rng.random((n, 3)) * L * spread - 0.3 * spread
    charges = rng.normal(0, 0.4, n)
    return run(pos, charges, box, grid, order, alpha, 138.935)


def main():
    direct.load_reference()
    q9 = [(i - 4) * 0.1 for i in range(9)]
    rect = [[1, 0, 0], [0, 1.1, 0], [0, 0, 1.2]]
    tric = [[1, 0, 0], [-0.1, 1.2, 0], [0.2, -0.15, 1.1]]
    cases = [run(direct.POS_RECT, q9, rect, (14, 15, 16), 5, 4.985823141035867, 138.935, -90.92361028496651),
             run(direct.POS_TRIC, q9, tric, (14, 16, 15), 5, 5.0, 138.935, -200.9420623172533),
             run(direct.POS_TRIC, q9, tric, (14, 16, 15), 5, 5.0, 138.935, -200.9420623172533)]
    rng = np.random.default_rng(23)
    cases += [random_case(rng, 200, (16, 16, 16), 4),                   # order 4, power-of-two grid
              random_case(rng, 200, (20, 18, 24), 5, triclinic=False),  # order 5, rectangular
              random_case(rng, 300, (13, 17, 11), 4),                   # odd grids
              random_case(rng, 300, (21, 9, 25), 5),                    # odd, non-power-of-two
              random_case(rng, 100, (12, 3, 14), 5),                    # grid smaller than the order along y
              random_case(rng, 100, (4, 10, 2), 4),                     # ... and along x (== order) and z
              random_case(rng, 150, (16, 20, 18), 5, spread=6.0)]       # positions several boxes outside the cell
    # atoms on cell faces and corners (fractional coordinates 0 and 1 exactly)
    L = 2.4
    face = np.array([[0, 0, 0], [L, 0.3, 0.7], [0.5, 1.1 * L, 0.2], [0.9, 0.4, 0.9 * L], [L, 1.1 * L, 0.9 * L], [-L, 0.5, 0.5]])
    cases.append(run(face, [0.3, -0.2, 0.5, -0.4, 0.1, -0.3], np.diag([L, 1.1 * L, 0.9 * L]), (16, 16, 16), 5, 3.2, 138.935))
    cases.append(run(np.zeros((0, 3)), np.zeros(0), rect, (14, 15, 16), 5, 4.985823141035867, 138.935))   # zero atoms
    out = {"num_cases": np.int64(len(cases))}
    for k, c in enumerate(cases):
        for name, v in c.items():
            out[f"c{k}_{name}"] = v
    np.savez_compressed(os.path.join(HERE, "pme_recip_ref.npz"), **out)
    print("pme_recip_ref.npz:", [round(float(c["energy"]), 4) for c in cases])


if __name__ == "__main__":
    main()
