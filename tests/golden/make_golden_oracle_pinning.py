#!/usr/bin/env python3
"""Store what the REFERENCE's own CPU classes compute on the seeded cases of tests/test_oracle_pinning.py.

Authoring container only (needs oracle/_ref, which __graft_entry__.build() compiles where the reference's
sources are present):

    python tests/golden/make_golden_oracle_pinning.py

The cases are the test module's own (ani_outputs / cfconv_outputs), run with RefAni / RefCFConv /
RefCFConvNeighbors.  The oracle must reproduce every array bit for bit, so each array is stored as its
dtype, shape and the SHA-256 of its bytes (test_oracle_pinning.digest): that pins the oracle wherever
the reference is absent, in a few KB instead of megabytes of AEV rows.

Output: tests/golden/oracle_pinning_ref.json
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402


def main():
    assert oracle.have_ref(), "oracle/_ref not built"
    spec = importlib.util.spec_from_file_location("pinning", os.path.join(ROOT, "tests", "test_oracle_pinning.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    out = {}
    for kind in t.ANI_KINDS:
        for torchani in (True, False):
            for name, arr in t.ani_outputs(oracle.RefAni, kind, torchani).items():
                out[f"ani_{kind}_torchani{int(torchani)}_{name}"] = t.digest(arr)
    for periodic in (False, True):
        for act in ("ssp", "tanh"):
            for k, arr in enumerate(t.cfconv_outputs(oracle.RefCFConvNeighbors, oracle.RefCFConv, periodic, act)):
                out[f"cfconv_periodic{int(periodic)}_{act}_{k}"] = t.digest(arr)
    path = os.path.join(HERE, "oracle_pinning_ref.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(out), "arrays")


if __name__ == "__main__":
    main()
