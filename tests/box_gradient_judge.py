"""What the box-gradient tests of the ANI symmetry functions and of the CFConv share (no GPU code, no tests; importable anywhere):
the moved 600-atom frames, the judgement of a box gradient against its float64 reference, and the clearing of a family's switches.
PME states its stress in its own box convention (pme_float64.virial)."""
import os

import numpy as np


def moved_frames(pos, box):
    """-> (shifted, wrapped): every atom 0.37 box lengths along x, a third of them outside the box, and those brought back by one
    box vector (other shifts, another dL/dB)"""
    shifted = (pos + np.array([0.37 * float(box[0, 0]), 0, 0], dtype=np.float32)).astype(np.float32)
    assert 0.25 < float((shifted[:, 0] > box[0, 0]).mean()) < 0.45
    wrapped = (shifted - (shifted[:, :1] > box[0, 0]) * box[0]).astype(np.float32)
    return shifted, wrapped


def judge(prefix, label, pos, box, ref, g, gbox, bar, what="box gradient"):
    """g = dL/dpositions and gbox = dL/dB (float64 arrays) against ref["g"], ref["gbox"]: the box gradient to `bar` of its largest
    entry, and the antisymmetric part of the stress W = x^T dL/dx + B^T dL/dB (rotation invariance) to `bar` of the largest entry
    of W.  Prints the measured figures first."""
    top = float(np.abs(ref["gbox"]).max())
    err = float(np.abs(gbox - ref["gbox"]).max())
    x, B = pos.astype(np.float64), box.astype(np.float64)
    W = x.T @ g + B.T @ gbox
    W_ref = x.T @ ref["g"] + B.T @ ref["gbox"]
    anti, anti_ref = float(np.abs(W - W.T).max()) / 2, float(np.abs(W_ref - W_ref.T).max()) / 2
    wtop = float(np.abs(W_ref).max())
    print(f"\n[{prefix}] {label}: {what} {err / top:.2e} of max {top:.3e}; antisymmetric stress {anti / wtop:.2e} of max {wtop:.3e} "
          f"(float64: {anti_ref / wtop:.1e}); force {np.abs(g - ref['g']).max() / np.abs(ref['g']).max():.2e}")
    assert np.isfinite(gbox).all() and top > 0 and np.abs(gbox).max() > 0
    assert err <= bar * top, (label, err, top)
    assert anti <= bar * wtop, (label, anti, wtop)


def clean_env(monkeypatch, prefix):
    for k in [k for k in os.environ if k.startswith(prefix)]:
        monkeypatch.delenv(k)
