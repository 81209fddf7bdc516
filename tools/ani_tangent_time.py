"""The AEV tangent J.v (nnpops_ani_tangent_strided) next to compute() and backprop() (C ABI), on the headline frame (10 000-atom
ANI-2x liquid) and on a batch of 64 conformers of 60 atoms behind one handle: stream time per call, interleaved rounds, medians.
The outside comparison is a float32 torch restatement of the AEV over an exported pair / triple list (index tensors on the device,
built once, not timed), differentiated forward by torch.func.jvp: what J.v costs when autograd does it.  Prints the largest
difference between the two tangents as a sanity figure, no float64 evaluation.

    python tools/ani_tangent_time.py [atoms]
    python tools/ani_tangent_time.py --profile [atoms]      (a few calls only, for rocprofv3 --kernel-trace --stats)"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnpops_amd import workloads  # noqa: E402
from nnpops_amd.capi import AniSymmetryFunctions  # noqa: E402

dev = torch.device("cuda:0")
S, RCR, RCA = 7, 5.1, 3.5
NB = S * (S + 1) // 2


def timed(fn, reps=100, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def export_lists(pos, species, box, offsets):
    """-> device index tensors of the directed radial pairs (i, j, shift) and of the triples (centre, j, k, shift_j, shift_k)"""
    n = len(pos)
    x = torch.tensor(pos, device=dev, dtype=torch.float64)
    B = None if box is None else torch.tensor(box, device=dev, dtype=torch.float64)
    mol = None if offsets is None else torch.tensor(np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)), device=dev)
    pi, pj, pn = [], [], []
    for lo in range(0, n, 1024):
        d = x[None, :, :] - x[lo:lo + 1024, None, :]
        shift = torch.zeros_like(d)
        if B is not None:                                   # (cubic boxes here: one round per axis)
            shift = -torch.round(d / torch.diagonal(B)) * torch.diagonal(B)
        r2 = ((d + shift) ** 2).sum(-1)
        near = r2 < RCR * RCR
        near[torch.arange(d.shape[0], device=dev), torch.arange(lo, lo + d.shape[0], device=dev)] = False
        if mol is not None:
            near &= mol[lo:lo + 1024, None] == mol[None, :]
        a, b = torch.nonzero(near, as_tuple=True)
        pi.append(a + lo); pj.append(b); pn.append(shift[a, b])
    pi, pj, pn = torch.cat(pi), torch.cat(pj), torch.cat(pn)
    d = x[pj] - x[pi] + pn
    ang = (d * d).sum(1) < RCA * RCA
    ai, aj, an = pi[ang].cpu().numpy(), pj[ang].cpu().numpy(), pn[ang].cpu().numpy()
    start = np.searchsorted(ai, np.arange(n + 1))
    ti, tj, tk, nj, nk = [], [], [], [], []
    for i in range(n):
        lo, hi = start[i], start[i + 1]
        if hi - lo >= 2:
            a, b = np.triu_indices(hi - lo, 1)
            ti.append(np.full(len(a), i)); tj.append(aj[lo + a]); tk.append(aj[lo + b]); nj.append(an[lo + a]); nk.append(an[lo + b])
    cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape)
    sp = torch.tensor(species, device=dev, dtype=torch.long)
    t = lambda a, dt: torch.tensor(a, device=dev, dtype=dt)
    ti, tj, tk = (t(cat(p, (0,)), torch.long) for p in (ti, tj, tk))
    lo_s, hi_s = torch.minimum(sp[tj], sp[tk]), torch.maximum(sp[tj], sp[tk])
    bucket = lo_s * S - lo_s * (lo_s - 1) // 2 + (hi_s - lo_s)
    return dict(pi=pi, pj=pj, pn=pn.float(), prow=pi * S + sp[pj], ti=ti, tj=tj, tk=tk, nj=t(cat(nj, (0, 3)), torch.float32),
                nk=t(cat(nk, (0, 3)), torch.float32), trow=ti * NB + bucket, n=n)


def torch_aev(x, L, rf, af):
    """the AEV in float32 torch over the exported lists -> (radial [N, S nR], angular [N, NB nA])"""
    d = x[L["pj"]] - x[L["pi"]] + L["pn"]
    r = d.norm(dim=1)
    sh = r[:, None] - rf[None, :, 1]
    terms = 0.25 * (0.5 * torch.cos(math.pi * r / RCR) + 0.5)[:, None] * torch.exp(-rf[None, :, 0] * sh * sh)
    radial = torch.zeros((L["n"] * S, rf.shape[0]), device=dev).index_add(0, L["prow"], terms)
    u, w = x[L["tj"]] - x[L["ti"]] + L["nj"], x[L["tk"]] - x[L["ti"]] + L["nk"]
    ru, rw = u.norm(dim=1), w.norm(dim=1)
    theta = torch.acos(0.95 * (u * w).sum(1) / (ru * rw))
    fcfc = (0.5 * torch.cos(math.pi * ru / RCA) + 0.5) * (0.5 * torch.cos(math.pi * rw / RCA) + 0.5)
    eta, rs, zeta, ths = (af[None, :, c] for c in range(4))
    sh = 0.5 * (ru + rw)[:, None] - rs
    terms = fcfc[:, None] * (1.0 + torch.cos(theta[:, None] - ths)) ** zeta * torch.exp(-eta * sh * sh) * 2.0 ** (1.0 - zeta)
    angular = torch.zeros((L["n"] * NB, af.shape[0]), device=dev).index_add(0, L["trow"], terms)
    return radial.reshape(L["n"], -1), angular.reshape(L["n"], -1)


def frame(label, pos, species, box, offsets, profile):
    rf, af = workloads.ani2x_functions()
    sym = AniSymmetryFunctions(S, RCR, RCA, species, rf, af, periodic=box is not None)
    if offsets is not None:
        sym.set_molecules(offsets)
    tpos = torch.tensor(pos, device=dev)
    tbox = None if box is None else torch.tensor(box, device=dev)
    radial, angular = sym.compute(tpos, tbox)
    gen = torch.Generator(device=dev).manual_seed(0)
    wr = torch.randn(radial.shape, device=dev, generator=gen)
    wa = torch.randn(angular.shape, device=dev, generator=gen)
    v = torch.randn(tpos.shape, device=dev, generator=gen)
    g, tr, ta = torch.empty_like(tpos), torch.empty_like(radial), torch.empty_like(angular)
    calls = dict(compute=lambda: sym.compute(tpos, tbox, radial, angular, check=False), backprop=lambda: sym.backprop(wr, wa, g),
                 tangent=lambda: sym.tangent(v, tr, ta))
    if profile:
        for _ in range(5):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        return
    L = export_lists(pos, species, box, offsets)
    trf, taf = torch.tensor(rf, device=dev), torch.tensor(af, device=dev)
    outside = lambda: torch.func.jvp(lambda x: torch_aev(x, L, trf, taf), (tpos,), (v,))[1]
    rounds = [{name: timed(fn) for name, fn in calls.items()} for _ in range(5)]      # interleaved: all see the same clocks
    t = {name: float(np.median([r[name] for r in rounds])) for name in calls}
    t_out = float(np.median([timed(outside, reps=5, warm=2) for _ in range(3)]))
    sym.compute(tpos, tbox, radial, angular, check=False)
    sym.tangent(v, tr, ta)
    jr, ja = outside()
    diff = max(float((tr - jr).abs().max() / jr.abs().max()), float((ta - ja).abs().max() / ja.abs().max()))
    what = sym.describe()
    print(f"{label}: compute {t['compute']:.1f} us, backprop {t['backprop']:.1f} us, tangent {t['tangent']:.1f} us; torch float32 jvp over "
          f"{len(L['pi'])} pairs / {len(L['ti'])} triples {t_out:.0f} us ({t_out / t['tangent']:.0f} x)  (cap_angular={what['cap_angular']} "
          f"cells={what['cells']} fused_build={what['fused_build']}; kernel vs torch float32 {diff:.1e} of max)")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    profile = "--profile" in sys.argv
    n = int(args[0]) if args else 10000
    frame(f"liquid {n}", *workloads.random_box(n, seed=1), None, profile)
    if not args:
        parts = [workloads.conformer(60, seed=200 + b) for b in range(64)]
        pos = np.concatenate([p for p, _ in parts]).astype(np.float32)
        species = np.concatenate([s for _, s in parts]).astype(np.int32)
        frame("64 conformers x 60 atoms", pos, species, None, np.arange(65, dtype=np.int32) * 60, profile)
