"""The float64 judge of the fused atomic networks' weight gradients UNDER A FORCE LOSS (csrc/mlp_weight_grad_tangent.h; no GPU code, no
tests; importable anywhere) and the table of cases tests/test_mlp_force_weights_gpu.py runs, so that the CPU file that pins the judge
and the GPU file that uses it see the same numbers.

The function is mlp_float64's restatement of the reference's TorchANIBatchedNN.  With g_m(a) = dE_m(a)/dx_a (a first backward pass,
recorded), a tangent row t_a per atom and the upstream weight c of every (molecule, member), the quantity is

    M = sum over the kinds, their atoms a and the members m of  c[molecule of a][m] <t_a, g_m(a)>  =  sum c E'

and the judge is dM/d(the eight arrays of every kind), and E' per (grouped atom, member):
  `autograd`     float64 autograd -- create_graph in x, then backward in the eight leaves -- (the judge), or float32 (the WITNESS: what
                 plain float32 arithmetic of the same sums loses, never a kernel);
  `closed_form`  the same numbers from the forward tangent and the reverse pass over the joint (z, z') graph written out.

THE KINK.  CELU'' jumps by 1 / alpha at z = 0: a float32 pre-activation on the other side of zero from the float64 one changes that unit's
second-order term by its full size -- in any float32 arithmetic, float32 torch included.  So the table is seeded such that no unit of
any case has |z| < tau, tau = KINK_FACTOR x the largest |z_witness - z_float64| over the table (`preactivations`, `kink_margin`); the
CPU test asserts it.  It is a condition on the inputs, not an allowance in the comparison.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import mlp_float64 as MJ
import mlp_weights_float64 as W

G_BAR = MJ.G_BAR
NAMES, ARRAY_OF = W.NAMES, W.ARRAY_OF
KINK_FACTOR = 16                     # the device's split-fp16 arithmetic is not the witness's: room for it


def _forward(p, xs, alpha):
    """p: the eight arrays, xs [M][n][F] -> e [M][n] and the pre-activations z1, z2, z3"""
    y, zs = xs, []
    for w, b in (("w0", "b0"), ("w2", "b2"), ("w4", "b4")):
        z = torch.baddbmm(p[b].unsqueeze(1), y, p[w].transpose(1, 2))
        zs.append(z)
        y = torch.nn.functional.celu(z, alpha=alpha)
    return torch.einsum("mnh,mh->mn", y, p["w6"]) + p["b6"].unsqueeze(1), zs


def autograd(kinds, x, t, weights=None, offsets=None, alpha=0.1, dtype=torch.float64):
    """-> (gradient: one dict per kind, keys NAMES; E' [grouped atoms][M]; M), numpy in `dtype`"""
    cs = W.atom_weights(kinds, weights, offsets)
    leaves, edots, total = [], [], 0
    for kd, c in zip(kinds, cs):
        p = {name: kd[name].to(dtype).clone().requires_grad_(True) for name in ARRAY_OF.values()}
        leaves.append(p)
        rows = kd["atoms"].long()
        M = p["w0"].shape[0]
        xs = x.to(dtype)[rows].unsqueeze(0).repeat(M, 1, 1).requires_grad_(True)      # member m reads its own copy: g [M][n][F] in one pass
        e, _ = _forward(p, xs, alpha)
        if e.numel() == 0:
            edots.append(np.zeros((0, M)))
            continue
        (g,) = torch.autograd.grad(e.sum(), xs, create_graph=True)
        edot = (g * t.to(dtype)[rows].unsqueeze(0)).sum(-1)                            # [M][n]
        edots.append(edot.detach().numpy().T.copy())
        total = total + (edot * torch.as_tensor(c, dtype=dtype)).sum()
    if torch.is_tensor(total):
        total.backward()
    out = [{g: (p[a].grad if p[a].grad is not None else torch.zeros_like(p[a])).numpy() for g, a in ARRAY_OF.items()} for p in leaves]
    return out, np.concatenate(edots, 0), float(total.detach()) if torch.is_tensor(total) else 0.0


def tangent_energy(kinds, x, t, alpha=0.1):
    """E' [grouped atoms][M] by the forward tangent alone, float64 numpy (no autograd)"""
    out = []
    for kd in kinds:
        p = {name: kd[name].double().numpy() for name in ARRAY_OF.values()}
        rows = kd["atoms"].long().numpy()
        xs, ts = x.double().numpy()[rows], t.double().numpy()[rows]
        slope = lambda z: np.where(z > 0, 1.0, np.exp(np.minimum(z, 0) / alpha))
        celu = lambda z: np.where(z > 0, z, alpha * np.expm1(np.minimum(z, 0) / alpha))
        z = np.einsum("mhf,nf->mnh", p["w0"], xs) + p["b0"][:, None]; zd = np.einsum("mhf,nf->mnh", p["w0"], ts)
        for w, b in (("w2", "b2"), ("w4", "b4")):
            y, yd = celu(z), slope(z) * zd
            z = np.einsum("mhk,mnk->mnh", p[w], y) + p[b][:, None]; zd = np.einsum("mhk,mnk->mnh", p[w], yd)
        out.append(np.einsum("mnh,mh->nm", slope(z) * zd, p["w6"]))
    return np.concatenate(out, 0)


def energy(kinds, x, alpha=0.1):
    """E [grouped atoms][M], float64 numpy: what `tangent_energy` is the directional derivative of"""
    out = []
    for kd in kinds:
        p = {name: kd[name].double() for name in ARRAY_OF.values()}
        xs = x.double()[kd["atoms"].long()].unsqueeze(0).repeat(p["w0"].shape[0], 1, 1)
        out.append(_forward(p, xs, alpha)[0].numpy().T)
    return np.concatenate(out, 0)


def closed_form(kinds, x, t, weights=None, offsets=None, alpha=0.1):
    """e3 = c w6 s''(z3) z'3, e2 = s'(z2) W4^T e3 + s''(z2) z'2 W4^T (c d3), e1 likewise; dW4 = sum (c d3) (x) y'2 + e3 (x) y2, ... in
    float64 numpy"""
    cs = W.atom_weights(kinds, weights, offsets)
    out = []
    for kd, c in zip(kinds, cs):
        p = {name: kd[name].double().numpy() for name in ARRAY_OF.values()}
        rows = kd["atoms"].long().numpy()
        xs, ts = x.double().numpy()[rows], t.double().numpy()[rows]
        celu = lambda z: np.where(z > 0, z, alpha * np.expm1(np.minimum(z, 0) / alpha))
        s1 = lambda z: np.where(z > 0, 1.0, np.exp(np.minimum(z, 0) / alpha))
        s2 = lambda z: np.where(z > 0, 0.0, np.exp(np.minimum(z, 0) / alpha) / alpha)
        z1 = np.einsum("mhf,nf->mnh", p["w0"], xs) + p["b0"][:, None]; y1 = celu(z1)
        z2 = np.einsum("mhk,mnk->mnh", p["w2"], y1) + p["b2"][:, None]; y2 = celu(z2)
        z3 = np.einsum("mhk,mnk->mnh", p["w4"], y2) + p["b4"][:, None]
        zd1 = np.einsum("mhf,nf->mnh", p["w0"], ts); yd1 = s1(z1) * zd1
        zd2 = np.einsum("mhk,mnk->mnh", p["w2"], yd1); yd2 = s1(z2) * zd2
        zd3 = np.einsum("mhk,mnk->mnh", p["w4"], yd2); yd3 = s1(z3) * zd3
        d3 = c[:, :, None] * p["w6"][:, None] * s1(z3)
        d2 = np.einsum("mhk,mnh->mnk", p["w4"], d3) * s1(z2)
        d1 = np.einsum("mhk,mnh->mnk", p["w2"], d2) * s1(z1)
        e3 = c[:, :, None] * p["w6"][:, None] * s2(z3) * zd3
        e2 = s1(z2) * np.einsum("mhk,mnh->mnk", p["w4"], e3) + s2(z2) * zd2 * np.einsum("mhk,mnh->mnk", p["w4"], d3)
        e1 = s1(z1) * np.einsum("mhk,mnh->mnk", p["w2"], e2) + s2(z1) * zd1 * np.einsum("mhk,mnh->mnk", p["w2"], d2)
        out.append(dict(dw6=np.einsum("mn,mnh->mh", c, yd3), db6=np.zeros(c.shape[0]),
                        dw4=np.einsum("mnh,mnk->mhk", d3, yd2) + np.einsum("mnh,mnk->mhk", e3, y2), db4=e3.sum(1),
                        dw2=np.einsum("mnh,mnk->mhk", d2, yd1) + np.einsum("mnh,mnk->mhk", e2, y1), db2=e2.sum(1),
                        dw0=np.einsum("mnh,nf->mhf", d1, ts) + np.einsum("mnh,nf->mhf", e1, xs), db0=e1.sum(1)))
    return out


def preactivations(kinds, x, alpha=0.1, dtype=torch.float64):
    """every z of every unit of every (kind, atom, member), one flat float64 numpy array, computed in `dtype`"""
    out = []
    for kd in kinds:
        p = {name: kd[name].to(dtype) for name in ARRAY_OF.values()}
        xs = x.to(dtype)[kd["atoms"].long()].unsqueeze(0).repeat(p["w0"].shape[0], 1, 1)
        out += [z.double().numpy().ravel() for z in _forward(p, xs, alpha)[1]]
    return np.concatenate(out)


def kink_margin(name):
    """-> (the smallest |z| over all units of the case in float64, the largest |z_witness - z_float64|)"""
    f = frame(name)
    xj = f.x[:, f.columns].contiguous()
    z64, z32 = preactivations(f.judged, xj), preactivations(f.judged, xj, dtype=torch.float32)
    return float(np.abs(z64).min()), float(np.abs(z32 - z64).max())


def worst(got, want):
    return W.worst(got, want)


def worst_edot(got, want):
    """the largest error of E' in units of the judge's largest entry"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and np.isfinite(got).all()
    if want.size == 0:
        return 0.0
    return float(np.abs(got.astype(np.float64) - want).max()) / float(np.abs(want).max())


# ---------------------------------------------------------------------------------------------- the cases
# The default frame: one kind of 37 atoms on a shuffled subset of the rows of x, two members, widths (96, 64, 32), F = 64, alpha 0.1,
# act_scale_log2 4, inputs and tangents N(0, 1), no weights.  The tile pass takes 32 atoms per workgroup and a contraction wave walks every
# atom of the kind in steps of 16.  Frames are kept small -- a case is there for an edge, and every unit is one more chance to sit on
# the kink -- and the seeds are chosen so that the kink condition holds (see the module's docstring).
# `t_scale`: the tangent is multiplied by it; `t_width`: t is wider than x and NaN behind the features.
Case = namedtuple("Case", "name F widths M counts k saturate x_width live weights offsets t_scale t_width seed",
                  defaults=(64, (96, 64, 32), 2, (37,), 4, False, None, None, None, None, 1.0, None, 0))
ATOM_COUNTS = (1, 31, 32, 33, 63, 64, 65, 129)
FEATURES = (8, 24, 40, 72, 1000)
WIDTHS = ((32, 32, 32), (64, 256, 32), (256, 256, 256), (40, 96, 17))
MEMBERS = (1, 3, 8)
SEEDS = {}                           # filled below: name -> seed


def _cases():
    out = [Case("default")]
    out += [Case(f"atoms-{n}", widths=(32, 64, 32), M=1 if n > 65 else 2, counts=(n,)) for n in ATOM_COUNTS]
    out += [Case(f"F-{F}", F=F) for F in FEATURES]
    out += [Case("widths-" + "x".join(map(str, w)), widths=w, M=3 if max(w) < 256 else 1, counts=(33,)) for w in WIDTHS]
    out += [Case(f"members-{M}", M=M, widths=(32, 64, 32), counts=(33,), weights="random") for M in MEMBERS]
    out.append(Case("molecules", M=3, counts=(70,), widths=(32, 64, 32), weights="random", offsets=MJ.MOLECULES))
    out.append(Case("zero-member", M=3, counts=(70,), widths=(32, 64, 32), weights="zero-member", offsets=MJ.MOLECULES))
    out.append(Case("two-kinds", F=40, widths=((32, 32, 32), (64, 32, 96)), counts=(0, 33), weights="random"))
    out.append(Case("live", F=64, M=3, x_width=160, live=MJ.C_LIVE, weights="random"))
    out.append(Case("ldt-nan", F=72, t_width=80))
    out.append(Case("scale-12", F=40, widths=(32, 96, 32), k=12, saturate=True))
    out.append(Case("saturated", F=96, widths=(64, 64, 64), saturate=True, weights="random"))
    out.append(Case("t-large", t_scale=2.0 ** 20, weights="random"))
    out.append(Case("t-small", t_scale=2.0 ** -20, weights="random"))
    return {c.name: c for c in out}


CASES = _cases()
SEEDS.update({name: 1200 + 10 * i for i, name in enumerate(CASES)})
# seeds moved to the next one that keeps every unit of the case clear of the kink (docs/LAB_NOTEBOOK_mlp_force_weights.md: the largest
# |z_witness - z_float64| of the table is 3.6e-6, at F-1000, so tau = 5.8e-5; the smallest |z| of the table is 8.7e-5)
SEEDS.update({"atoms-31": 1221, "atoms-65": 1281, "atoms-129": 1287, "F-24": 1303, "widths-32x32x32": 1345, "widths-64x256x32": 1352,
              "widths-256x256x256": 1395, "widths-40x96x17": 1379, "members-1": 1381, "members-3": 1393, "members-8": 1427,
              "molecules": 1414, "zero-member": 1433, "two-kinds": 1431, "live": 1447, "scale-12": 1461})
Frame = namedtuple("Frame", "case kinds x t weights offsets judged columns want edot")


def build(c, seed):
    """the seeded networks, inputs, tangents and weights of a case (no judgement)"""
    gen = torch.Generator().manual_seed(seed)
    n = sum(c.counts)
    rows = max(MJ.ROWS, n + 10)
    live_route = c.live is not None
    x_width = c.x_width or c.F
    perm = torch.randperm(n if c.offsets is not None else rows, generator=gen)[:n]
    x = torch.randn((rows, x_width), generator=gen)
    t = torch.randn((rows, c.t_width or x_width), generator=gen) * c.t_scale
    widths = c.widths if isinstance(c.widths[0], tuple) else (c.widths,) * len(c.counts)
    kinds, first = [], 0
    for s, (w, count) in enumerate(zip(widths, c.counts)):
        kd = MJ.networks(w, c.M, x_width, seed=seed * 10 + s)
        if c.saturate:
            kd = MJ.saturating_biases(kd, seed * 10 + s)
        kd["atoms"] = perm[first:first + count].to(torch.int32)
        first += count
        kinds.append(kd)
    columns = torch.arange(c.F) if not live_route else torch.tensor([16 * g + i for g in c.live for i in range(16)])
    judged = [dict(kd, w0=kd["w0"][:, :, columns].contiguous()) if live_route else kd for kd in kinds]
    tj = t[:, columns].contiguous()
    t = t.clone()
    dead = torch.ones(t.shape[1], dtype=torch.bool)
    dead[columns] = False
    t[:, dead] = float("nan")                                  # columns the networks do not read: behind the features, or dead blocks
    batch = 1 if c.offsets is None else len(c.offsets) - 1
    weights = None
    if c.weights == "random":
        weights = MJ.random_weights(batch, c.M, seed)
    elif c.weights == "zero-member":
        weights = MJ.random_weights(batch, c.M, seed)
        weights[weights == 0.0] = 0.25
        weights[:, 1] = 0.0
    return kinds, x, t, tj, weights, judged, columns


@functools.lru_cache(maxsize=None)
def frame(name):
    """a case's frame and the judge's gradient and E': computed once, not changed.  `kinds` as capi.FusedMLP takes them; `judged`: the
    kinds over the F columns the networks read (`columns` of x and t)."""
    c = CASES[name]
    kinds, x, t, tj, weights, judged, columns = build(c, SEEDS[name])
    want, edot, _ = autograd(judged, x[:, columns].contiguous(), tj, weights, c.offsets)
    for a in [edot] + [a for kd in want for a in kd.values()]:
        a.setflags(write=False)
    return Frame(c, kinds, x, t, weights, c.offsets, judged, columns, want, edot)


def tangent_of(f):
    """the tangent over the judged columns (no NaN)"""
    return f.t[:, f.columns].contiguous()


def witness(name):
    f = frame(name)
    got, edot, _ = autograd(f.judged, f.x[:, f.columns].contiguous(), tangent_of(f), f.weights, f.offsets, dtype=torch.float32)
    return got, edot


# ---------------------------------------------------------------------------------------------- a force loss through a whole model
def force_loss_float64(kinds, species, frames, box, e0=None, f0=None, what="mean"):
    """The parameter gradient of a loss with forces in it, in float64: the restatement's AEV (ani_float64), the networks as `kinds`
    states them (mlp_weights_float64.kinds_of_module(nets, torch.float64)), F = -dS/dx by autograd with create_graph, summed over the
    frames [B][N][3].  what = "mean": S = E, the ensemble mean with the self energy, loss = (E - E0)^2 + sum (F - F0)^2;
    "qbcs": S = the QBC factor std_m(E_m) / sqrt(N) (unbiased), loss = sum (F - F0)^2 -- the upstream weights of the member energies
    depend on the parameters.  Targets that are None are made up next to the values (E + 0.3, F + 0.05 N(0, 1)).
    -> (gradient per kind, E0 [B], F0 [B][N][3], loss)"""
    import ani_members_float64 as AJ
    import ani_tangent_float64 as AT
    from ani_float64 import Restatement
    from nnpops_amd import workloads
    rf, af = workloads.ani2x_functions()
    rest = Restatement(7, 5.1, 3.5, species, rf, af, True)
    leaves = [{name: kd[name].clone().requires_grad_(True) for name in ARRAY_OF.values()} for kd in kinds]
    members = leaves[0]["w0"].shape[0]
    box64 = np.asarray(AT.VACUUM if box is None else box, dtype=np.float32).astype(np.float64).reshape(3, 3)
    loss, energies, forces = 0, [], []
    for b in range(len(frames)):
        pos64 = np.asarray(frames[b], dtype=np.float32).astype(np.float64)
        pairs, triples = rest.lists(pos64, box64)
        x, B = torch.tensor(pos64, requires_grad=True), torch.tensor(box64)
        radial = torch.zeros(rest.N * rest.S, rest.nR, dtype=torch.float64)
        angular = torch.zeros(rest.N * rest.NB, rest.nA, dtype=torch.float64)
        terms, rows = rest._radial_terms(x, B, pairs)
        radial = radial.index_add(0, rows, terms)
        if len(triples[0]):
            terms, rows = rest._angular_terms(x, B, triples)
            angular = angular.index_add(0, rows, terms)
        aev = torch.cat([radial.reshape(rest.N, -1), angular.reshape(rest.N, -1)], dim=1)
        per_member = torch.zeros(members, dtype=torch.float64) + AJ.self_energy(species)
        for kd, p in zip(kinds, leaves):
            xs = aev[kd["atoms"].long()].unsqueeze(0).expand(members, -1, -1)
            per_member = per_member + _forward(p, xs, 0.1)[0].sum(1)
        value = per_member.mean() if what == "mean" else per_member.std(unbiased=True) / float(rest.N) ** 0.5
        force = -torch.autograd.grad(value, x, create_graph=True)[0]
        e0_b = float(value.detach()) + 0.3 if e0 is None else e0[b]
        f0_b = force.detach() + 0.05 * torch.randn(force.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(70 + b)) \
            if f0 is None else torch.as_tensor(f0[b])
        loss = loss + ((value - e0_b) ** 2 if what == "mean" else 0) + ((force - f0_b) ** 2).sum()
        energies.append(e0_b)
        forces.append(f0_b.numpy())
    flat = [p[name] for p in leaves for name in ARRAY_OF.values()]
    grads = torch.autograd.grad(loss, flat)
    it = iter(grads)
    out = [{g: next(it).numpy() for g in ARRAY_OF} for _ in leaves]
    return out, np.array(energies), np.stack(forces), float(loss.detach())
