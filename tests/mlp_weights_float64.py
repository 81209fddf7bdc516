"""The float64 judge of the fused atomic networks' WEIGHT gradients (csrc/mlp_weight_grad.h; no GPU code, no tests; importable
anywhere) and the table of cases tests/test_mlp_weights_gpu.py runs, so that the CPU file that pins the judge and the GPU file that
uses it see the same numbers.

The function is mlp_float64's restatement of the reference's TorchANIBatchedNN (per atom and member Linear CELU Linear CELU Linear
CELU Linear).  The loss is  L = sum over the kinds, their atoms a and the members m of  c[molecule of a][m] * e[a][m]  -- `c` the
upstream weight of every (molecule, member), all ones without a table -- and the judge is dL/d(the eight arrays of every kind):
  `autograd`     float64 autograd with the eight arrays as leaves (the judge), or float32 (the WITNESS: what plain float32 arithmetic
                 of the same sums loses, never a kernel);
  `closed_form`  the same numbers from the four lines of the backward pass written out, without autograd.
A gradient is a list with one dict per kind, keys NAMES, in the shapes of the kind's arrays.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import mlp_float64 as MJ

G_BAR = MJ.G_BAR                     # the project's gradient bar: of the largest entry of each array of each kind
NAMES = ("dw0", "db0", "dw2", "db2", "dw4", "db4", "dw6", "db6")
ARRAY_OF = dict(dw0="w0", db0="b0", dw2="w2", db2="b2", dw4="w4", db4="b4", dw6="w6", db6="b6")


def atom_weights(kinds, weights, offsets):
    """-> per kind c [M][n] float64: the weight of (the molecule of every atom of the kind, member); weights None: ones, [M] or [1][M]:
    one molecule, [B][M] with offsets [B + 1] over the rows of x"""
    M = kinds[0]["w0"].shape[0]
    out = []
    for kd in kinds:
        rows = kd["atoms"].long().numpy()
        if weights is None:
            c = np.ones((M, len(rows)))
        else:
            w = np.asarray(weights, dtype=np.float64).reshape(-1, M)
            mol = np.zeros(len(rows), dtype=np.int64) if offsets is None else MJ.molecule_of_rows(offsets, rows)
            c = w[mol].T.copy() if len(rows) else np.zeros((M, 0))
        out.append(c)
    return out


def autograd(kinds, x, weights=None, offsets=None, alpha=0.1, dtype=torch.float64):
    cs = atom_weights(kinds, weights, offsets)
    leaves, loss = [], 0
    for kd, c in zip(kinds, cs):
        p = {name: kd[name].to(dtype).clone().requires_grad_(True) for name in ARRAY_OF.values()}
        leaves.append(p)
        y = x.to(dtype)[kd["atoms"].long()].unsqueeze(0).expand(p["w0"].shape[0], -1, -1)             # [M][n][F]
        for w, b in (("w0", "b0"), ("w2", "b2"), ("w4", "b4")):
            y = torch.nn.functional.celu(torch.baddbmm(p[b].unsqueeze(1), y, p[w].transpose(1, 2)), alpha=alpha)
        e = torch.einsum("mnh,mh->mn", y, p["w6"]) + p["b6"].unsqueeze(1)                              # [M][n]
        loss = loss + (e * torch.as_tensor(c, dtype=dtype)).sum()
    loss.backward()
    out = [{g: p[a].grad.numpy() for g, a in ARRAY_OF.items()} for p in leaves]
    return out, float(loss.detach())


def closed_form(kinds, x, weights=None, offsets=None, alpha=0.1):
    """d3 = c w6 CELU'(z3), d2 = (W4^T d3) CELU'(z2), d1 = (W2^T d2) CELU'(z1); dW6 = sum c y3, db6 = sum c, dW4 = sum d3 (x) y2, ...
    in float64 numpy"""
    cs = atom_weights(kinds, weights, offsets)
    out = []
    for kd, c in zip(kinds, cs):
        p = {name: kd[name].double().numpy() for name in ARRAY_OF.values()}
        xs = x.double().numpy()[kd["atoms"].long().numpy()]                                            # [n][F]
        celu = lambda z: np.where(z > 0, z, alpha * np.expm1(np.minimum(z, 0) / alpha))
        slope = lambda z: np.where(z > 0, 1.0, np.exp(np.minimum(z, 0) / alpha))
        z1 = np.einsum("mhf,nf->mnh", p["w0"], xs) + p["b0"][:, None]; y1 = celu(z1)
        z2 = np.einsum("mhk,mnk->mnh", p["w2"], y1) + p["b2"][:, None]; y2 = celu(z2)
        z3 = np.einsum("mhk,mnk->mnh", p["w4"], y2) + p["b4"][:, None]; y3 = celu(z3)
        d3 = c[:, :, None] * p["w6"][:, None] * slope(z3)
        d2 = np.einsum("mhk,mnh->mnk", p["w4"], d3) * slope(z2)
        d1 = np.einsum("mhk,mnh->mnk", p["w2"], d2) * slope(z1)
        out.append(dict(dw6=np.einsum("mn,mnh->mh", c, y3), db6=c.sum(1),
                        dw4=np.einsum("mnh,mnk->mhk", d3, y2), db4=d3.sum(1),
                        dw2=np.einsum("mnh,mnk->mhk", d2, y1), db2=d2.sum(1),
                        dw0=np.einsum("mnh,nf->mhf", d1, xs), db0=d1.sum(1)))
    return out


def worst(got, want):
    """-> the largest error of `got` (a gradient, numpy or tensors) in units of the largest entry of the judge's array, over all arrays
    of all kinds, with its place.  An array the judge has as zeros must be zeros."""
    top, where = 0.0, None
    for k, (g, w) in enumerate(zip(got, want)):
        for name in NAMES:
            a = g[name].detach().cpu().numpy() if torch.is_tensor(g[name]) else np.asarray(g[name])
            assert a.shape == w[name].shape, (k, name, a.shape, w[name].shape)
            assert np.isfinite(a).all(), (k, name)
            scale = float(np.abs(w[name]).max()) if w[name].size else 0.0
            err = float(np.abs(a.astype(np.float64) - w[name]).max()) if w[name].size else 0.0
            if scale == 0.0:
                assert err == 0.0, (k, name, err)
                continue
            if err / scale > top:
                top, where = err / scale, (k, name)
    return top, where


# ---------------------------------------------------------------------------------------------- the cases
# The default frame is mlp_float64's: one kind of 70 atoms on a shuffled subset of 80 rows, two members, widths (96, 64, 32), F = 96,
# alpha 0.1, act_scale_log2 4, inputs N(0, 1), no weights.  `weights`: None, "random" (MJ.random_weights: both signs, an exact zero from
# three members on), "zero-member" (member 1 is zero for every molecule); `offsets`: the molecules the rows of x belong to.
Case = namedtuple("Case", "name F widths M counts k saturate x_width live weights offsets seed",
                  defaults=(96, (96, 64, 32), 2, (70,), 4, False, None, None, None, None, 0))
# (the tile pass takes 64 atoms per workgroup and a contraction wave walks every atom of the kind: 200 is three tiles and a part)
ATOM_COUNTS = (1, 63, 64, 65, 129, 200)
FEATURES = (8, 24, 40, 72, 1000)
WIDTHS = ((32, 32, 32), (64, 256, 32), (256, 256, 256), (40, 96, 17))
MEMBERS = (1, 3, 8)


def _cases():
    out = [Case("default", seed=900)]
    out += [Case(f"atoms-{n}", counts=(n,), seed=910 + i) for i, n in enumerate(ATOM_COUNTS)]
    out += [Case(f"F-{F}", F=F, seed=920 + i) for i, F in enumerate(FEATURES)]
    out += [Case("widths-" + "x".join(map(str, w)), widths=w, M=3, counts=(65,), seed=930 + i) for i, w in enumerate(WIDTHS)]
    out += [Case(f"members-{M}", M=M, F=64, weights="random", seed=940 + i) for i, M in enumerate(MEMBERS)]
    out.append(Case("molecules", M=3, F=64, weights="random", offsets=MJ.MOLECULES, seed=950))
    out.append(Case("zero-member", M=3, F=64, weights="zero-member", offsets=MJ.MOLECULES, seed=951))
    out.append(Case("eight-kinds", F=40, widths=MJ.F_WIDTHS, counts=MJ.F_COUNTS, weights="random", seed=960))
    out.append(Case("live", F=64, M=3, x_width=160, live=MJ.C_LIVE, weights="random", seed=970))
    out.append(Case("ldx-nan", F=72, x_width=80, seed=980))                    # the networks read 72 of 80 columns, the rest is NaN
    out.append(Case("scale-12", F=40, widths=(32, 96, 32), k=12, saturate=True, seed=990))
    out.append(Case("saturated", F=96, widths=(64, 64, 64), saturate=True, weights="random", seed=991))
    return {c.name: c for c in out}


CASES = _cases()
Frame = namedtuple("Frame", "case kinds x weights offsets judged columns want")


@functools.lru_cache(maxsize=None)
def frame(name):
    """the seeded networks, inputs and weights of a case and the judge's gradient: computed once, not changed.  `kinds` as
    capi.FusedMLP takes them (w0 over all x_width columns for the live route); `judged`: the kinds over the F columns the networks
    read (`columns` of x); `want`: dL/d(judged arrays), float64."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    n = sum(c.counts)
    rows = max(MJ.ROWS, n + 10)
    live_route = c.live is not None
    x_width = c.x_width or c.F
    w_width = x_width if live_route else c.F                                   # (ldx-nan: x is wider than the networks)
    perm = torch.randperm(n if c.offsets is not None else rows, generator=gen)[:n]
    x = torch.randn((rows, x_width), generator=gen)
    widths = c.widths if isinstance(c.widths[0], tuple) else (c.widths,) * len(c.counts)
    kinds, first = [], 0
    for s, (w, count) in enumerate(zip(widths, c.counts)):
        kd = MJ.networks(w, c.M, w_width, seed=c.seed * 10 + s)
        if c.saturate:
            kd = MJ.saturating_biases(kd, c.seed * 10 + s)
        kd["atoms"] = perm[first:first + count].to(torch.int32)
        first += count
        kinds.append(kd)
    columns = torch.arange(c.F) if not live_route else torch.tensor([16 * g + i for g in c.live for i in range(16)])
    judged = [dict(kd, w0=kd["w0"][:, :, columns].contiguous()) if live_route else kd for kd in kinds]
    xj = x[:, columns].contiguous()
    if not live_route and x_width > c.F:
        x = x.clone()
        x[:, c.F:] = float("nan")
    batch = 1 if c.offsets is None else len(c.offsets) - 1
    weights = None
    if c.weights == "random":
        weights = MJ.random_weights(batch, c.M, c.seed)
    elif c.weights == "zero-member":
        weights = MJ.random_weights(batch, c.M, c.seed)
        weights[weights == 0.0] = 0.25
        weights[:, 1] = 0.0
    want, _ = autograd(judged, xj, weights, c.offsets)
    for kd in want:
        for a in kd.values():
            a.setflags(write=False)
    return Frame(c, kinds, x, weights, c.offsets, judged, columns, want)


def witness(name):
    f = frame(name)
    got, _ = autograd(f.judged, f.x[:, f.columns].contiguous(), f.weights, f.offsets, dtype=torch.float32)
    return got


# ---------------------------------------------------------------------------------------------- modules
def kinds_of_module(nets, dtype=torch.float32):
    """the eight arrays of a species-grouped TorchANIBatchedNN implementation (nets = module[0]) as the judge's kinds, at the padded
    widths of the module (the padding is zeros: the same function), atoms = the module's atoms of every kind"""
    kinds, first = [], 0
    order = nets.atom_order.cpu()
    for k, n in enumerate(nets.group_sizes):
        get = lambda name: getattr(nets, name).detach().cpu().to(dtype)[k]
        kinds.append(dict(w0=get("layer0_weights"), b0=get("layer0_biases")[:, :, 0], w2=get("layer2_weights"), b2=get("layer2_biases")[:, :, 0],
                          w4=get("layer4_weights"), b4=get("layer4_biases")[:, :, 0], w6=get("layer6_weights")[:, 0, :],
                          b6=get("layer6_biases")[:, 0, 0], atoms=order[first:first + n].to(torch.int32)))
        first += n
    return kinds


def gradients_of_module(nets):
    """the .grad of the module's eight parameters as a gradient of the judge's shape (a parameter without .grad counts as zeros)"""
    def grad(name):
        p = getattr(nets, name)
        return (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu()
    out = []
    for k in range(len(nets.group_sizes)):
        out.append(dict(dw0=grad("layer0_weights")[k], db0=grad("layer0_biases")[k][:, :, 0], dw2=grad("layer2_weights")[k],
                        db2=grad("layer2_biases")[k][:, :, 0], dw4=grad("layer4_weights")[k], db4=grad("layer4_biases")[k][:, :, 0],
                        dw6=grad("layer6_weights")[k][:, 0, :], db6=grad("layer6_biases")[k][:, 0, 0]))
    return out
