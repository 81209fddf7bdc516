"""The float64 judge of the CFConv weight gradients (no GPU code, no tests; importable anywhere), its closed form, a float32 witness
and the table of cases.

With the four arrays of the filter network as float64 leaves and L = <g, CFConv(x)> over a fixed half list {i < j} at distances r,
`judge` returns dL/d(w1 [W][G], b1, w2 [out][in], b2) from torch.autograd.grad over cfconv_float64.Restatement's layer.  `closed_form`
writes the same four sums out pair by pair, as nnpops_cfconv_backprop_weights evaluates them:

    q_c = g[i][c] x[j][c] + g[j][c] x[i][c]      s_c = cut(r) q_c
    db2[c] = sum_p s_c                           dw2[c][a] = sum_p s_c y_a
    t_a = act'(z_a) sum_c s_c w2[c][a]           db1[a] = sum_p t_a             dw1[a][g] = sum_p t_a gamma_g

in float64, or -- `dtype=torch.float32`: the WITNESS -- in CPU float32 from float32 distances: what any float32 evaluation of these
sums may be expected to reach.  tests/test_cfconv_weights_reference_cpu.py pins all three; tests/test_cfconv_weights_gpu.py judges the
kernels by them.

Frames and layers come from cfconv_dispatch_float64 (`frame`, `layer`, `chain:P`) and, for the periodic cell-grid frame, from
cfconv_float64.frame("liquid1500").
"""
import collections
import functools
import math

import numpy as np
import torch

import cfconv_dispatch_float64 as dispatch
import cfconv_float64
from cfconv_float64 import FORCE_RTOL, Restatement, SecondOrder, sigma_of

BAR = FORCE_RTOL                    # each gradient to this fraction of its largest entry: the project's bar for CFConv gradients
NAMES = ("w1", "b1", "w2", "b2")
TILE = 16                           # pair slots per tile of both weight-gradient kernels (kWgradTile)


# ---------------------------------------------------------------------------------------------- frames and pair lists
def frame(tag):
    """-> (pos, box or None, cutoff)"""
    if tag == "liquid1500":                       # periodic, 1500 atoms: the cell grid builds its rows
        pos, box = cfconv_float64.frame(tag)
        return pos, box, dispatch.CUTOFF
    return dispatch.frame(tag)


def layer(tag, W, G):
    """-> (w1, b1, w2, b2, x, gout), seeded by the shape as cfconv_dispatch_float64.layer seeds them"""
    return cfconv_float64.weights(W, G, len(frame(tag)[0]), 1000 * W + G)


def judge_of(W, G, cutoff, act, w1, b1, w2, b2):
    return Restatement(W, G, cutoff, sigma_of(G), act, w1, b1, w2, b2)


def pair_list(J, pos, box=None, offsets=None):
    """-> (i, j, r float64) of the half list: Restatement.pairs with a box, SecondOrder.open without; `offsets` (batched molecules):
    the molecules' own lists, one behind the other"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    if offsets is not None:
        parts = []
        for lo, hi in zip(offsets[:-1], offsets[1:]):
            i, j, r = pair_list(J, pos[lo:hi])
            parts.append((i + lo, j + lo, r))
        return tuple(np.concatenate([q[k] for q in parts]) for k in range(3))
    if box is not None:
        B = np.asarray(box, np.float32).astype(np.float64).reshape(3, 3)
        i, j, n = J.pairs(p, B)
        d = p[j] - p[i] + n @ B
    else:
        so = SecondOrder.open(J, pos)
        i, j = so.i.numpy(), so.j.numpy()
        d = p[j] - p[i]
    return np.asarray(i, np.int64), np.asarray(j, np.int64), np.sqrt((d * d).sum(axis=1))


# ---------------------------------------------------------------------------------------------- the judge
def _wide(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64)).to(dtype)


def layer_output(J, w1, b1, w2, b2, i, j, r, x):
    """Restatement's layer with the four arrays given (tensors): the filter rows from the distances, the symmetric accumulation"""
    it, jt = torch.as_tensor(i), torch.as_tensor(j)
    gamma = torch.exp(-0.5 * ((r[:, None] - J.mu[None, :].to(r.dtype)) / J.sigma) ** 2)
    s1 = gamma @ w1.T + b1
    y1 = torch.log(0.5 * torch.exp(s1) + 0.5) if J.act == 0 else torch.tanh(s1)
    fc = 0.5 * torch.cos(math.pi * r / J.cutoff) + 0.5
    y2 = fc[:, None] * (y1 @ w2.T + b2)
    return torch.zeros_like(x).index_add(0, it, y2 * x[jt]).index_add(0, jt, y2 * x[it])


def judge(J, i, j, r, x, g, weights=None):
    """-> dict(w1, b1, w2, b2: float64 numpy gradients of L = <g, CFConv(x)>, L, out); `weights`: four arrays in place of J's own"""
    src = (J.w1, J.b1, J.w2, J.b2) if weights is None else [_wide(w).reshape(s.shape) for w, s in zip(weights, (J.w1, J.b1, J.w2, J.b2))]
    leaves = [w.clone().requires_grad_(True) for w in src]
    out = layer_output(J, *leaves, i, j, torch.tensor(np.asarray(r, np.float64)), _wide(x))
    L = (out * _wide(g)).sum()
    grads = torch.autograd.grad(L, leaves)
    res = {n: v.numpy() for n, v in zip(NAMES, grads)}
    res.update(L=float(L.detach()), out=out.detach().numpy())
    return res


def loss(J, weights, i, j, r, x, g):
    """L alone, float64, at the given four arrays (float64 numpy, any values: the central differences displace them)"""
    ws = [torch.tensor(np.asarray(w, np.float64)) for w in weights]
    out = layer_output(J, *ws, i, j, torch.tensor(np.asarray(r, np.float64)), _wide(x))
    return float((out * _wide(g)).sum())


# ---------------------------------------------------------------------------------------------- closed form and witness
def closed_form(J, i, j, r, x, g, dtype=torch.float64, chunk=8192):
    """The four sums of the module docstring, pair by pair (no autograd).  dtype float32: every array, the distances included, rounded
    to float32 first and every operation in CPU float32 -- the witness."""
    W, G = J.W, J.G
    w1, b1, w2, b2 = (t.to(dtype) for t in (J.w1, J.b1, J.w2, J.b2))
    mu = J.mu.to(dtype)
    xt, gt = _wide(x, dtype), _wide(g, dtype)
    rt = torch.tensor(np.asarray(r, np.float64)).to(dtype)
    it, jt = torch.as_tensor(i), torch.as_tensor(j)
    dw1, db1 = torch.zeros((W, G), dtype=dtype), torch.zeros(W, dtype=dtype)
    dw2, db2 = torch.zeros((W, W), dtype=dtype), torch.zeros(W, dtype=dtype)
    for lo in range(0, len(i), chunk):
        ii, jj, rr = it[lo:lo + chunk], jt[lo:lo + chunk], rt[lo:lo + chunk]
        gamma = torch.exp(-0.5 * ((rr[:, None] - mu[None, :]) / J.sigma) ** 2)
        z = gamma @ w1.T + b1
        if J.act == 0:
            e = torch.exp(z)
            y, dact = torch.log(0.5 * e + 0.5), e / (e + 1.0)
        else:
            y = torch.tanh(z)
            dact = 1.0 - y * y
        cut = 0.5 * torch.cos(math.pi * rr / J.cutoff) + 0.5
        s = cut[:, None] * (gt[ii] * xt[jj] + gt[jj] * xt[ii])          # [P][W]
        t = dact * (s @ w2)                                            # sum_c s_c w2[c][a]
        db2 += s.sum(0)
        dw2 += s.T @ y
        db1 += t.sum(0)
        dw1 += t.T @ gamma
    return dict(w1=dw1.numpy(), b1=db1.numpy(), w2=dw2.numpy(), b2=db2.numpy())


def witness(J, i, j, r, x, g):
    return closed_form(J, i, j, np.asarray(r, np.float64).astype(np.float32), x, g, dtype=torch.float32)


def errors(got, ref):
    """{name: max |got - ref| / max |ref|} over the four gradients (0 for two all-zero arrays)"""
    return {n: dispatch.force_error(np.asarray(got[n]).reshape(np.asarray(ref[n]).shape), ref[n]) for n in NAMES}


def figures(err):
    return " ".join(f"{n} {v:.2e}" for n, v in err.items())


# ---------------------------------------------------------------------------------------------- the table
# kernel: which weight-gradient kernel the layer takes (by the width and LDS alone): "mfma" = cfconv_wgrad_mfma (W a multiple of 16 up to
#   128, the kernel's LDS image -- W2, W1^T, three [16][W + 16] tiles, the [16][64 or 256] Gaussian tile -- inside 160 KiB), "vector" else
# env: the NNPOPS_CFCONV_* switches of the case as (name, value) pairs (hashable: `reference` is cached by case)
# path: the forward path the handle's describe() must name (cfconv_dispatch_float64's words)
Case = collections.namedtuple("Case", "name W G act frame env path kernel")
REG, PLANES, MATRIX, VECTOR = dispatch.REG, dispatch.PLANES, dispatch.MATRIX, dispatch.VECTOR


def _cases():
    t = []

    def add(name, W, G, path, kernel, frame="conformer90", acts=dispatch.BOTH, env=None):
        for act in acts:
            t.append(Case(f"{name}-{act}", W, G, act, frame, tuple(sorted((env or {}).items())), path, kernel))

    # layers (conformer90: 2 493 pairs = 155 full tiles and one of 13 pairs)
    add("w1_g10", 1, 10, VECTOR, "vector")
    add("w8_g10", 8, 10, VECTOR, "vector")
    add("w16_g8", 16, 8, MATRIX, "mfma")
    add("w48_g7", 48, 7, MATRIX, "mfma")
    add("w32_g50", 32, 50, REG, "mfma")
    add("w64_g50", 64, 50, REG, "mfma")
    add("w128_g50", 128, 50, REG, "mfma")
    add("w64_g64_planes", 64, 64, PLANES, "mfma")
    add("w128_g173_streamed", 128, 173, VECTOR, "vector")
    add("w136_g10", 136, 10, VECTOR, "vector")
    add("w32_g2", 32, 2, REG, "mfma")
    add("w64_g10_valu", 64, 10, VECTOR, "mfma", env={"NNPOPS_CFCONV_VALU": "1"})
    # the edges of the weight-gradient kernels' own choice: 4 or 16 blocks of Gaussians (G = 64 | 65), and at W = 128 the last G whose
    # image fits in LDS (16384 + 104 * 128 + 6912 + 4096 + 64 floats = 159.3 KiB) and the first that does not
    add("w32_g64_four_blocks", 32, 64, PLANES, "mfma", acts=("ssp",))
    add("w32_g65_sixteen_blocks", 32, 65, PLANES, "mfma", acts=("tanh",))
    add("w16_g256_sixteen_blocks", 16, 256, MATRIX, "mfma", acts=("ssp",))
    add("w128_g104_last_mfma", 128, 104, PLANES, "mfma", acts=("tanh",))
    add("w128_g105_first_vector", 128, 105, PLANES, "vector", acts=("ssp",))
    # pair counts around the tile of each kernel
    for P in (0, 1, TILE - 1, TILE, TILE + 1):
        add(f"chain{P}_w16_g8", 16, 8, MATRIX, "mfma", frame=f"chain:{P}", acts=("ssp",))
        add(f"chain{P}_w24_g10", 24, 10, VECTOR, "vector", frame=f"chain:{P}", acts=("tanh",))
    # more pairs than one sweep of the launch (256 workgroups x 16 pairs), on a periodic frame whose rows the cell grid builds
    add("liquid1500_w32_g16", 32, 16, REG, "mfma", frame="liquid1500", acts=("ssp",))
    add("liquid1500_w24_g10", 24, 10, VECTOR, "vector", frame="liquid1500", acts=("tanh",))
    assert len({c.name for c in t}) == len(t)
    return tuple(t)


CASES = _cases()


def expected_kernel(W, G):
    """the weight-gradient kernel of a layer, from the LDS formula written out by hand (cfconv_weight_grad.h: wgrad_mfma_floats)"""
    if W % 16 or W > 128:
        return "vector"
    floats = W * W + (G + 3) // 4 * 4 * W + 3 * TILE * (W + 16) + TILE * (64 if G <= 64 else 256) + 4 * TILE
    return "mfma" if 4 * floats <= dispatch.LDS_LIMIT else "vector"


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> dict(J, i, j, r, judge = the float64 gradients, witness = the float32 ones) of a case: computed once, read-only"""
    pos, box, cutoff = frame(case.frame)
    w1, b1, w2, b2, x, g = layer(case.frame, case.W, case.G)
    J = judge_of(case.W, case.G, cutoff, case.act, w1, b1, w2, b2)
    i, j, r = pair_list(J, pos, box)
    ref = dict(J=J, i=i, j=j, r=r, judge=judge(J, i, j, r, x, g), witness=witness(J, i, j, r, x, g))
    for d in (ref["judge"], ref["witness"]):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return ref
