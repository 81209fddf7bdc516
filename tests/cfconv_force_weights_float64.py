"""The float64 judge of the CFConv weight gradients of a force loss (no GPU code, no tests; importable anywhere), its closed form, a
float32 witness and the table of cases.

The backward pass maps (g, x, positions) to gx = dL/dx and gp = dL/dpositions of L = <g, CFConv(x)>.  With cotangents V [N][W] of gx and
Q [N][3] of gp, the double backward differentiates M = <V, gx> + <Q, gp>; nnpops_cfconv_double_backward_weights returns
dM/d(w1 [W][G], b1, w2 [out][in], b2).  `judge` builds M from a create_graph first backward over cfconv_weights_float64.layer_output's
arithmetic, with the pair displacements d [P][3] and the four arrays as float64 leaves (gp gathers dL/dd with +1 at j and -1 at i, so
<Q, gp> = sum_p dL/dd_p . (Q_j - Q_i)), and differentiates it in the four arrays.  `closed_form` writes the same sums out pair by pair,
as the kernels evaluate them:

    A = V_j g_i + V_i g_j     B = x_j g_i + x_i g_j     a = u.(Q_j - Q_i)     p_c = fc A_c + a fc' B_c     q_c = a fc B_c
    db2[c] = sum_p p_c                                  dw2[c][a] = sum_p p_c y_a + q_c y'_a
    P_a = sum_c p_c w2[c][a]   R_a = sum_c q_c w2[c][a]
    t_a = act'(z_a) P_a + act''(z_a) z'_a R_a           t'_a = act'(z_a) R_a
    db1[a] = sum_p t_a                                  dw1[a][g] = sum_p t_a gamma_g + t'_a gamma'_g

in float64, or -- `dtype=torch.float32`: the WITNESS -- in CPU float32 from float32 displacements: what any float32 evaluation of these
sums may be expected to reach.  tests/test_cfconv_force_weights_reference_cpu.py pins all three;
tests/test_cfconv_force_weights_gpu.py judges the kernels by them.

Frames and seeded layers are those of cfconv_weights_float64 / cfconv_dispatch_float64; the cotangents come from
cfconv_float64.cotangents.
"""
import collections
import functools
import math

import numpy as np
import torch

import cfconv_dispatch_float64 as dispatch
import cfconv_float64
import cfconv_weights_float64 as wf
from cfconv_weights_float64 import BAR, NAMES, errors, figures, frame, judge_of, layer

TILE = 16                           # pair slots per tile of the matrix-core kernel (kWgradTile)
VECTOR_TILE = 8                     # ... and of the vector kernel (kWgrad2VectorTile)


def cotangents(tag, W, which="VQ"):
    """-> (V or None, Q or None), seeded by the shape"""
    V, Q = cfconv_float64.cotangents(len(frame(tag)[0]), W, 77000 + W)
    return (V if "V" in which else None), (Q if "Q" in which else None)


def pair_displacements(J, pos, box=None, offsets=None):
    """-> (i, j, d float64 [P][3]) of the half list, d = x_j - x_i (+ n B): cfconv_weights_float64.pair_list with the displacement kept"""
    p = np.asarray(pos, np.float32).astype(np.float64)
    if offsets is not None:
        parts = []
        for lo, hi in zip(offsets[:-1], offsets[1:]):
            i, j, d = pair_displacements(J, pos[lo:hi])
            parts.append((i + lo, j + lo, d))
        return tuple(np.concatenate([q[k] for q in parts]) for k in range(3))
    if box is not None:
        B = np.asarray(box, np.float32).astype(np.float64).reshape(3, 3)
        i, j, n = J.pairs(p, B)
        d = p[j] - p[i] + n @ B
    else:
        so = cfconv_float64.SecondOrder.open(J, pos)
        i, j = so.i.numpy(), so.j.numpy()
        d = p[j] - p[i]
    return np.asarray(i, np.int64), np.asarray(j, np.int64), d.reshape(-1, 3)


# ---------------------------------------------------------------------------------------------- the judge
def _M(J, ws, i, j, d, x, g, V, Q, create_graph):
    """M = <V, gx> + <Q, gp> at the four arrays `ws` (tensors), from a first backward over layer_output"""
    it, jt = torch.as_tensor(i), torch.as_tensor(j)
    dt = torch.tensor(np.asarray(d, np.float64).reshape(-1, 3)).requires_grad_(True)
    xt = wf._wide(x).requires_grad_(True)
    out = wf.layer_output(J, *ws, i, j, dt.norm(dim=1), xt)
    L = (out * wf._wide(g)).sum()
    gx, gd = torch.autograd.grad(L, [xt, dt], create_graph=create_graph, allow_unused=True)
    M = torch.zeros((), dtype=torch.float64)
    if V is not None:
        M = M + (wf._wide(V) * gx).sum()
    if Q is not None and len(i):
        Qt = wf._wide(Q)
        M = M + (gd * (Qt[jt] - Qt[it])).sum()
    return M


def judge(J, i, j, d, x, g, V, Q, weights=None):
    """-> dict(w1, b1, w2, b2: float64 numpy gradients of M, M); `weights`: four arrays in place of J's own"""
    src = (J.w1, J.b1, J.w2, J.b2) if weights is None else [wf._wide(w).reshape(s.shape) for w, s in zip(weights, (J.w1, J.b1, J.w2, J.b2))]
    leaves = [w.clone().requires_grad_(True) for w in src]
    M = _M(J, leaves, i, j, d, x, g, V, Q, True)
    if M.requires_grad:
        grads = torch.autograd.grad(M, leaves, allow_unused=True)
    else:                                                   # (a list without pairs)
        grads = [None] * 4
    res = {n: (torch.zeros_like(w) if v is None else v).detach().numpy() for n, v, w in zip(NAMES, grads, leaves)}
    res["M"] = float(M.detach())
    return res


def M_value(J, weights, i, j, d, x, g, V, Q):
    """M alone, float64, by first-order autograd only, at the given four arrays (float64 numpy: the central differences displace them)"""
    ws = [torch.tensor(np.asarray(w, np.float64)) for w in weights]
    return float(_M(J, ws, i, j, d, x, g, V, Q, False).detach())


# ---------------------------------------------------------------------------------------------- closed form and witness
def closed_form(J, i, j, d, x, g, V, Q, dtype=torch.float64, chunk=8192):
    """The sums of the module docstring, pair by pair (no autograd).  dtype float32: every array, the displacements included, rounded
    to float32 first and every operation in CPU float32 -- the witness."""
    W, G = J.W, J.G
    w1, b1, w2, b2 = (t.to(dtype) for t in (J.w1, J.b1, J.w2, J.b2))
    mu = J.mu.to(dtype)
    xt, gt = wf._wide(x, dtype), wf._wide(g, dtype)
    Vt = wf._wide(V, dtype) if V is not None else torch.zeros_like(xt)
    Qt = wf._wide(Q, dtype) if Q is not None else torch.zeros((len(xt), 3), dtype=dtype)
    dall = torch.tensor(np.asarray(d, np.float64).reshape(-1, 3)).to(dtype)
    it, jt = torch.as_tensor(i), torch.as_tensor(j)
    dw1, db1 = torch.zeros((W, G), dtype=dtype), torch.zeros(W, dtype=dtype)
    dw2, db2 = torch.zeros((W, W), dtype=dtype), torch.zeros(W, dtype=dtype)
    k = math.pi / J.cutoff
    for lo in range(0, len(i), chunk):
        ii, jj, dd = it[lo:lo + chunk], jt[lo:lo + chunk], dall[lo:lo + chunk]
        rr = torch.sqrt((dd * dd).sum(1))
        tt = rr[:, None] - mu[None, :]
        gamma = torch.exp(-0.5 * (tt / J.sigma) ** 2)
        dgamma = -tt / J.sigma ** 2 * gamma
        z, dz = gamma @ w1.T + b1, dgamma @ w1.T
        if J.act == 0:
            e = torch.exp(z)
            y, a1 = torch.log(0.5 * e + 0.5), e / (e + 1.0)
            a2 = a1 * (1.0 - a1)
        else:
            y = torch.tanh(z)
            a1 = 1.0 - y * y
            a2 = -2.0 * y * a1
        dy = a1 * dz
        fc, dfc = 0.5 * torch.cos(k * rr) + 0.5, -0.5 * k * torch.sin(k * rr)
        a = (dd * (Qt[jj] - Qt[ii])).sum(1) / rr
        A = Vt[jj] * gt[ii] + Vt[ii] * gt[jj]
        B = xt[jj] * gt[ii] + xt[ii] * gt[jj]
        p = fc[:, None] * A + (a * dfc)[:, None] * B
        q = (a * fc)[:, None] * B
        Pa, Ra = p @ w2, q @ w2
        t = a1 * Pa + a2 * dz * Ra
        td = a1 * Ra
        db2 += p.sum(0)
        dw2 += p.T @ y + q.T @ dy
        db1 += t.sum(0)
        dw1 += t.T @ gamma + td.T @ dgamma
    return dict(w1=dw1.numpy(), b1=db1.numpy(), w2=dw2.numpy(), b2=db2.numpy())


def witness(J, i, j, d, x, g, V, Q):
    return closed_form(J, i, j, np.asarray(d, np.float64).astype(np.float32), x, g, V, Q, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------- the table
# kernel: which kernel the layer takes (by the width and LDS alone): "mfma" = cfconv_wgrad2_mfma (W a multiple of 16 up to 128, the
#   kernel's LDS image -- W2, W1^T, six [16][W + 16] tiles, two [16][64 or 256] Gaussian tiles -- inside 160 KiB), "vector" else
# cot: the cotangents given: "VQ", "V" (Q = NULL) or "Q" (V = NULL)
Case = collections.namedtuple("Case", "name W G act frame kernel cot")


def _cases():
    t = []

    def add(name, W, G, kernel, frame="conformer90", acts=dispatch.BOTH, cot="VQ"):
        for act in acts:
            t.append(Case(f"{name}-{act}", W, G, act, frame, kernel, cot))

    # layers (conformer90: 2 493 pairs = 155 full tiles of 16 and one of 13 pairs)
    add("w1_g10", 1, 10, "vector")
    add("w8_g10", 8, 10, "vector")
    add("w24_g10", 24, 10, "vector")
    add("w16_g8", 16, 8, "mfma")                            # one wave
    add("w48_g7", 48, 7, "mfma")                            # odd block count, G below one k-step of 4
    add("w32_g50", 32, 50, "mfma")
    add("w64_g50", 64, 50, "mfma")
    add("w128_g50", 128, 50, "mfma")                        # the SchNet layer
    add("w136_g10", 136, 10, "vector")                      # beyond the matrix-core widths
    # 4 or 16 blocks of Gaussians (G = 64 | 65), and at W = 128 the last G whose image fits in LDS
    # (16384 + 64 * 128 + 6 * 16 * 144 + 2 * 16 * 64 + 96 floats = 158.4 KiB) and the first that does not (G = 65: sixteen blocks, 184.9 KiB)
    add("w32_g64_four_blocks", 32, 64, "mfma")
    add("w32_g65_sixteen_blocks", 32, 65, "mfma")
    add("w128_g64_last_mfma", 128, 64, "mfma")
    add("w128_g65_first_vector", 128, 65, "vector")
    # the cotangents one at a time, on one layer of each kernel
    for cot in ("V", "Q"):
        add(f"w32_g50_{cot}_only", 32, 50, "mfma", acts=("ssp",), cot=cot)
        add(f"w24_g10_{cot}_only", 24, 10, "vector", acts=("tanh",), cot=cot)
    # pair counts around the tile of each kernel
    for P in (0, 1, TILE - 1, TILE, TILE + 1):
        add(f"chain{P}_w16_g8", 16, 8, "mfma", frame=f"chain:{P}", acts=("ssp",))
        add(f"chain{P}_w24_g10", 24, 10, "vector", frame=f"chain:{P}", acts=("tanh",))
    for P in (VECTOR_TILE - 1, VECTOR_TILE, VECTOR_TILE + 1):
        add(f"chain{P}_w24_g10", 24, 10, "vector", frame=f"chain:{P}", acts=("tanh",))
    # more pairs than one sweep of the launch (256 workgroups x 16 pairs), on a periodic frame whose rows the cell grid builds
    add("liquid1500_w32_g16", 32, 16, "mfma", frame="liquid1500", acts=("ssp",))
    add("liquid1500_w24_g10", 24, 10, "vector", frame="liquid1500", acts=("tanh",))
    assert len({c.name for c in t}) == len(t)
    return tuple(t)


CASES = _cases()


def expected_kernel(W, G):
    """the kernel of a layer, from the LDS formula written out by hand (cfconv_weight_grad_second.h: wgrad2_mfma_floats)"""
    if W % 16 or W > 128:
        return "vector"
    floats = W * W + (G + 3) // 4 * 4 * W + 6 * TILE * (W + 16) + 2 * TILE * (64 if G <= 64 else 256) + 6 * TILE
    return "mfma" if 4 * floats <= dispatch.LDS_LIMIT else "vector"


def inputs(case):
    """-> (pos, box, cutoff, (w1, b1, w2, b2), x, g, V, Q) of a case"""
    pos, box, cutoff = frame(case.frame)
    w1, b1, w2, b2, x, g = layer(case.frame, case.W, case.G)
    V, Q = cotangents(case.frame, case.W, case.cot)
    return pos, box, cutoff, (w1, b1, w2, b2), x, g, V, Q


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> dict(J, i, j, d, judge = the float64 gradients, witness = the float32 ones) of a case: computed once, read-only"""
    pos, box, cutoff, weights, x, g, V, Q = inputs(case)
    J = judge_of(case.W, case.G, cutoff, case.act, *weights)
    i, j, d = pair_displacements(J, pos, box)
    ref = dict(J=J, i=i, j=j, d=d, judge=judge(J, i, j, d, x, g, V, Q), witness=witness(J, i, j, d, x, g, V, Q))
    for part in (ref["judge"], ref["witness"]):
        for v in part.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return ref


# ---------------------------------------------------------------------------------------------- a force loss through stacked layers
def force_loss(J, params, i, j, pos, x, readout, E0, F0, shift=None):
    """(E - E0)^2 + |F - F0|^2 of E = <readout, layers(x)>, F = -dE/dpositions, in float64 over the fixed half list (i, j) with frozen
    shifts; `params`: 4 tensors per stacked layer (w1 [W][G], b1, w2, b2), differentiable.  -> (loss, E, F)"""
    p = wf._wide(pos).requires_grad_(True)
    it, jt = torch.as_tensor(i), torch.as_tensor(j)
    d = p[jt] - p[it]
    if shift is not None:
        d = d + torch.as_tensor(np.asarray(shift, np.float64))
    r = d.norm(dim=1)
    h = wf._wide(x)
    for k in range(0, len(params), 4):
        h = wf.layer_output(J, *params[k:k + 4], i, j, r, h)
    E = (h * wf._wide(readout)).sum()
    F = -torch.autograd.grad(E, p, create_graph=True)[0]
    return (E - E0) ** 2 + ((F - wf._wide(F0)) ** 2).sum(), E, F
