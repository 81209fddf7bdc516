"""The float64 judge of the fused atomic networks (mlp_fused.hip; no GPU code, no tests; importable anywhere) and the table of the
edge cases test_mlp_edges_gpu.py runs, with their seeded frames -- so the CPU file that pins the judge and the GPU file that uses it
see the same numbers.

The function is the reference's TorchANIBatchedNN (src/pytorch/BatchedNN.py:100-111): per atom and ensemble member
Linear(F,H1) CELU Linear(H1,H2) CELU Linear(H2,H3) CELU Linear(H3,1).  `judge` evaluates it in float64 and, as the float32 WITNESS,
once more in float32 torch on the CPU (never a kernel): what plain float32 arithmetic of the same sums loses is the yardstick the
kernels' split-fp16 arithmetic is held against, next to the project's fixed bars.  It returns the energies per (grouped atom, member)
and every member's own gradient G[m] = d(sum over atoms of e[:, m])/dx, so that everything the weighted kernels compute is linear algebra
on G in float64 (`combine`, `magnitude`: as ani_members_float64 does it, with the molecule of a row as one more index).
tests/test_mlp_reference_cpu.py pins the module.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

E_BAR, G_BAR = 1e-5, 1e-4           # the project's bars (test_mlp_fused_gpu.py, test_ani_members_gpu.py): of max |e|, of max |g|
G_FLOOR = 1e-3                      # a frame whose gradient is smaller than this judges nothing (a relative bar on denormals)


def networks(widths, members, features, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    h1, h2, h3 = widths
    def rnd(*shape, fan):
        return (scale * torch.randn(shape, generator=gen) / np.sqrt(fan)).float()
    return dict(w0=rnd(members, h1, features, fan=features), b0=0.1 * torch.randn((members, h1), generator=gen),
                w2=rnd(members, h2, h1, fan=h1), b2=0.1 * torch.randn((members, h2), generator=gen),
                w4=rnd(members, h3, h2, fan=h2), b4=0.1 * torch.randn((members, h3), generator=gen),
                w6=rnd(members, h3, fan=h3), b6=0.1 * torch.randn((members,), generator=gen))


def host_reference(kinds, x):
    """-> per (grouped atom, member) energies [n, M] and dE_total/dx [atoms, F], float64."""
    xd = x.double().requires_grad_(True)
    outs = []
    for kd in kinds:
        xs = xd[kd["atoms"].long()]
        per_member = []
        for m in range(kd["w0"].shape[0]):
            y = torch.nn.functional.celu(xs @ kd["w0"][m].double().t() + kd["b0"][m].double(), alpha=0.1)
            y = torch.nn.functional.celu(y @ kd["w2"][m].double().t() + kd["b2"][m].double(), alpha=0.1)
            y = torch.nn.functional.celu(y @ kd["w4"][m].double().t() + kd["b4"][m].double(), alpha=0.1)
            per_member.append(y @ kd["w6"][m].double() + kd["b6"][m].double())
        outs.append(torch.stack(per_member, dim=1))
    e = torch.cat(outs, dim=0)
    e.sum().backward()
    return e.detach(), xd.grad


def saturating_biases(kd, seed):
    """-> a copy of the networks `kd` whose hidden biases drive CELU into both of its ends: a quarter of them -4 (with alpha <= 0.1
    exp(v / alpha) underflows: the flat end, CELU' = 0), a quarter +2 (the linear end), the rest left N(0, 0.1).  (Shifting ALL of them
    down switches every unit off: the gradient falls to 1e-25 and a relative bar says nothing.)"""
    gen = torch.Generator().manual_seed(7000 + seed)
    out = dict(kd)
    for name in ("b0", "b2", "b4"):
        b = kd[name].clone()
        u = torch.rand(b.shape, generator=gen)
        b[u < 0.25] = -4.0
        b[(u >= 0.25) & (u < 0.5)] = 2.0
        out[name] = b
    return out


# ---------------------------------------------------------------------------------------------- the judge
def _evaluate(kinds, x, alpha, dtype):
    """-> e [n][M], G [M][atoms][F] in `dtype`: member m reads its own copy of x, so one backward pass gives every member's gradient"""
    M = kinds[0]["w0"].shape[0]
    xm = x.to(dtype).unsqueeze(0).repeat(M, 1, 1).requires_grad_(True)
    outs = []
    for kd in kinds:
        y = xm[:, kd["atoms"].long()]                                      # [M][n][F]
        for w, b in (("w0", "b0"), ("w2", "b2"), ("w4", "b4")):
            y = torch.nn.functional.celu(torch.baddbmm(kd[b].to(dtype).unsqueeze(1), y, kd[w].to(dtype).transpose(1, 2)), alpha=alpha)
        outs.append(torch.einsum("mnh,mh->nm", y, kd["w6"].to(dtype)) + kd["b6"].to(dtype))
    e = torch.cat(outs, dim=0)
    if e.numel():
        e.sum().backward()
    return e.detach(), (xm.grad if xm.grad is not None else torch.zeros_like(xm)).detach()


Judgement = namedtuple("Judgement", "e G e32 G32")       # float64 numpy e [n][M], G [M][atoms][F]; the float32 witness's (as float32)


def judge(kinds, x, alpha=0.1):
    """kinds: dicts of float32 CPU tensors as capi.FusedMLP takes them (w0 [M,H1,F] ... b6 [M], atoms: rows of x); x [atoms][F] float32.
    -> Judgement; arrays are read-only."""
    assert x.dtype == torch.float32 and all(kd["w0"].dtype == torch.float32 for kd in kinds)
    e, G = _evaluate(kinds, x, alpha, torch.float64)
    e32, G32 = _evaluate(kinds, x, alpha, torch.float32)
    out = Judgement(e.numpy(), G.numpy(), e32.numpy(), G32.numpy())
    for a in out:
        a.setflags(write=False)
    return out


def molecule_of_rows(offsets, rows):
    """offsets [B + 1] (rows offsets[b] .. offsets[b + 1] - 1 of x are molecule b) -> the molecule of every row in `rows`"""
    offsets = np.asarray(offsets)
    rows = np.asarray(rows)
    assert offsets[0] == 0 and (np.diff(offsets) >= 0).all() and (rows < offsets[-1]).all(), "a row outside the molecules"
    return np.searchsorted(offsets[1:], rows, side="right")


def combine(w, G, mol=None):
    """the gradient of sum_b sum_m w[b][m] E_m(molecule b): w [M], or [B][M] with mol [atoms] (the molecule of every row of x);
    G [M][atoms][F] -> [atoms][F], in G's precision (float64 for the judge; float32, members added in order, for the witness)"""
    w = np.asarray(w, dtype=G.dtype)
    per_row = np.broadcast_to(w[:, None], (G.shape[0], G.shape[1])) if mol is None else w[np.asarray(mol)].T      # [M][atoms]
    out = np.zeros(G.shape[1:], dtype=G.dtype)
    for m in range(G.shape[0]):
        out += per_row[m][:, None] * G[m]
    return out


def magnitude(w, G, mol=None):
    """the largest entry of sum_m |w_m| |G_m|: the scale a rounding error of the parts is measured against"""
    return float(combine(np.abs(np.asarray(w, dtype=np.float64)), np.abs(np.asarray(G, dtype=np.float64)), mol).max())


def ones(J):
    return np.ones(J.G.shape[0])


Errors = namedtuple("Errors", "e_scale g_ref g_scale e32 g32")


def reference(J, w=None, mol=None):
    """-> Errors: max |e|, the float64 gradient of the (weighted) sum with its scale, and the float32 witness's errors on both"""
    w = ones(J) if w is None else w
    g_ref = combine(w, J.G, mol)
    g32 = combine(w, J.G32, mol)
    return Errors(float(np.abs(J.e).max()) if J.e.size else 0.0, g_ref, magnitude(w, J.G, mol),
                  float(np.abs(J.e32.astype(np.float64) - J.e).max()) if J.e.size else 0.0, float(np.abs(g32.astype(np.float64) - g_ref).max()))


def check_frame(J):
    """what a frame must be to judge anything: finite, a gradient of size, and a float32 witness ten times inside the project's bars"""
    assert np.isfinite(J.e).all() and np.isfinite(J.G).all() and np.isfinite(J.e32).all() and np.isfinite(J.G32).all()
    r = reference(J)
    assert float(np.abs(r.g_ref).max()) >= G_FLOOR, float(np.abs(r.g_ref).max())
    assert r.e32 <= 0.1 * E_BAR * r.e_scale, (r.e32, r.e_scale)
    assert r.g32 <= 0.1 * G_BAR * r.g_scale, (r.g32, r.g_scale)
    return r


def random_weights(batch, members, seed):
    """[batch][members] float32 in [-1, 1]: both signs in every row (where there are two members), and one exact zero per row
    (where there are three) -- a member the weighted kernels skip"""
    w = np.random.default_rng(3000 + seed).uniform(-1.0, 1.0, (batch, members)).astype(np.float32)
    w[:, 0] = np.abs(w[:, 0])
    if members >= 2:
        w[:, -1] = -np.abs(w[:, -1])
    if members >= 3:
        for b in range(batch):
            w[b, 1 + (b + seed) % (members - 2)] = 0.0
    return w


# ---------------------------------------------------------------------------------------------- the cases of test_mlp_edges_gpu.py
# One kind of 70 atoms (a full tile and six atoms) on a shuffled subset of the 80 rows of x, two members, widths (96, 64, 32),
# alpha 0.1, act_scale_log2 4 and inputs N(0, 1) unless the case says otherwise.
ROWS = 80
MOLECULES = (0, 20, 21, 70)          # section c, weights per molecule: a tile holds atoms of all three
Case = namedtuple("Case", "name section F widths M counts alpha k saturate x_width live seed",
                  defaults=((96, 64, 32), 2, (70,), 0.1, 4, False, None, None, 0))

A_FEATURES = (8, 16, 24, 32, 40, 64, 72, 96, 128, 136, 160, 192, 200, 224, 1000, 1024)
B_WIDTHS = ((32, 32, 32), (64, 256, 32), (256, 32, 256), (128, 160, 224), (224, 128, 64), (160, 96, 192), (192, 224, 96), (96, 64, 160),
            (64, 192, 128), (256, 256, 256), (8, 40, 17), (33, 65, 129), (250, 100, 10))
C_MEMBERS = ((1, 32), (2, 32), (3, 32), (5, 32), (3, 64), (7, 32), (5, 96), (128, 32))
C_LIVE = (1, 4, 6, 9)               # section c and d, live_groups route: F = 64 as four live 16-column blocks of a 160-column x
E_SHAPES = ((96, (64, 64, 64)), (40, (32, 96, 32)))
E_ALPHAS = (0.05, 0.1, 1.0)
E_SCALES = (4, 12)
F_COUNTS = (0, 64, 1, 0, 65, 63, 2, 0)
F_WIDTHS = ((32, 32, 32), (64, 32, 96), (32, 64, 32), (96, 32, 64), (40, 96, 32), (64, 64, 17), (32, 33, 64), (64, 32, 32))


def _cases():
    out = []
    for i, F in enumerate(A_FEATURES):
        out.append(Case(f"a-F{F}", "a", F, seed=100 + i))
    for i, widths in enumerate(B_WIDTHS):
        out.append(Case("b-" + "x".join(map(str, widths)), "b", 96, widths=widths, M=3, counts=(65,), seed=200 + i))
    for i, (M, h1) in enumerate(C_MEMBERS):
        out.append(Case(f"c-M{M}-h{h1}", "c", 64, widths=(h1, 64, 32), M=M, seed=300 + i))
        if M != 128:
            out.append(Case(f"c-M{M}-h{h1}-live", "c", 64, widths=(h1, 64, 32), M=M, x_width=160, live=C_LIVE, seed=320 + i))
    out.append(Case("d-separate", "d", 64, seed=400))
    out.append(Case("d-live", "d", 64, x_width=160, live=C_LIVE, seed=401))
    i = 0
    for F, widths in E_SHAPES:
        for alpha in E_ALPHAS:
            for k in E_SCALES:
                out.append(Case(f"e-F{F}-alpha{alpha}-k{k}", "e", F, widths=widths, alpha=alpha, k=k, saturate=True, seed=500 + i))
                i += 1
    out.append(Case("f-eight-kinds", "f", 40, widths=F_WIDTHS, counts=F_COUNTS, seed=600))
    return {c.name: c for c in out}


CASES = _cases()


def section(letter, live=None):
    return [c.name for c in CASES.values() if c.section == letter and (live is None or (c.live is not None) == live)]


Frame = namedtuple("Frame", "case kinds x columns J")    # kinds as FusedMLP takes them (w0 over all x_width columns); x [rows][x_width];
                                                         # columns: where the F features live in x; J: the judgement over those columns


@functools.lru_cache(maxsize=None)
def frame(name):
    """the seeded networks and inputs of a case, and its judgement: computed once, not changed"""
    c = CASES[name]
    gen = torch.Generator().manual_seed(c.seed)
    n = sum(c.counts)
    rows = max(ROWS, n + 10)
    x_width = c.x_width or c.F
    # section c: the atoms are rows 0 .. 69 shuffled, so that every atom lies inside MOLECULES; otherwise any of the rows
    perm = torch.randperm(n if c.section == "c" else rows, generator=gen)[:n]
    x = torch.randn((rows, x_width), generator=gen)
    widths = c.widths if isinstance(c.widths[0], tuple) else (c.widths,) * len(c.counts)
    kinds, first = [], 0
    for s, (w, count) in enumerate(zip(widths, c.counts)):
        kd = networks(w, c.M, x_width, seed=c.seed * 10 + s)
        if c.saturate:
            kd = saturating_biases(kd, c.seed * 10 + s)
        kd["atoms"] = perm[first:first + count].to(torch.int32)
        first += count
        kinds.append(kd)
    columns = torch.arange(c.F) if c.live is None else torch.tensor([16 * g + i for g in c.live for i in range(16)])
    judged = [dict(kd, w0=kd["w0"][:, :, columns].contiguous()) for kd in kinds]
    J = judge(judged, x[:, columns].contiguous(), alpha=c.alpha)
    check_frame(J)
    return Frame(c, kinds, x, columns, J)
