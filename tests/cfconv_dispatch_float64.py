"""The frames and the dispatch table of the CFConv dispatch tests (no GPU code, no tests; importable anywhere).

nnpops_cfconv_create chooses among four kernel families -- the vector kernel, the filters kernel on the fp32 matrix instruction, the
split-fp16 filters kernel through LDS planes and the register-fed split-fp16 pair -- from the width W, the number of Gaussians G, the
weights and three LDS-fit formulas.  TABLE lists one row per edge of that choice with the plan each row is EXPECTED to get (path,
waves per workgroup forward / backward; on the vector path channels per lane and where each direction keeps its weights), written
down by hand from the formulas, not computed by them: tests/test_cfconv_dispatch_reference_cpu.py holds nnpops_cfconv_plan against
it, tests/test_cfconv_dispatch_gpu.py holds the handle's describe() against it and the numbers against cfconv_float64.Restatement.

Frames (cutoff 5 unless the row says otherwise; float32, read-only):
    conformer90   workloads.conformer(90, seed=7): 2 493 pairs, rows of 15 to 80 entries (above 64: the row capacity grows once)
    chain:P       P + 1 atoms along x, seeded spacings in [0.56 c, 0.94 c], +-0.05 jitter in y and z: only neighbours pair, exactly P pairs
                  (P = 0: two atoms 2 c apart)
    blob:n        n atoms in a sphere of radius 0.49 c, no two closer than 0.7: every atom sees every other, rows of exactly n - 1 entries
    atom1         one atom: no pair at all
    box1000c10    workloads.random_box(1000, density=0.1, seed=13), periodic, cutoff 10: ~210 000 pairs, more than one sweep of the
                  forward register kernel's grid (256 workgroups x 8 waves x 32 pairs)
Weights, input and output gradient of a case are seeded by the shape alone (cfconv_float64.weights with seed 1000 W + G), as
cfconv_float64.layer seeds them.
"""
import collections
import functools

import numpy as np

from cfconv_float64 import sigma_of, weights
from nnpops_amd import workloads

CUTOFF = 5.0
FAR_BOX = np.eye(3, dtype=np.float32) * np.float32(1000.0)      # what the judge is given for a frame in vacuum: no image is ever nearer
LDS_LIMIT = 160 * 1024                                           # bytes a workgroup of gfx950 can ask for
VECTOR_LDS_LIMIT = 156 * 1024                                    # what the vector kernel's launch budgets


# ---------------------------------------------------------------------------------------------- frames
def _chain(P, cutoff=CUTOFF):
    rng = np.random.default_rng(4000 + P)
    if P == 0:
        return np.array([[0, 0, 0], [2 * cutoff, 0, 0]], dtype=np.float32)
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.56 * cutoff, 0.94 * cutoff, P))])
    yz = rng.uniform(-0.05, 0.05, (P + 1, 2))
    return np.concatenate([x[:, None], yz], axis=1).astype(np.float32)


def _blob(n, cutoff=CUTOFF, min_dist=0.7):
    """random sequential addition, seeded; the margin of 0.01 on both bounds outlives the rounding to float32"""
    rng = np.random.default_rng(5000 + n)
    radius = 0.49 * cutoff - 0.01
    pts = np.zeros((0, 3))
    while len(pts) < n:
        for c in rng.uniform(-radius, radius, (4096, 3)):
            if c @ c <= radius * radius and (len(pts) == 0 or ((pts - c) ** 2).sum(axis=1).min() >= (min_dist + 0.01) ** 2):
                pts = np.concatenate([pts, c[None]])
                if len(pts) == n:
                    break
    return pts.astype(np.float32)


@functools.lru_cache(maxsize=None)
def frame(tag):
    """-> (pos float32 [N][3], box float32 [3][3] or None, cutoff)"""
    box, cutoff = None, CUTOFF
    if tag == "conformer90":
        pos, _ = workloads.conformer(90, seed=7)
    elif tag.startswith("chain:"):
        pos = _chain(int(tag[6:]))
    elif tag.startswith("blob:"):
        pos = _blob(int(tag[5:]))
    elif tag == "atom1":
        pos = np.zeros((1, 3), dtype=np.float32)
    elif tag == "box1000c10":
        pos, _, box = workloads.random_box(1000, density=0.1, seed=13)
        cutoff = 10.0
    else:
        raise KeyError(tag)
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    for a in (pos, box):
        if a is not None:
            a.setflags(write=False)
    return pos, box, cutoff


SMALL_FRAMES = (["conformer90", "atom1"] + [f"chain:{P}" for P in (0, 1, 15, 16, 17, 31, 32, 33)]
                + [f"blob:{n}" for n in (2, 8, 9, 10, 64, 65, 66, 129, 130)])


def layer(tag, W, G):
    """-> (w1, b1, w2, b2, x, gout) of a layer on a frame, seeded by the shape"""
    return weights(W, G, len(frame(tag)[0]), 1000 * W + G)


# ---------------------------------------------------------------------------------------------- the table
# env: the NNPOPS_CFCONV_* switches of the row (the environment is cleaned of the family's switches first).
# cpl / wlds: vector path only -- channels per lane, (forward, backward) weights in LDS.
# grows: the frame's longest row exceeds the initial capacity of 64 entries -- the first check() must report it.
Row = collections.namedtuple("Row", "name W G frame acts env path waves_fwd waves_bwd cpl wlds grows")
BOTH = ("ssp", "tanh")
REG, PLANES, MATRIX, VECTOR = "split_registers", "split_planes", "matrix", "vector"


def _row(name, W, G, path, wf, wb, frame="conformer90", acts=None, env=None, cpl=0, wlds=(False, False), grows=None):
    if acts is None:            # every matrix-core row under both activations; the vector rows alternate
        acts = BOTH if path != VECTOR else (("ssp",) if (W + G) % 2 == 0 else ("tanh",))
    if grows is None:
        grows = frame == "conformer90" or frame == "box1000c10" or (frame.startswith("blob:") and int(frame[5:]) > 65)
    return Row(name, W, G, frame, tuple(acts), dict(env or {}), path, wf, wb, cpl, tuple(wlds), grows)


def _table():
    t = []
    # layer-1 K steps of the register-fed kernels (the Gaussians and the bias column k = G share 32-wide steps) and where they end
    t += [_row("w32_g2_smallest", 32, 2, REG, 8, 8), _row("w32_g31_one_step", 32, 31, REG, 8, 8),
          _row("w32_g32_bias_alone", 32, 32, REG, 8, 8), _row("w32_g63_two_steps", 32, 63, REG, 8, 8),
          _row("w32_g64_planes", 32, 64, PLANES, 8, 8)]
    t += [_row("w64_g63", 64, 63, REG, 8, 8), _row("w64_g64_planes", 64, 64, PLANES, 8, 8)]
    t += [_row("w96_g63", 96, 63, REG, 8, 4), _row("w96_g64_planes", 96, 64, PLANES, 8, 8)]
    # W = 128: the LDS condition ends the register path at G = 55; the plane kernel thins out to one wave; one shape on the fp32 matrix
    # kernel with a single wave; then the vector kernel with streamed weights
    t += [_row("w128_g55_last_registers", 128, 55, REG, 8, 4), _row("w128_g56_planes_7_waves", 128, 56, PLANES, 7, 7),
          _row("w128_g155_planes_2_waves", 128, 155, PLANES, 2, 2), _row("w128_g171_planes_1_wave", 128, 171, PLANES, 1, 1),
          _row("w128_g172_matrix_1_wave", 128, 172, MATRIX, 1, 1),
          _row("w128_g173_vector_streamed", 128, 173, VECTOR, 8, 8, cpl=2)]
    # odd numbers of column blocks: the fp32 matrix kernel only
    t += [_row("w16_g2", 16, 2, MATRIX, 8, 8), _row("w16_g5_padded_k", 16, 5, MATRIX, 8, 8), _row("w16_g256", 16, 256, MATRIX, 8, 8),
          _row("w48_g7", 48, 7, MATRIX, 8, 8), _row("w80_g256", 80, 256, MATRIX, 8, 8),
          _row("w112_g236_last_matrix", 112, 236, MATRIX, 1, 1), _row("w112_g237_vector", 112, 237, VECTOR, 8, 7, cpl=2)]
    # the vector kernel: one to eight channels per lane, dead lanes, weights in LDS or streamed
    t += [_row("w1_g2", 1, 2, VECTOR, 8, 8, cpl=1, wlds=(True, True)), _row("w63_g10", 63, 10, VECTOR, 8, 8, cpl=1, wlds=(True, True)),
          # W = 64 is a multiple of 32: without a switch it takes the register-fed kernels; the vector kernel with every lane live is forced
          _row("w64_g10_default", 64, 10, REG, 8, 8),
          _row("w64_g10_vector", 64, 10, VECTOR, 8, 8, env={"NNPOPS_CFCONV_VALU": "1"}, cpl=1, wlds=(True, True)),
          _row("w65_g10", 65, 10, VECTOR, 8, 8, cpl=2, wlds=(True, True)), _row("w127_g10", 127, 10, VECTOR, 8, 8, cpl=2, wlds=(True, True)),
          _row("w129_g10", 129, 10, VECTOR, 8, 8, cpl=4), _row("w256_g10", 256, 10, VECTOR, 8, 8, cpl=4),
          _row("w257_g10_fifth_slot", 257, 10, VECTOR, 8, 8, cpl=8), _row("w512_g256_maxima", 512, 256, VECTOR, 6, 3, cpl=8),
          _row("w100_g256_two_instantiations", 100, 256, VECTOR, 1, 6, cpl=2, wlds=(True, False))]
    # forced paths
    for W in (32, 64, 96, 128):
        t.append(_row(f"w{W}_g16_split0", W, 16, MATRIX, 8, 8, env={"NNPOPS_CFCONV_SPLIT": "0"}))
        t.append(_row(f"w{W}_g16_split1", W, 16, PLANES, 8, 8, env={"NNPOPS_CFCONV_SPLIT": "1"}))
    # pair counts around the tiles of the filters kernels (16 or 32 pairs), rows around the tile of the vector kernel (8 entries) and
    # around the row capacities (64 -> 128 -> 256)
    filters_layers = [(32, 16, REG, 8, 8), (32, 70, PLANES, 8, 8), (16, 8, MATRIX, 8, 8), (96, 16, REG, 8, 4)]
    for P in (0, 1, 15, 16, 17, 31, 32, 33):
        for W, G, path, wf, wb in filters_layers:
            t.append(_row(f"chain{P}_w{W}_g{G}", W, G, path, wf, wb, frame=f"chain:{P}"))
    for W, G, path, wf, wb in filters_layers + [(24, 10, VECTOR, 8, 8)]:
        kw = dict(cpl=1, wlds=(True, True)) if path == VECTOR else {}
        t.append(_row(f"atom1_w{W}_g{G}", W, G, path, wf, wb, frame="atom1", **kw))
    for n in (2, 8, 9, 10):
        t.append(_row(f"blob{n}_w24_g10", 24, 10, VECTOR, 8, 8, frame=f"blob:{n}", cpl=1, wlds=(True, True)))
    for n in (64, 65, 66, 129, 130):
        for W, G, path, wf, wb in [(128, 50, REG, 8, 4), (32, 16, REG, 8, 8), (16, 8, MATRIX, 8, 8), (24, 10, VECTOR, 8, 8)]:
            kw = dict(cpl=1, wlds=(True, True)) if path == VECTOR else {}
            t.append(_row(f"blob{n}_w{W}_g{G}", W, G, path, wf, wb, frame=f"blob:{n}", **kw))
    # more pairs than one sweep of the grid
    t += [_row("sweep_w128_g50", 128, 50, REG, 8, 4, frame="box1000c10", acts=("ssp",)),
          _row("sweep_w128_g56", 128, 56, PLANES, 7, 7, frame="box1000c10", acts=("ssp",))]
    assert len({r.name for r in t}) == len(t)
    return tuple(t)


TABLE = _table()
CASES = tuple((r, act) for r in TABLE for act in r.acts)


def case_id(case):
    return f"{case[0].name}-{case[1]}"


def expected_plan(row):
    """the part of capi.cfconv_plan's dict the table states"""
    e = dict(path=row.path, waves_fwd=row.waves_fwd, waves_bwd=row.waves_bwd)
    if row.path == VECTOR:
        e.update(channels_per_lane=row.cpl, weights_in_lds_fwd=row.wlds[0], weights_in_lds_bwd=row.wlds[1])
    else:
        e.update(channels_per_lane=0, weights_in_lds_fwd=False, weights_in_lds_bwd=False)
    return e


def path_switches(W):
    """{G: path} -- where, by the table's rows without a switch, the path of width W changes between G - 1 and G"""
    rows = sorted((r.G, r.path) for r in TABLE if r.W == W and not r.env)
    return {g: p for (g0, p0), (g, p) in zip(rows, rows[1:]) if g == g0 + 1 and p != p0}


def plan_of(row, act):
    """capi.cfconv_plan of a row's layer (host arithmetic; the caller has set the row's environment)"""
    from nnpops_amd import capi
    w1, b1, w2, _, _, _ = layer(row.frame, row.W, row.G)
    return capi.cfconv_plan(row.W, row.G, sigma_of(row.G), act, w1, b1, w2)


# ---------------------------------------------------------------------------------------------- judging
def bar_fractions(out, ref_out, rtol, atol_frac):
    """largest |a - ref| / (rtol |ref| + atol_frac max|ref|) over the elements (0 for two all-zero arrays)"""
    ref = np.asarray(ref_out, dtype=np.float64)
    top = float(np.abs(ref).max()) if ref.size else 0.0
    if top == 0.0:
        return 0.0 if not np.any(out) else float("inf")
    return float((np.abs(np.asarray(out, dtype=np.float64) - ref) / (rtol * np.abs(ref) + atol_frac * top)).max())


def force_error(g, ref_g):
    """max |g - ref| / max |ref| (0 for two all-zero arrays)"""
    ref = np.asarray(ref_g, dtype=np.float64)
    top = float(np.abs(ref).max()) if ref.size else 0.0
    if top == 0.0:
        return 0.0 if not np.any(g) else float("inf")
    return float(np.abs(np.asarray(g, dtype=np.float64) - ref).max()) / top


ENERGY_RTOL = 1e-5      # L = <gout, out> to this fraction of sum |gout out|


def measure(ref, gout, out=None, gx=None, gp=None):
    """What a result is judged by, each as a fraction of its bar (cfconv_float64's OUT_RTOL, OUT_ATOL_FRAC, FORCE_RTOL): `out` and `gx`
    element-wise, L = <gout, out> against sum |gout out|, `gp` against the largest component; `force` is the raw relative figure."""
    from cfconv_float64 import FORCE_RTOL, OUT_ATOL_FRAC, OUT_RTOL
    fig = {}
    if out is not None:
        fig["out"] = bar_fractions(out, ref["out"], OUT_RTOL, OUT_ATOL_FRAC)
        g64 = np.asarray(gout, dtype=np.float64)
        scale = float(np.abs(g64 * ref["out"]).sum())
        L = float((g64 * np.asarray(out, dtype=np.float64)).sum())
        fig["L"] = abs(L - ref["L"]) / (ENERGY_RTOL * scale) if scale > 0 else (0.0 if L == 0.0 else float("inf"))
    if gx is not None:
        fig["gx"] = bar_fractions(gx, ref["gx"], OUT_RTOL, OUT_ATOL_FRAC)
    if gp is not None:
        fig["force"] = force_error(gp, ref["g"])
        fig["gp"] = fig["force"] / FORCE_RTOL
    return fig


def within(fig, fraction=1.0):
    """every judged figure inside `fraction` of its bar (and a number at all)"""
    return all(np.isfinite(v) and v <= fraction for k, v in fig.items() if k != "force")


def figures(fig):
    return " ".join(f"{k} {v:.2e}" if k == "force" else f"{k} {v:.3f}" for k, v in fig.items())
