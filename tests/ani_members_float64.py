"""The float64 judge of the per-member energies of an ANI ensemble (no GPU code, no tests; importable anywhere), and the inputs of
its tests -- the ones of test_ani_batch_energy_gpu.py, rebuilt here: workloads.conformer(23) with its species overwritten ("HCNO": 11 H,
7 C, 1 N, 4 O; "HCO": 12 H, 7 C, 4 O), 67 conformers jittered by up to 0.1 A, the batch of five at slots 60, 3, 17, 41, 66, the
70-atom molecule, and torchani_like_model(seed=12) with 3, 8 or 2 members.

`judge_frames` evaluates, per frame, E[m] of every member WITHOUT the self energy -- the networks per species in float64 on the
oracle's AEV, as the mean's judge does -- and dE_m/dpositions [M][n][3], one oracle.backward per member.  Everything else is linear
algebra on those in float64: a weighted combination sum_m w_m E_m has the gradient sum_m w_m G_m, and sigma = std(E_1..E_M) has
d sigma / dE_m = (E_m - mean) / ((M - ddof) sigma).  tests/test_ani_members_reference_cpu.py pins the module.
"""
import functools

import numpy as np
import torch

from nnpops_amd import workloads
from oracle import AniOracle

SAE = [-0.5, -38.0, -54.7, -75.2, -398.1, -99.8, -460.1]
SLOTS = [60, 3, 17, 41, 66]
SYMS = list(workloads.ANI2X_WIDTHS)


@functools.lru_cache(maxsize=None)
def molecule(n_atoms, count, kinds="HCNO"):
    """-> (species [n], conformers [count][n][3] float32); the conformers do not depend on `kinds`"""
    base, species = workloads.conformer(n_atoms, seed=40 + n_atoms)
    if n_atoms == 23:
        species = np.array({"HCNO": [0] * 11 + [1] * 7 + [2] + [3] * 4, "HCO": [0] * 12 + [1] * 7 + [3] * 4}[kinds], dtype=np.int32)
        species = species[np.random.default_rng(5).permutation(23)]
    rng = np.random.default_rng(100 + n_atoms)
    confs = np.stack([base + rng.uniform(-0.1, 0.1, base.shape).astype(np.float32) for _ in range(count)]).astype(np.float32)
    return species, confs


@functools.lru_cache(maxsize=None)
def model_of(members=3, seed=12):
    return workloads.torchani_like_model(n_models=members, seed=seed, self_energies=SAE)


@functools.lru_cache(maxsize=None)
def periodic_frame():
    """-> (species [100], positions, box): a cubic box of L = 10.8 A, more than twice the radial cutoff, all seven species"""
    pos, species, box = workloads.random_box(100, density=0.08, seed=6)
    return species, pos, box


def self_energy(species):
    return float(sum(SAE[s] for s in species))


def member_energies(nets, species, aev):
    """nets: per member a dict symbol -> float64 network; aev [n][1008] float64 tensor -> tensor [M], every member's sum over the atoms"""
    out = []
    for member in nets:
        total = 0
        for s in sorted(set(species.tolist())):
            idx = torch.tensor(np.nonzero(species == s)[0])
            total = total + member[SYMS[s]](aev[idx]).sum()
        out.append(total)
    return torch.stack(out)


def judge_frames(species, frames, model, box=None, oracle_cls=AniOracle, gradients=True):
    """-> E [frames][M] float64 (no self energy) and G [frames][M][n][3] float64 = dE_m/dpositions (None without `gradients`)"""
    species = np.asarray(species)
    n = len(species)
    oracle = oracle_cls(7, 5.1, 3.5, species, *workloads.ani2x_functions(), periodic=box is not None)
    nets = [{sym: net.double() for sym, net in member.items()} for member in model.neural_networks]
    E = np.empty((len(frames), len(nets)))
    G = np.empty((len(frames), len(nets), n, 3)) if gradients else None
    try:
        for b, pos in enumerate(frames):
            r_ref, a_ref = oracle.forward(pos, box) if box is not None else oracle.forward(pos)
            aev = torch.tensor(np.concatenate([r_ref, a_ref], axis=1), dtype=torch.float64, requires_grad=gradients)
            e = member_energies(nets, species, aev)
            E[b] = e.detach().numpy()
            for m in range(len(nets) if gradients else 0):
                g = torch.autograd.grad(e[m], aev, retain_graph=True)[0].numpy()
                if oracle_cls is AniOracle:
                    g = g.astype(np.float32)
                G[b, m] = oracle.backward(np.ascontiguousarray(g[:, :112]), np.ascontiguousarray(g[:, 112:]))
    finally:
        for member in model.neural_networks:
            member.float()
    return E, G


@functools.lru_cache(maxsize=None)
def judge(n_atoms, count, kinds="HCNO", members=3, picks=None):
    """the conformers `picks` (a tuple; None: all `count`) of molecule(n_atoms, count, kinds) under model_of(members); computed once,
    not changed"""
    species, confs = molecule(n_atoms, count, kinds)
    frames = confs if picks is None else confs[list(picks)]
    E, G = judge_frames(species, frames, model_of(members))
    E.setflags(write=False)
    G.setflags(write=False)
    return E, G


# ---------------------------------------------------------------------------------------------- linear algebra on the judge
def combine(w, G):
    """w [M], G [M][n][3] -> the gradient of sum_m w_m E_m"""
    return np.einsum("m,mnc->nc", np.asarray(w, dtype=np.float64), G)


def magnitude(w, G):
    """the largest entry of sum_m |w_m| |G_m|: the scale a rounding error of the parts is measured against"""
    return float(np.einsum("m,mnc->nc", np.abs(np.asarray(w, dtype=np.float64)), np.abs(G)).max())


def sigma(E, unbiased=True):
    """E [..., M] -> the standard deviation over the members"""
    return np.std(np.asarray(E, dtype=np.float64), axis=-1, ddof=1 if unbiased else 0)


def sigma_weights(E, unbiased=True):
    """E [M] -> d sigma / dE_m [M]"""
    E = np.asarray(E, dtype=np.float64)
    return (E - E.mean()) / ((len(E) - (1 if unbiased else 0)) * sigma(E, unbiased))


def random_weights(batch, members, seed):
    """[batch][members] in [-1, 1], a different row per conformer, both signs in every row"""
    w = np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, (batch, members))
    w[:, 0], w[:, -1] = np.abs(w[:, 0]), -np.abs(w[:, -1])
    return w
