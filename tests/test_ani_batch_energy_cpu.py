"""The batched energy step of OptimizedTorchANI: what exists without a GPU, and what pins the float64 judge of the segmented mean,
`segment_means` of tests/ani_float64.py (CPU only).

What pins it: a direct per-molecule sum over a random grouping with unequal molecule sizes (one empty, one larger than 64 atoms).  Both
sides are float64 sums of the same numbers in different orders: bar 1e-13 of the sum of the absolute values.
"""
import ctypes

import numpy as np
import torch

from ani_float64 import random_grouping, segment_means


def test_judge_is_the_per_molecule_sum():
    sizes = [23, 1, 70, 0, 64, 65, 7]
    members = 3
    energies, rows, places, offsets, _ = random_grouping(sizes, 4, members, 11)
    by_row = np.empty_like(energies, dtype=np.float64)
    by_row[rows] = energies                                   # the energy of every ROW: undo the grouping
    got = segment_means(energies, places, offsets, 1.0 / members)
    first = 0
    for b, size in enumerate(sizes):
        own = by_row[first:first + size]
        want = sum(float(v) for v in own.reshape(-1)) / members
        assert abs(got[b] - want) <= 1e-13 * max(float(np.abs(own).sum()), 1.0), (b, got[b], want)
        first += size
    assert got[3] == 0.0 and len(got) == len(sizes)


def test_library_exports_the_segment_entries_and_reports_null_pointers():
    from nnpops_amd import capi
    L = capi.lib()
    null = ctypes.c_void_p()
    for name in ("nnpops_mlp_energy_mean_segments", "nnpops_mlp_energy_mean_segments_shifted", "nnpops_scale_by_segment"):
        assert hasattr(L, name) and name in capi.SIGNATURES
    assert L.nnpops_mlp_energy_mean_segments(null, null, 8, 2, null, 1, null, 0.5, null) < 0 and b"NULL" in L.nnpops_last_error()
    assert L.nnpops_mlp_energy_mean_segments_shifted(null, null, 8, 2, null, 1, null, 0.5, null, null) < 0 and b"NULL" in L.nnpops_last_error()
    assert L.nnpops_scale_by_segment(null, null, 8, null, 1, null, 0, null) < 0 and b"NULL" in L.nnpops_last_error()
    # an empty batch is refused before any pointer is looked at twice
    one = ctypes.c_void_p(16)
    assert L.nnpops_mlp_energy_mean_segments(null, one, 8, 2, one, 0, one, 0.5, one) < 0 and b"empty batch" in L.nnpops_last_error()
    assert L.nnpops_scale_by_segment(null, one, 8, one, 0, one, 0, one) < 0 and b"empty batch" in L.nnpops_last_error()


def test_batch_ops_are_registered_with_their_tables():
    from nnpops_amd import torch_binding
    torch_binding.load()
    for name, returns in (("energy_batch", "-> Tensor"), ("energy_forces_batch", "-> (Tensor, Tensor)")):
        assert hasattr(torch.ops.NNPOpsANISymmetryFunctions, name)
        schema = str(getattr(torch.ops.NNPOpsANISymmetryFunctions, name).default._schema)
        assert "Tensor molecule_offsets" in schema and "Tensor row_positions" in schema and schema.endswith(returns), schema


def test_modules_have_the_batched_methods_and_still_script():
    from NNPOps import OptimizedTorchANI
    from nnpops_amd import workloads
    model = workloads.torchani_like_model(n_models=2, seed=3)
    _, species = workloads.conformer(23, seed=1)
    numbers = torch.tensor([[workloads.Z_OF_SPECIES[s] for s in species]])
    fused = OptimizedTorchANI(model, numbers)
    plain = OptimizedTorchANI(model, numbers, fused_step=False)
    assert type(fused).__name__ == "FusedOptimizedTorchANI" and type(plain).__name__ == "OptimizedTorchANI"
    assert callable(fused.forward_batch) and callable(plain.forward_batch) and callable(fused.energy_and_forces_batch)
    assert not hasattr(plain, "energy_and_forces_batch")
    for module in (fused, plain):
        torch.jit.script(module)
        with np.testing.assert_raises(ValueError):
            module.forward_batch((numbers, torch.zeros(3, 22, 3)))
        with np.testing.assert_raises(ValueError):
            module.forward_batch((numbers, torch.zeros(3, 23, 3)), torch.eye(3))
        with np.testing.assert_raises(ValueError):
            module.forward_batch((numbers, torch.zeros(0, 23, 3)))
    # the plan of a batch: rows grouped by species, conformer after conformer inside a species; places is its inverse
    nets = fused.neural_networks[0]
    holder = fused.aev_computer.batch_holder(3)
    assert fused.aev_computer.batch_holder(3) is holder
    kept, rows, sizes, places, offsets = nets._batch_plan(holder, 3, torch.device("cpu"))
    assert kept is holder and sizes == [3 * n for n in nets.group_sizes] and offsets.tolist() == [0, 23, 46, 69]
    assert rows.dtype == places.dtype == offsets.dtype == torch.int32
    assert sorted(rows.tolist()) == list(range(69)) and places[rows.long()].tolist() == list(range(69))
    order = nets.atom_order.tolist()
    first = 0
    for n in nets.group_sizes:
        want = [b * 23 + a for b in range(3) for a in order[first:first + n]]
        assert rows[3 * first:3 * (first + n)].tolist() == want
        first += n
