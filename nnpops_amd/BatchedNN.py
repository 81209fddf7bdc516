"""TorchANIBatchedNN -- the atomic networks of an ANI ensemble evaluated as batched linear layers
(reference src/pytorch/BatchedNN.py:37-122): per-atom, per-model weight matrices zero-padded to a
common shape, four BatchedLinear calls with CELU(0.1) in between, and one fused sum / mean.

Buffer names (``layer{0,2,4,6}_{weights,biases}``) and the ModuleList-of-one structure are kept so
that state dicts and TorchScript files stay interchangeable.
"""
import math
from typing import List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor, nn
from torch.nn import functional as F

from . import torch_binding

torch_binding.load()


class SpeciesEnergies(NamedTuple):
    species: Tensor
    energies: Tensor


def _members(ensemble) -> List:
    """An Ensemble is a ModuleList of ANIModels; a single ANIModel stands for an ensemble of one."""
    return list(ensemble) if isinstance(ensemble, nn.ModuleList) else [ensemble]


def _networks_of(model) -> List[nn.Module]:
    """ANIModel is an ordered dict species-symbol -> Sequential; accept dicts and plain sequences too."""
    return list(model.values()) if hasattr(model, 'values') else list(model)


class _BatchedNN(nn.Module):
    """The reference's layout, kept bit-for-bit: one zero-padded weight matrix PER ATOM per model
    (``layer{k}_weights [1, atoms, models, out, in]``, reference BatchedNN.py:55-83) driven through the
    ``BatchedLinear`` op.  State dicts / TorchScript archives of the reference load into it unchanged.  It is
    a pure weight-streaming workload (21.6 GB of replicated weights for 2 000 atoms x 8 models): use it for
    interchange, and :class:`_SpeciesGroupedNN` (the default of ``TorchANIBatchedNN``) for speed."""

    def __init__(self, converter, ensemble, atomicNumbers: Tensor):
        super().__init__()
        species_list = converter((atomicNumbers, torch.empty(0))).species[0].tolist()
        models = [_networks_of(m) for m in _members(ensemble)]
        for ilayer in (0, 2, 4, 6):
            layers = [[model[s][ilayer] for s in species_list] for model in models]
            weights, biases = self.batchLinearLayers(layers)
            self.register_buffer(f'layer{ilayer}_weights', weights)
            self.register_buffer(f'layer{ilayer}_biases', biases)

    @staticmethod
    def batchLinearLayers(layers: List[List[nn.Linear]]) -> Tuple[Tensor, Tensor]:
        num_models, num_atoms = len(layers), len(layers[0])
        flat = [layer for sub in layers for layer in sub]
        max_out = max(layer.out_features for layer in flat)
        max_in = max(layer.in_features for layer in flat)
        weights = torch.zeros((1, num_atoms, num_models, max_out, max_in), dtype=torch.float32)
        biases = torch.zeros((1, num_atoms, num_models, max_out, 1), dtype=torch.float32)
        for imodel, sub in enumerate(layers):
            for iatom, layer in enumerate(sub):
                n_out, n_in = layer.weight.shape
                weights[0, iatom, imodel, :n_out, :n_in] = layer.weight.detach()
                biases[0, iatom, imodel, :n_out, 0] = layer.bias.detach()
        return weights, biases

    def _layers(self, aev: Tensor) -> Tensor:
        """the four BatchedLinear layers: aev [mols, atoms, features] -> v [mols, atoms, models, out, 1]"""
        linear = torch.ops.NNPOpsBatchedNN.BatchedLinear
        # [mols, atoms, features] -> [mols, atoms, 1, features, 1]
        v = aev.unsqueeze(-2).unsqueeze(-1)
        v = F.celu(linear(v, self.layer0_weights, self.layer0_biases), alpha=0.1)
        v = F.celu(linear(v, self.layer2_weights, self.layer2_biases), alpha=0.1)
        v = F.celu(linear(v, self.layer4_weights, self.layer4_biases), alpha=0.1)
        return linear(v, self.layer6_weights, self.layer6_biases)

    def forward(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        species, aev = species_aev
        v = self._layers(aev)
        # sum over atoms (and the padded dims) and mean over models in ONE reduction, as the reference does
        energies = torch.sum(v, (1, 2, 3, 4)) / v.shape[2]
        return SpeciesEnergies(species, energies)

    @torch.jit.unused
    def members_energies(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        """The same reduction without the sum over the models: energies [models, molecules] (TorchANI's ``members_energies``)."""
        species, aev = species_aev
        return SpeciesEnergies(species, torch.sum(self._layers(aev), (1, 3, 4)).t())


class _SpeciesGroupedNN(nn.Module):
    """Same function, MI355X layout: atoms are grouped by species once (the species of a Holder never change),
    so each layer is ONE batched GEMM per species, ``[models, out, in] x [in, atoms_of_species]`` -- the distinct
    weights (18.7 MB for ANI-2x x 8 models) instead of a per-atom replica of them (SURVEY.md s8(a) a15,
    s8(d) config 2).  The GEMMs go to the matrix cores through hipBLASLt/rocBLAS (plain library GEMMs).

    Buffers keep the reference's names, ``layer{k}_weights [kinds, models, out, in]`` and ``layer{k}_biases
    [kinds, models, out, 1]`` (zero-padded to the widest network of the layer, like the reference pads);
    ``load_state_dict`` also accepts the reference's per-atom tensors and compacts them."""

    group_sizes: List[int]

    def __init__(self, converter, ensemble, atomicNumbers: Tensor):
        super().__init__()
        species_list = converter((atomicNumbers, torch.empty(0))).species[0].tolist()
        kinds = sorted(set(species_list))
        kind_of_atom = torch.tensor([kinds.index(s) for s in species_list], dtype=torch.long)
        order = torch.sort(kind_of_atom, stable=True).indices
        self.register_buffer('atom_order', order)                          # atoms grouped by species, ascending inside
        self.register_buffer('first_atom_of_kind', torch.tensor([species_list.index(s) for s in kinds], dtype=torch.long))
        self.group_sizes = [int((kind_of_atom == k).sum()) for k in range(len(kinds))]
        self.num_atoms = len(species_list)
        models = [_networks_of(m) for m in _members(ensemble)]
        for ilayer in (0, 2, 4, 6):
            layers = [[model[s][ilayer] for s in kinds] for model in models]        # [model][kind]
            weights, biases = _BatchedNN.batchLinearLayers(layers)                   # [1, kinds, models, out, in]
            self.register_buffer(f'layer{ilayer}_weights', weights[0].contiguous())
            self.register_buffer(f'layer{ilayer}_biases', biases[0].contiguous())

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # a reference state dict holds [1, atoms, models, out, in]: keep one atom per species
        for ilayer in (0, 2, 4, 6):
            for what in ('weights', 'biases'):
                key = f'{prefix}layer{ilayer}_{what}'
                t = state_dict.get(key)
                if t is not None and t.dim() == 5 and t.shape[1] == self.num_atoms:
                    state_dict[key] = t[0].index_select(0, self.first_atom_of_kind.to(t.device)).contiguous()
        for extra in ('atom_order', 'first_atom_of_kind'):
            state_dict.setdefault(prefix + extra, getattr(self, extra))
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        return self._grouped_forward(species_aev)

    def _kind_outputs(self, kind: int, xs: Tensor) -> Tensor:
        """The four layers of one species: xs [features, cols] -> v [models, out, cols] (padded outputs are exactly zero)."""
        cols = xs.shape[1]
        # layer 0: every model reads the same AEVs -> ONE GEMM [models*out, features] x [features, cols]
        w0, b0 = self.layer0_weights[kind], self.layer0_biases[kind]
        v = torch.addmm(b0.reshape(-1, 1), w0.reshape(-1, w0.shape[2]), xs).reshape(w0.shape[0], w0.shape[1], cols)
        v = F.celu(v, alpha=0.1)                                         # [models, out, cols]
        v = F.celu(torch.baddbmm(self.layer2_biases[kind].expand(-1, -1, cols), self.layer2_weights[kind], v), alpha=0.1)
        v = F.celu(torch.baddbmm(self.layer4_biases[kind].expand(-1, -1, cols), self.layer4_weights[kind], v), alpha=0.1)
        return torch.baddbmm(self.layer6_biases[kind].expand(-1, -1, cols), self.layer6_weights[kind], v)

    @torch.jit.unused
    def members_energies(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        """Every model's energy, energies [models, molecules] (TorchANI's ``members_energies``): plain torch, twice differentiable."""
        species, aev = species_aev
        mols = aev.shape[0]
        x = aev.index_select(1, self.atom_order)
        num_models = self.layer0_weights.shape[1]
        energies = torch.zeros((num_models, mols), dtype=aev.dtype, device=aev.device)
        first = 0
        for kind, n in enumerate(self.group_sizes):                         # (the models are kept apart)
            v = self._kind_outputs(kind, x[:, first:first + n].reshape(mols * n, -1).t())
            first += n
            energies = energies + v.reshape(num_models, -1, mols, n).sum((1, 3))
        return SpeciesEnergies(species, energies)

    def _grouped_forward(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        species, aev = species_aev
        mols = aev.shape[0]
        x = aev.index_select(1, self.atom_order)                            # [mols, atoms, features], grouped
        num_models = self.layer0_weights.shape[1]
        energies = torch.zeros(mols, dtype=aev.dtype, device=aev.device)
        first = 0
        for kind, n in enumerate(self.group_sizes):
            v = self._kind_outputs(kind, x[:, first:first + n].reshape(mols * n, -1).t())     # xs [features, mols * n]
            first += n
            energies = energies + v.reshape(-1, mols, n).sum((0, 2))        # padded outputs are exactly zero
        return SpeciesEnergies(species, energies / num_models)


def _planes(w: Tensor) -> Tuple[Tensor, Tensor]:
    """fp32 [rows, cols] -> the two fp16 planes [rows, cols rounded up to 32] the split GEMM takes: w = hi + 2^-11 lo."""
    rows, cols = w.shape
    padded = torch.zeros((rows, (cols + 31) // 32 * 32), dtype=torch.float32, device=w.device)
    padded[:, :cols] = w
    hi = padded.half()
    lo = ((padded - hi.float()) * 2048.0).half()
    return hi, lo


def _pack_fragments(w: Tensor, permute: bool) -> Tensor:
    """fp32 [rows, cols] -> the fragment planes of csrc/mlp_fused.hip (what ``nnpops_mlp_pack`` writes; the GPU test compares
    the two): [row block][K step][plane][lane = r16 + 16 kg][8] fp16, ``w = hi + 2^-11 lo``; K order inside a step natural, or
    -- ``permute`` -- (4 kg + i | 16 + 4 kg + i - 4), the order in which a matrix-core accumulator hands over its rows."""
    rows, cols = w.shape
    nb, steps = (rows + 15) // 16, (cols + 31) // 32
    padded = torch.zeros((nb * 16, steps * 32), dtype=torch.float32, device=w.device)
    padded[:rows, :cols] = w
    kg = torch.arange(4, device=w.device).view(4, 1)
    i = torch.arange(8, device=w.device).view(1, 8)
    within = torch.where(i < 4, 4 * kg + i, 16 + 4 * kg + i - 4) if permute else 8 * kg + i          # [kg, i] -> k inside the step
    g = padded.view(nb, 16, steps, 32)[:, :, :, within.reshape(-1)]                                  # [rb, r16, s, (kg, i)]
    g = g.view(nb, 16, steps, 4, 8).permute(0, 2, 3, 1, 4)                                           # [rb, s, kg, r16, i]
    hi = g.half()
    lo = ((g - hi.float()) * 2048.0).half()
    return torch.stack([hi, lo], dim=2).reshape(-1)                                                  # [rb, s, plane, kg, r16, i]


def _up32(v: int) -> int:
    return (v + 31) // 32 * 32


def _takes_packed_path(aev: Tensor, planes: Tensor, order32: Tensor, fused_ok: bool, live_blocks: int = 0) -> bool:
    """Whether a module call goes to the kernels on its packed operands: one molecule on the device in float32, the planes and the
    atom order in the kernels' types (a ``.double()`` or ``.half()`` of the module has not touched them), the weights inside the
    activation bound.  ``live_blocks``: how many live column blocks stand in the way (members_energies: only the positions of
    OptimizedTorchANI vouch for them)."""
    return (aev.shape[0] == 1 and aev.is_cuda and aev.dtype == torch.float32 and planes.dtype == torch.float16
            and order32.dtype == torch.int32 and fused_ok and live_blocks == 0)


def _operand_bounds(weights: Tuple[Tensor, Tensor, Tensor, Tensor], biases: Tuple[Tensor, Tensor, Tensor]) -> Tuple[Tensor, Tensor]:
    """Crude bounds of what the kernels split into fp16, from the weights alone (AEV entries are sums of at most a few dozen terms
    <= 1): ``bound`` for the activations of the forward pass, ``back`` for the operands of the backward pass, which take the same
    planes: |d3| <= |w6|, |d2| <= |d3| ||W4||_1, |d1| <= |d2| ||W2||_1 (CELU' <= 1).  One-element tensors on the arrays' device."""
    w0, w2, w4, w6 = weights
    bound = torch.full((1,), 64.0, device=w0.device)
    for w, b in zip((w0, w2, w4), biases):
        bound = (w.abs().sum(-1).amax() * bound + b.abs().amax()).reshape(1)
    back = w6.abs().amax().reshape(1)
    for w in (w4, w2):
        back = (w.abs().sum(-2).amax() * back).reshape(1)
    return bound, back


def _activation_scale(worst: float) -> Tuple[int, bool]:
    """The kernels scale every activation by 2^-k before the fp16 split, k = ``act_scale_log2`` of the ops: the smallest k >= 4 whose
    bound 62 500 * 2^k (fp16's largest number, with margin) holds ``worst``; 4 for networks of ordinary size, up to 12 (bounds below
    2.56e8).  -> (k, whether it holds: beyond, the weights are left to the library-GEMM path)."""
    k = 4
    while k < 12 and worst >= 62500.0 * 2.0 ** k:
        k += 1
    return k, worst < 62500.0 * 2.0 ** k


def _cut(t: Tensor, rows: int, cols: int) -> Tensor:
    """[M, out, in] -> [M, rows, cols], zero padded / trimmed"""
    out = torch.zeros((t.shape[0], rows, cols), dtype=torch.float32, device=t.device)
    r, c = min(rows, t.shape[1]), min(cols, t.shape[2])
    out[:, :r, :c] = t[:, :r, :c]
    return out


def _kind_fragments(w0: Tensor, w2: Tensor, w4: Tensor, h1: int, h2: int, h3: int, columns: Optional[Tensor], with_w0tm: bool) -> List[Tensor]:
    """The planes of one kind at the packed widths h1, h2, h3, from its arrays [M, out, in], over all columns of the first layer
    or over ``columns`` of it: w0 (M members) | w2 (M) | w4 (M) | w4t (M) | w2t (M) | w0t [| w0tm (M)]."""
    M = w0.shape[0]
    if columns is not None:
        w0 = w0[:, :, columns]
    F = int(w0.shape[2])
    k0, k2, k4 = _cut(w0, h1, F), _cut(w2, h2, h1), _cut(w4, h3, h2)
    planes = [_pack_fragments(k0[m], False) for m in range(M)]
    planes += [_pack_fragments(k2[m], True) for m in range(M)]
    planes += [_pack_fragments(k4[m], True) for m in range(M)]
    planes += [_pack_fragments(k4[m].t(), True) for m in range(M)]
    planes += [_pack_fragments(k2[m].t(), True) for m in range(M)]
    planes.append(_pack_fragments(k0.reshape(M * h1, F).t(), True))
    if with_w0tm:
        planes += [_pack_fragments(k0[m].t(), True) for m in range(M)]
    return planes


class _FusedSpeciesNN(_SpeciesGroupedNN):
    """The species-grouped networks as TWO launches (``torch.ops.NNPOpsBatchedNN.FusedMLP``, csrc/mlp_fused.hip): a workgroup
    carries 64 atoms of one species and one ensemble member through all four layers -- and back through the small layers of
    the gradient -- with the activations in LDS / registers; a second launch forms dE/dAEV.  fp32 in and out, products as
    split-fp16 matrix instructions with fp32 accumulation.  Same buffers (and state dicts) as :class:`_SpeciesGroupedNN`; the
    packed operand planes are derived from them (non-persistent buffers, rebuilt when a state dict is loaded), each species at
    its OWN widths (the zero padding to the widest species that the reference's layout carries is stripped).  Frames with
    several molecules, CPU tensors, double precision and networks outside the kernels' shape (widths above 256, an input
    width that is not a multiple of 8, more than 8 species present) take the parent's path.

    Inside :class:`OptimizedTorchANI` the same kernels run behind ``torch.ops.NNPOpsANISymmetryFunctions.energy`` -- AEV and
    networks, forward and backward, as one autograd node (``fused_energy``)."""

    widths: List[int]
    live_blocks: List[int]
    act_scale_log2: int

    __jit_ignored_attributes__ = ["_batch_plans"]      # host-side state of the batched step

    def __init__(self, converter, ensemble, atomicNumbers: Tensor):
        super().__init__(converter, ensemble, atomicNumbers)
        self._batch_plans = {}
        self.num_models = int(self.layer0_weights.shape[1])
        self.widths = []
        self.live_blocks = []
        self.fused_ok = True
        self.act_scale_log2 = 4
        self.register_buffer('atom_order32', self.atom_order.to(torch.int32), persistent=False)
        for name in ('mlp_planes', 'mlp_floats', 'live_planes'):
            self.register_buffer(name, torch.empty(0), persistent=False)
        for name in ('x_blocks', 'dead_blocks'):
            self.register_buffer(name, torch.empty(0, dtype=torch.int32), persistent=False)
        self._refresh_planes()

    @torch.jit.unused
    def set_live_blocks(self, blocks: List[int]) -> None:
        """(inside OptimizedTorchANI) the 16-column blocks of the AEV that can be non-zero for this molecule
        (TorchANISymmetryFunctions.live_column_blocks): fused_energy() then runs the networks over those columns only --
        first layer packed over them, the others neither read nor multiplied, their gradient zero (nnpops_hip.h: x_groups)."""
        F = int(self.layer0_weights.shape[3])
        self.live_blocks = sorted(int(b) for b in blocks) if F % 16 == 0 and len(blocks) < F // 16 else []
        self._refresh_planes()

    @staticmethod
    def _true_width(w: Tensor, b: Tensor) -> int:
        """Rows of a (zero padded) layer that are not identically zero, rounded up to 32: w [models, out, in], b [models, out, 1]."""
        used = (w.abs().amax(dim=(0, 2)) > 0) | (b.abs().amax(dim=(0, 2)) > 0)
        last = int(torch.nonzero(used).max()) + 1 if bool(used.any()) else 1
        return _up32(last)

    @torch.jit.unused
    def _refresh_planes(self) -> None:
        w0, w2, w4, w6 = self.layer0_weights.float(), self.layer2_weights.float(), self.layer4_weights.float(), self.layer6_weights.float()
        b0, b2, b4, b6 = self.layer0_biases.float(), self.layer2_biases.float(), self.layer4_biases.float(), self.layer6_biases.float()
        kinds, M, F = w0.shape[0], w0.shape[1], w0.shape[3]
        planes, floats, widths = [], [], []
        for k in range(kinds):
            h1, h2, h3 = self._true_width(w0[k], b0[k]), self._true_width(w2[k], b2[k]), self._true_width(w4[k], b4[k])
            h1, h2, h3 = min(h1, _up32(w0.shape[2])), min(h2, _up32(w2.shape[2])), min(h3, _up32(w4.shape[2]))
            widths += [h1, h2, h3]
            planes += _kind_fragments(w0[k], w2[k], w4[k], h1, h2, h3, None, False)
            floats += [_cut(b0[k], h1, 1).reshape(-1), _cut(b2[k], h2, 1).reshape(-1), _cut(b4[k], h3, 1).reshape(-1),
                       _cut(w6[k][:, 0:1, :].transpose(1, 2), h3, 1).reshape(-1), b6[k].reshape(M, -1)[:, 0].reshape(-1)]
        self.mlp_planes = torch.cat(planes).contiguous()
        self.mlp_floats = torch.cat(floats).contiguous()
        self.widths = widths
        # the same networks over the live column blocks of the AEV only (set_live_blocks); at most 256 columns carry w0tm as well
        dev = w0.device
        if self.live_blocks:
            cols = torch.tensor([16 * g + c for g in self.live_blocks for c in range(16)], dtype=torch.long, device=dev)
            live = []
            for k in range(kinds):
                live += _kind_fragments(w0[k], w2[k], w4[k], widths[3 * k], widths[3 * k + 1], widths[3 * k + 2], cols, int(cols.numel()) <= 256)
            self.live_planes = torch.cat(live).contiguous()
            self.x_blocks = torch.tensor(self.live_blocks, dtype=torch.int32, device=dev)
            self.dead_blocks = torch.tensor([g for g in range(F // 16) if g not in set(self.live_blocks)], dtype=torch.int32, device=dev)
        else:
            self.live_planes = torch.empty(0, device=dev)
            self.x_blocks = torch.empty(0, dtype=torch.int32, device=dev)
            self.dead_blocks = torch.empty(0, dtype=torch.int32, device=dev)
        # the activation scale from the crude bounds of the weights; networks beyond every scale keep the library-GEMM path
        bound, back = _operand_bounds((w0, w2, w4, w6), (b0, b2, b4))
        worst = max(float(bound), float(back)) if bool(torch.isfinite(bound).all()) and bool(torch.isfinite(back).all()) else float("inf")
        self.act_scale_log2, holds = _activation_scale(worst)
        self.fused_ok = holds and F % 8 == 0 and F <= 1024 and max(widths) <= 256 and kinds <= 8 and int(w6.shape[2]) == 1
        self._reset_gradient_caches()

    @torch.jit.unused
    def _reset_gradient_caches(self) -> None:
        """new planes: the one-node step keeps dE/dAEV between the steps, cleared once for ONE list of live blocks
        (torch_binding.cpp, Holder::gradCache), and so does every batched holder"""
        holder = getattr(self, 'holder', None)
        if holder is not None:
            holder.reset_gradient_cache()
        for plan in self._batch_plans.values():
            plan[0].reset_gradient_cache()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._refresh_planes()

    def _require_fused(self, training: bool = False) -> None:
        """the steps that have no other path refuse weights beyond the activation bound (a state dict loaded since construction, an
        optimizer step: the weights no longer bound the fp16 operands)"""
        if self.fused_ok:
            return
        if training:
            raise RuntimeError("the weights exceed the activation bound of the fused network kernels (BatchedNN.py: fused_ok); "
                               "train with nn_layout='grouped'")
        raise RuntimeError("the loaded weights exceed the activation bound of the fused network kernels (BatchedNN.py: fused_ok); "
                           "build the model with OptimizedTorchANI(..., fused_step=False) or nn_layout='grouped'")

    def _operands(self, all_columns: bool = False) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
        """(planes, x_blocks, dead_blocks) of an op call: the networks packed over the live column blocks and the two block lists when
        there are live blocks (set_live_blocks), else -- or with ``all_columns`` -- the planes over all columns and no lists"""
        if self.x_blocks.numel() > 0 and not all_columns:
            return self.live_planes, self.x_blocks, self.dead_blocks
        return self.mlp_planes, None, None

    def forward(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        species, aev = species_aev
        if not _takes_packed_path(aev, self.mlp_planes, self.atom_order32, self.fused_ok):
            return self._grouped_forward(species_aev)
        total = torch.ops.NNPOpsBatchedNN.FusedMLP(aev[0].contiguous(), self.atom_order32, self.group_sizes, self.widths, self.num_models,
                                                   self.mlp_planes, self.mlp_floats, self.act_scale_log2)
        return SpeciesEnergies(species, total / self.num_models)

    @torch.jit.unused
    def fused_members(self, aev: Tensor, shift: Optional[Tensor] = None, batch: Optional[Tuple[Tensor, List[int], Tensor, Tensor]] = None) -> Tensor:
        """Every member's energy of the molecule(s) behind ``aev`` [atoms, features] (float32, on the device) as ONE autograd node
        (``torch.ops.NNPOpsBatchedNN.FusedMLPMembers``): -> [molecules, members], float32, or float64 and shifted with ``shift``.  Its
        backward is one launch of the networks' input gradient weighted by the upstream gradient of every (molecule, member); a
        zero there skips the member.  ``batch``: (rows, group sizes, places, offsets) of a conformer batch (``_batch_plan``).  Inside
        OptimizedTorchANI the networks run over the live column blocks, as in ``fused_energy``."""
        self._require_fused()
        rows, sizes, places, offsets = batch if batch is not None else (self.atom_order32, self.group_sizes, None, None)
        planes, x_blocks, dead_blocks = self._operands()
        return torch.ops.NNPOpsBatchedNN.FusedMLPMembers(aev, rows, sizes, self.widths, self.num_models, planes, self.mlp_floats,
                                                         x_blocks, dead_blocks, self.act_scale_log2, offsets, places, shift)

    @torch.jit.unused
    def members_energies(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        species, aev = species_aev
        if not _takes_packed_path(aev, self.mlp_planes, self.atom_order32, self.fused_ok, int(self.x_blocks.numel())):
            return _SpeciesGroupedNN.members_energies(self, species_aev)
        return SpeciesEnergies(species, self.fused_members(aev[0].contiguous()).t())

    def set_check_interval(self, interval: int) -> None:
        """(inside OptimizedTorchANI) how often the AEV holder behind fused_energy() verifies its neighbour capacities."""
        self.holder.set_check_interval(interval)

    def fused_energy(self, positions: Tensor, cell: Optional[Tensor], shift: Optional[Tensor] = None) -> Tensor:
        """AEV + networks of the whole frame as one autograd node (only inside OptimizedTorchANI, which hands over the AEV
        holder): positions [N, 3] or [1, N, 3] -> ensemble-mean energy [1]; with ``shift`` (the molecule's self energy, one
        float64 on the device) the energy comes back in float64, shifted as the reference's EnergyShifter does it."""
        self._require_fused()
        planes, x_blocks, dead_blocks = self._operands()
        return torch.ops.NNPOpsANISymmetryFunctions.energy(self.holder, positions, cell, self.atom_order32, self.group_sizes, self.widths,
                                                           self.num_models, planes, self.mlp_floats, shift, x_blocks, dead_blocks, self.act_scale_log2)

    def fused_energy_forces(self, positions: Tensor, cell: Optional[Tensor], shift: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """The same step outside autograd: (energy [1], forces = -dE/dpositions in the shape of ``positions``) from one call."""
        self._require_fused()
        planes, x_blocks, dead_blocks = self._operands()
        return torch.ops.NNPOpsANISymmetryFunctions.energy_forces(self.holder, positions, cell, self.atom_order32, self.group_sizes, self.widths,
                                                                  self.num_models, planes, self.mlp_floats, shift, x_blocks, dead_blocks,
                                                                  self.act_scale_log2)

    @torch.jit.unused
    def _batch_plan(self, holder, batch: int, device: torch.device):
        """What the batched step needs for ``batch`` conformers, made once per batch size (and device): the batched AEV holder (the
        one of TorchANISymmetryFunctions.batch_holder: no second holder for the same size), the rows of the batch * N atoms grouped by
        species -- conformer after conformer inside a species --, the group sizes, the place of every row in that order and the
        molecule offsets.  The packed planes, live blocks and activation scale are the ones of the single-molecule step."""
        key = (batch, str(device), id(holder))      # (the periodic and the non-periodic holder of one batch size each keep their plan)
        plan = self._batch_plans.get(key)
        if plan is None or plan[0] is not holder:
            n = self.num_atoms
            order = self.atom_order.to(device=device, dtype=torch.int64)
            base = torch.arange(batch, dtype=torch.int64, device=device).unsqueeze(1) * n
            parts, first = [], 0
            for size in self.group_sizes:
                parts.append((base + order[first:first + size].unsqueeze(0)).reshape(-1))
                first += size
            rows = torch.cat(parts)
            places = torch.empty_like(rows)
            places[rows] = torch.arange(batch * n, dtype=torch.int64, device=device)
            offsets = torch.arange(batch + 1, dtype=torch.int32, device=device) * n
            plan = (holder, rows.to(torch.int32).contiguous(), [size * batch for size in self.group_sizes], places.to(torch.int32).contiguous(),
                    offsets.contiguous())
            self._batch_plans[key] = plan
        return plan

    @torch.jit.unused
    def _batch_call(self, op, holder, positions: Tensor, shift: Optional[Tensor], cell: Optional[Tensor] = None):
        self._require_fused()
        holder, rows, sizes, places, offsets = self._batch_plan(holder, int(positions.shape[0]), positions.device)
        planes, x_blocks, dead_blocks = self._operands()
        return op(holder, positions, cell, rows, sizes, self.widths, self.num_models, planes, self.mlp_floats, offsets, places, shift,
                  x_blocks, dead_blocks, self.act_scale_log2)

    @torch.jit.unused
    def fused_energy_batch(self, holder, positions: Tensor, shift: Optional[Tensor] = None, cell: Optional[Tensor] = None) -> Tensor:
        """fused_energy() for B conformers (only inside OptimizedTorchANI, which hands over the batched AEV holder): positions [B, N, 3]
        -> ensemble-mean energies [B] as one autograd node (``torch.ops.NNPOpsANISymmetryFunctions.energy_batch``); float64 and shifted
        with ``shift``.  ``cell`` [B, 3, 3]: a periodic batch, every frame in its own box (``holder`` is then the periodic batch holder);
        a cell that requires a gradient gets dE_b/dcell_b."""
        return self._batch_call(torch.ops.NNPOpsANISymmetryFunctions.energy_batch, holder, positions, shift, cell)

    @torch.jit.unused
    def fused_energy_forces_batch(self, holder, positions: Tensor, shift: Optional[Tensor] = None,
                                  cell: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """The same step outside autograd: (energies [B], forces [B, N, 3] = -dE_b/dpositions); no virial."""
        return self._batch_call(torch.ops.NNPOpsANISymmetryFunctions.energy_forces_batch, holder, positions, shift, cell)


PARAMETER_NAMES = tuple(f'layer{ilayer}_{what}' for ilayer in (0, 2, 4, 6) for what in ('weights', 'biases'))


def _buffers_to_parameters(module: nn.Module) -> None:
    """the eight ``layer{0,2,4,6}_{weights,biases}`` buffers of a species-grouped module become ``nn.Parameter``s of the same names (and
    the same places in its state dict)"""
    for name in PARAMETER_NAMES:
        value = module._buffers.pop(name)
        module.register_parameter(name, nn.Parameter(value.detach().clone()))


class _TrainableGroupedNN(_SpeciesGroupedNN):
    """:class:`_SpeciesGroupedNN` with its eight arrays as parameters: plain torch, differentiable in the AEV and in the parameters
    to any order.  ``TorchANIBatchedNN(..., layout='grouped', trainable=True)``; what the fused trainable layout is compared with.
    The zero padding to the widest species is structural: its gradient is exactly zero (a padded unit has no input weights, no bias
    and no output weights), so it stays zero under any optimizer that leaves a zero-gradient entry alone.  Not scriptable."""

    def __init__(self, converter, ensemble, atomicNumbers: Tensor):
        super().__init__(converter, ensemble, atomicNumbers)
        _buffers_to_parameters(self)


class _TrainableFusedNN(_FusedSpeciesNN):
    """:class:`_FusedSpeciesNN` with its eight arrays as parameters (``TorchANIBatchedNN(..., trainable=True)``).  One molecule on the
    device in float32 runs ``torch.ops.NNPOpsBatchedNN.FusedMLPMembersTrainable``: the forward pass of ``FusedMLPMembers`` on the
    packed planes, bit for bit, and a backward pass that returns the gradient of the AEV as before and, from one call of
    ``nnpops_mlp_weight_grad`` (csrc/mlp_weight_grad.h), the gradients of all eight arrays for whatever function of the member
    energies was differentiated.  CPU tensors, float64, several molecules and networks outside the kernels' shape take the parent's
    plain-torch path, which is differentiable in the parameters as it stands.

    The packed planes are derived from the parameters: they are rebuilt on the first forward pass after a parameter's version has
    changed (an optimizer step, an in-place edit) and after ``load_state_dict``; while the parameters stand, nothing is rebuilt
    (``plane_rebuilds`` counts).  With float32 parameters on a GPU the rebuild is ``torch.ops.NNPOpsBatchedNN.PackNetworks``
    (csrc/mlp_pack_networks.h: two launches, fresh tensors, the planes the host route writes bit for bit) and one small copy to the host
    that carries every decision (``device_packs`` counts those); the constructor, CPU parameters, other dtypes and a new list of live
    blocks pack on the host as the default module does.  The widths every species is packed at are fixed at construction from the
    source networks; a rebuild that finds others raises and leaves the module as it was.  First derivatives only (a loss on forces
    trains ``force_trainable=True``), not scriptable."""

    __jit_ignored_attributes__ = ["_batch_plans", "_plane_versions", "_fixed_widths", "plane_rebuilds", "device_packs", "_blocks_packed"]

    _fixed_widths = None           # (class defaults: _refresh_planes runs inside the parent's constructor)
    _plane_versions = None
    plane_rebuilds = 0
    device_packs = 0               # the rebuilds among them that packed on the device (torch.ops.NNPOpsBatchedNN.PackNetworks)
    _blocks_packed = None          # the live blocks x_blocks / dead_blocks were last built for (on the host)

    def __init__(self, converter, ensemble, atomicNumbers: Tensor):
        super().__init__(converter, ensemble, atomicNumbers)
        self._fixed_widths = list(self.widths)
        _buffers_to_parameters(self)
        self._plane_versions = self._versions()

    def _versions(self):
        return tuple((id(p), p._version, p.device) for p in (getattr(self, name) for name in PARAMETER_NAMES))

    @torch.jit.unused
    def _packed_widths(self) -> List[int]:
        """the widths _refresh_planes would pack every kind at, from the current values"""
        out = []
        for k in range(int(self.layer0_weights.shape[0])):
            for w, b in ((self.layer0_weights, self.layer0_biases), (self.layer2_weights, self.layer2_biases), (self.layer4_weights, self.layer4_biases)):
                out.append(min(self._true_width(w[k].float(), b[k].float()), _up32(int(w.shape[2]))))
        return out

    @torch.jit.unused
    def _packs_on_device(self) -> bool:
        """whether a rebuild can take ``torch.ops.NNPOpsBatchedNN.PackNetworks``: a constructed module whose eight parameters are float32
        on one GPU, in the shape of the fused kernels, with the live blocks its ``x_blocks`` already holds"""
        if self._fixed_widths is None or self._blocks_packed != self.live_blocks:
            return False
        parameters = [getattr(self, name) for name in PARAMETER_NAMES]
        w0, w6 = parameters[0], parameters[6]
        if any(not p.is_cuda or p.dtype != torch.float32 or p.device != w0.device or not p.is_contiguous() for p in parameters):
            return False
        if self.x_blocks.device != w0.device or self.x_blocks.dtype != torch.int32:
            return False
        return (int(w0.shape[3]) % 8 == 0 and int(w0.shape[3]) <= 1024 and max(self._fixed_widths) <= 256 and int(w0.shape[0]) <= 8
                and int(w0.shape[1]) <= 128 and int(w6.shape[2]) == 1)

    @torch.jit.unused
    def _refresh_planes_on_device(self) -> None:
        """``_FusedSpeciesNN._refresh_planes`` with the planes packed by one op (csrc/mlp_pack_networks.h) and every decision taken from
        its status block: one small copy to the host, nothing else waits for the device"""
        parameters = [getattr(self, name).detach() for name in PARAMETER_NAMES]
        planes, floats, live, status = torch.ops.NNPOpsBatchedNN.PackNetworks(parameters, self._fixed_widths, self.x_blocks if self.live_blocks else None)
        words = status.cpu()
        last, not_finite, scalars = words[:24].tolist(), int(words[24]), words[26:44].view(torch.float64).tolist()
        shapes = [int(parameters[i].shape[2]) for i in (0, 2, 4)]
        kinds = int(parameters[0].shape[0])
        widths = [min(_up32(max(last[3 * k + layer], 1)), _up32(shapes[layer])) for k in range(kinds) for layer in range(3)]
        self._require_fixed_widths(widths)                 # (BEFORE anything is replaced, as on the host)
        rows, columns, biases, last_weight = scalars[0:3], scalars[3:5], scalars[5:8], scalars[8]
        bound = 64.0                                       # (the bounds of _operand_bounds, from the block's nine scalars)
        for row, bias in zip(rows, biases):
            bound = row * bound + bias
        back = last_weight * columns[0] * columns[1]
        worst = max(bound, back) if not not_finite and math.isfinite(bound) and math.isfinite(back) else float("inf")
        self.mlp_planes, self.mlp_floats, self.live_planes = planes, floats, live
        self.act_scale_log2, self.fused_ok = _activation_scale(worst)     # (the shape was checked before this route was taken)
        self._reset_gradient_caches()
        self.device_packs += 1

    @torch.jit.unused
    def _require_fixed_widths(self, widths: List[int]) -> None:
        """a rebuild that would pack other widths than the constructor did is refused, and leaves the module as it was"""
        if widths != self._fixed_widths:
            raise RuntimeError(f"the networks' widths changed from {self._fixed_widths} to {widths}: the structure of a trainable "
                               "module is fixed at construction (the zero padding must stay zero)")

    @torch.jit.unused
    def _refresh_planes(self) -> None:
        with torch.no_grad():
            if self._packs_on_device():
                self._refresh_planes_on_device()
            else:
                if self._fixed_widths is not None:         # (checked BEFORE anything is replaced; none yet inside the base class's constructor)
                    self._require_fixed_widths(self._packed_widths())
                super()._refresh_planes()
                self._blocks_packed = list(self.live_blocks)
        self.plane_rebuilds += 1
        self._plane_versions = self._versions()

    @torch.jit.unused
    def _current_planes(self) -> None:
        if self._plane_versions != self._versions():
            self._refresh_planes()

    def forward(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        species, aev = species_aev
        self._current_planes()
        if not _takes_packed_path(aev, self.mlp_planes, self.atom_order32, self.fused_ok):
            return self._grouped_forward(species_aev)
        # (the default module's arithmetic, over all columns as there: the sum over atoms and members from the kernel, divided here)
        return SpeciesEnergies(species, self._trainable_op(aev[0].contiguous(), None, None, True, True, True) / self.num_models)

    @torch.jit.unused
    def fused_members(self, aev: Tensor, shift: Optional[Tensor] = None, batch: Optional[Tuple[Tensor, List[int], Tensor, Tensor]] = None) -> Tensor:
        """``_FusedSpeciesNN.fused_members`` as a node that is differentiable in the parameters as well"""
        self._current_planes()
        return self._trainable_op(aev, shift, batch, False)

    @torch.jit.unused
    def fused_mean(self, aev: Tensor, shift: Optional[Tensor] = None, batch: Optional[Tuple[Tensor, List[int], Tensor, Tensor]] = None) -> Tensor:
        """The ensemble mean of the molecule(s) behind ``aev`` -> [molecules] (``torch.ops.NNPOpsBatchedNN.FusedMLPMeanTrainable``): the
        energy of ``fused_energy`` / ``fused_energy_batch``, bit for bit, as a node that is differentiable in the AEV and the parameters"""
        self._current_planes()
        return self._trainable_op(aev, shift, batch, True)

    @torch.jit.unused
    def _trainable_op(self, aev: Tensor, shift: Optional[Tensor], batch: Optional[Tuple[Tensor, List[int], Tensor, Tensor]], mean: bool,
                      total: bool = False, all_columns: bool = False) -> Tensor:
        self._require_fused(training=True)
        rows, sizes, places, offsets = batch if batch is not None else (self.atom_order32, self.group_sizes, None, None)
        planes, x_blocks, dead_blocks = self._operands(all_columns)
        args = (aev, rows, sizes, self.widths, self.num_models, planes, self.mlp_floats, x_blocks, dead_blocks, self.act_scale_log2, offsets, places,
                shift, [getattr(self, name) for name in PARAMETER_NAMES])
        if mean:
            return torch.ops.NNPOpsBatchedNN.FusedMLPMeanTrainable(*args, total)
        return torch.ops.NNPOpsBatchedNN.FusedMLPMembersTrainable(*args)

    @torch.jit.unused
    def members_energies(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        self._current_planes()
        species, aev = species_aev
        if not _takes_packed_path(aev, self.mlp_planes, self.atom_order32, self.fused_ok, int(self.x_blocks.numel())):
            return _SpeciesGroupedNN.members_energies(self, species_aev)
        return SpeciesEnergies(species, self._trainable_op(aev[0].contiguous(), None, None, False).t())

    # (the one-node steps take no parameter gradient: they run outside the parameters' autograd, on the current weights)
    def fused_energy(self, positions: Tensor, cell: Optional[Tensor], shift: Optional[Tensor] = None) -> Tensor:
        self._current_planes()
        return super().fused_energy(positions, cell, shift)

    def fused_energy_forces(self, positions: Tensor, cell: Optional[Tensor], shift: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        self._current_planes()
        return super().fused_energy_forces(positions, cell, shift)

    @torch.jit.unused
    def _batch_call(self, op, holder, positions: Tensor, shift: Optional[Tensor]):
        self._current_planes()
        return super()._batch_call(op, holder, positions, shift)


class _ForceTrainableFusedNN(_TrainableFusedNN):
    """:class:`_TrainableFusedNN` for a loss on forces (``TorchANIBatchedNN(..., force_trainable=True)``): the same parameters, names,
    state dicts, lazy plane rebuild and counters, behind ``torch.ops.NNPOpsBatchedNN.FusedMLPMembersForceTrainable`` /
    ``FusedMLPMeanForceTrainable``.  Forward passes and -- without ``create_graph`` -- backward passes are those of ``trainable=True``,
    bit for bit.  Under ``create_graph=True`` the backward pass is recorded: the gradient of the AEV comes with a graph whose own
    backward, given the AEV's tangent ``J.v``, is ONE call of ``nnpops_mlp_weight_grad_tangent`` (csrc/mlp_weight_grad_tangent.h) for the
    eight parameter gradients, and the gradient of the upstream tensor where a function of the member energies asks for it.  Refused
    with a message: the gradient of a force in the AEV (Hessians, ``loss.backward()`` without ``inputs=``), second derivatives in the
    parameters alone, third derivatives.  Not scriptable."""

    @torch.jit.unused
    def _trainable_op(self, aev: Tensor, shift: Optional[Tensor], batch: Optional[Tuple[Tensor, List[int], Tensor, Tensor]], mean: bool,
                      total: bool = False, all_columns: bool = False) -> Tensor:
        self._require_fused(training=True)
        rows, sizes, places, offsets = batch if batch is not None else (self.atom_order32, self.group_sizes, None, None)
        planes, x_blocks, dead_blocks = self._operands(all_columns)
        args = (aev, rows, sizes, self.widths, self.num_models, planes, self.mlp_floats, x_blocks, dead_blocks, self.act_scale_log2, offsets, places,
                shift, [getattr(self, name) for name in PARAMETER_NAMES])
        if mean:
            return torch.ops.NNPOpsBatchedNN.FusedMLPMeanForceTrainable(*args, total)
        return torch.ops.NNPOpsBatchedNN.FusedMLPMembersForceTrainable(*args)


class _SplitGemmSpeciesNN(_SpeciesGroupedNN):
    """(Round-1/2 default, kept as ``layout='gemm'`` for comparison and for widths the fused kernels do not take.)  The
    species-grouped networks on the library's own GEMM (``torch.ops.NNPOpsBatchedNN.GroupedMLP``, csrc/batched_nn.hip): fp32 in and out, products as split-fp16 matrix instructions with fp32 accumulation, bias + CELU
    fused into the epilogues and CELU' into the input-gradient pass -- six launches per species and step instead of
    GEMM + elementwise kernels for every layer.  Same buffers (and state dicts) as :class:`_SpeciesGroupedNN`; the packed
    operand planes are derived from them (non-persistent buffers, rebuilt when a state dict is loaded).  Frames with
    several molecules, CPU tensors and double precision take the parent's path."""

    def __init__(self, converter, ensemble, atomicNumbers: Tensor):
        super().__init__(converter, ensemble, atomicNumbers)
        self.num_models = int(self.layer0_weights.shape[1])
        self.h1 = int(self.layer0_weights.shape[2])
        self.h2 = int(self.layer2_weights.shape[2])
        self.h3 = int(self.layer4_weights.shape[2])
        self.last_b: List[float] = []
        self.fused_ok = True
        self.register_buffer('atom_order32', self.atom_order.to(torch.int32), persistent=False)
        for name in ('fwd_hi', 'fwd_lo', 'bwd_hi', 'bwd_lo', 'packed_biases', 'last_w'):
            self.register_buffer(name, torch.empty(0), persistent=False)
        self._refresh_planes()

    @torch.jit.unused
    def _refresh_planes(self) -> None:
        w0, w2, w4, w6 = self.layer0_weights, self.layer2_weights, self.layer4_weights, self.layer6_weights
        kinds, models = w0.shape[0], w0.shape[1]
        fwd_hi, fwd_lo, bwd_hi, bwd_lo, biases, last_w, last_b = [], [], [], [], [], [], []
        for k in range(kinds):
            fwd = [w0[k].reshape(-1, w0.shape[3]), w2[k].reshape(-1, w2.shape[3]), w4[k].reshape(-1, w4.shape[3])]
            bwd = [w0[k].reshape(-1, w0.shape[3]).t().contiguous(),
                   torch.cat([w2[k][m].t() for m in range(models)], 0).contiguous(),
                   torch.cat([w4[k][m].t() for m in range(models)], 0).contiguous()]
            for mats, his, los in ((fwd, fwd_hi, fwd_lo), (bwd, bwd_hi, bwd_lo)):
                for w in mats:
                    hi, lo = _planes(w.float())
                    his.append(hi.reshape(-1))
                    los.append(lo.reshape(-1))
            biases += [self.layer0_biases[k].reshape(-1), self.layer2_biases[k].reshape(-1), self.layer4_biases[k].reshape(-1)]
            last_w.append(w6[k][:, 0, :].reshape(-1))
            last_b.append(float(self.layer6_biases[k].sum()))
        self.fwd_hi, self.fwd_lo = torch.cat(fwd_hi), torch.cat(fwd_lo)
        self.bwd_hi, self.bwd_lo = torch.cat(bwd_hi), torch.cat(bwd_lo)
        # the split GEMM scales its A operand by 1/16 before the fp16 split: activations must stay below ~1e6, in the forward pass
        # and in the backward pass; networks that could exceed it keep the library-GEMM path.
        bound, back = _operand_bounds((w0, w2, w4, w6), (self.layer0_biases, self.layer2_biases, self.layer4_biases))
        self.fused_ok = (bool(torch.isfinite(bound).all()) and float(bound) < 1.0e6
                         and bool(torch.isfinite(back).all()) and float(back) < 1.0e6)
        self.packed_biases = torch.cat(biases).float().contiguous()
        self.last_w = torch.cat(last_w).float().contiguous()
        self.last_b = last_b

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._refresh_planes()

    def forward(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        species, aev = species_aev
        if not _takes_packed_path(aev, self.fwd_hi, self.atom_order32, self.fused_ok):
            return self._grouped_forward(species_aev)
        # (the op reads the atoms of a species through atom_order32 and writes their gradients back through it: no gather
        #  into species order, no scatter back)
        per_atom = torch.ops.NNPOpsBatchedNN.GroupedMLP(aev[0].contiguous(), self.atom_order32, self.group_sizes, self.num_models,
                                                        self.h1, self.h2, self.h3,
                                                        self.fwd_hi, self.fwd_lo, self.bwd_hi, self.bwd_lo,
                                                        self.packed_biases, self.last_w, self.last_b)
        return SpeciesEnergies(species, per_atom.sum().reshape(1) / self.num_models)


class TorchANIBatchedNN(nn.ModuleList):
    """``layout='fused'`` (default): species-grouped networks as two launches of the fused kernels (csrc/mlp_fused.hip);
    ``'gemm'``: one split-fp16 GEMM per layer and species with fused activations (csrc/batched_nn.hip); ``'grouped'``: the same
    grouping on torch's library GEMMs; ``'reference'``: the reference's per-atom replicated weights through ``BatchedLinear``
    (interchange with reference state dicts / archives).

    ``trainable=True`` (extension; ``'fused'`` and ``'grouped'`` only): the eight ``layer{0,2,4,6}_{weights,biases}`` arrays are
    ``nn.Parameter``s under the same names -- state dicts interchange with the default module in both directions, the reference's
    per-atom state dict still loads -- and every output is differentiable in them: ``'fused'`` through
    ``torch.ops.NNPOpsBatchedNN.FusedMLPMembersTrainable`` for one molecule on the device in float32 (first derivatives), plain torch
    otherwise and for ``'grouped'``.  Out of scope: scripting a trainable module, second derivatives through the fused op (training
    on forces: ``force_trainable``).

    ``force_trainable=True`` (extension; stands alone, ``'fused'`` and ``'grouped'`` only): the parameters of ``trainable=True`` -- same
    names, state dicts interchange -- behind ``torch.ops.NNPOpsBatchedNN.FusedMLPMembersForceTrainable``, whose backward pass is recorded
    under ``create_graph=True``, so that a loss on forces reaches the parameters (:class:`_ForceTrainableFusedNN`).  For ``'grouped'``,
    which is plain torch and differentiable to any order, it is a synonym of ``trainable=True``."""

    def __init__(self, converter, ensemble, atomicNumbers: Tensor, layout: str = 'fused', trainable: bool = False, force_trainable: bool = False):
        if layout not in ('fused', 'gemm', 'grouped', 'reference'):
            raise ValueError("layout must be 'fused', 'gemm', 'grouped' or 'reference'")
        if force_trainable and trainable:
            raise ValueError("force_trainable=True stands alone: it already has the parameters and the first derivatives of trainable=True")
        if trainable and layout not in ('fused', 'grouped'):
            raise ValueError(f"trainable=True needs layout='fused' or layout='grouped' (got {layout!r}: its packed operands have no weight gradient)")
        if force_trainable and layout not in ('fused', 'grouped'):
            raise ValueError(f"force_trainable=True needs layout='fused' or layout='grouped' (got {layout!r}: its packed operands have no weight gradient)")
        impl = {'fused': _FusedSpeciesNN, 'gemm': _SplitGemmSpeciesNN, 'grouped': _SpeciesGroupedNN, 'reference': _BatchedNN}[layout]
        if trainable:
            impl = {'fused': _TrainableFusedNN, 'grouped': _TrainableGroupedNN}[layout]
        if force_trainable:
            impl = {'fused': _ForceTrainableFusedNN, 'grouped': _TrainableGroupedNN}[layout]
        super().__init__([impl(converter, ensemble, atomicNumbers)])

    def forward(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        return self[0].forward(species_aev)

    @torch.jit.unused
    def members_energies(self, species_aev: Tuple[Tensor, Tensor]) -> SpeciesEnergies:
        """Extension (TorchANI's ``Ensemble.members_energies``): (species, aev [molecules, atoms, features]) ->
        SpeciesEnergies(species, energies [models, molecules]), every model's sum over the atoms, differentiable with respect to the
        AEV.  ``layout='fused'`` runs one molecule on the fused kernels as one autograd node (first derivatives); every other layout,
        CPU tensors, float64, several molecules and networks outside the kernels' shape take plain torch (twice differentiable)."""
        return self[0].members_energies(species_aev)

    def fused_energy(self, positions: Tensor, cell: Optional[Tensor], shift: Optional[Tensor] = None) -> Tensor:
        return self[0].fused_energy(positions, cell, shift)

    def fused_energy_forces(self, positions: Tensor, cell: Optional[Tensor], shift: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        return self[0].fused_energy_forces(positions, cell, shift)

    def set_check_interval(self, interval: int) -> None:
        self[0].set_check_interval(interval)

    @torch.jit.unused
    def fused_energy_batch(self, holder, positions: Tensor, shift: Optional[Tensor] = None, cell: Optional[Tensor] = None) -> Tensor:
        return self[0].fused_energy_batch(holder, positions, shift, cell)

    @torch.jit.unused
    def fused_energy_forces_batch(self, holder, positions: Tensor, shift: Optional[Tensor] = None,
                                  cell: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        return self[0].fused_energy_forces_batch(holder, positions, shift, cell)
