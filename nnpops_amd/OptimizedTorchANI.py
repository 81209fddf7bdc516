"""OptimizedTorchANI -- an ANI model with all four stages replaced
(reference src/pytorch/OptimizedTorchANI.py:33-54)."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from .BatchedNN import TorchANIBatchedNN, _FusedSpeciesNN
from .EnergyShifter import SpeciesEnergies, TorchANIEnergyShifter
from .SpeciesConverter import TorchANISpeciesConverter
from .SymmetryFunctions import TorchANISymmetryFunctions


class OptimizedTorchANI(torch.nn.Module):
    """The reference's four-module composition.  ``nn_layout`` (additive) picks the layout of the networks
    (:class:`TorchANIBatchedNN`); with the default ``'fused'`` and networks the fused kernels take, the instance becomes a
    :class:`FusedOptimizedTorchANI`: same modules, same state dict, same results, but AEV and networks run as ONE autograd
    node (``fused_step=False`` keeps the plain composition).

    ``trainable=True`` (extension): the networks' arrays are parameters (``TorchANIBatchedNN(..., trainable=True)``) and, with the
    fused layout, the instance becomes a :class:`TrainableOptimizedTorchANI`.

    ``force_trainable=True`` (extension; stands alone): the parameters of ``trainable=True`` behind nodes whose backward pass is recorded
    under ``create_graph=True`` (``TorchANIBatchedNN(..., force_trainable=True)``); with the fused layout the instance becomes a
    :class:`ForceTrainableOptimizedTorchANI`.

    A loss on FORCES trains ``force_trainable=True`` on the fused layout (``forward``, ``forward_batch``, ``members_energies(_batch)``,
    ``energies_qbcs(_batch)``) and ``nn_layout='grouped', trainable=True`` (this composition; ``forward`` and ``forward_batch``)::

        E = model((Z, x)).energies                                      # x.requires_grad_()
        F = -torch.autograd.grad(E.sum(), x, create_graph=True)[0]
        loss = (E - E0) ** 2 + ((F - F0) ** 2).sum()
        loss.backward(inputs=list(model.neural_networks.parameters()))   # or torch.autograd.grad(loss, parameters)

    Under ``create_graph=True`` the AEV op records its backward; the derivative of that node in the AEV cotangent is the AEV's tangent
    ``J.v`` (``Holder.tangent``), which autograd carries through the networks.  Refused with a message, never dropped: the gradient of
    a force in the POSITIONS (``loss.backward()`` without ``inputs=``, Hessians -- second derivatives of the AEV are not implemented),
    third derivatives, a forward pass on the same module between the forward and the derivatives that belong to it, and
    ``create_graph=True`` with a cell that requires a gradient.  The fused layout with ``trainable=True`` trains on energies only
    (there ``create_graph=True`` is refused); ``force_trainable=True`` is the fused layout for a loss with forces in it.

    Periodic batches (extension): every ``*_batch`` method takes ``cell`` [B, 3, 3] with ``pbc`` all True -- B periodic frames, each in
    its own box (see ``forward_batch``) -- on every layout, ``trainable`` and ``force_trainable`` included.

    Out of scope: scripting a trainable module, second derivatives in positions or box, weight-weight second derivatives, frames of
    thousands of atoms in a periodic batch (its neighbour search is the all-pairs scan inside each frame)."""

    def __init__(self, model, atomicNumbers: Tensor, nn_layout: str = 'fused', fused_step: bool = True, live_columns: bool = True,
                 trainable: bool = False, force_trainable: bool = False) -> None:
        super().__init__()
        self.species_converter = TorchANISpeciesConverter(model.species_converter, atomicNumbers)
        self.aev_computer = TorchANISymmetryFunctions(model.species_converter, model.aev_computer, atomicNumbers)
        self.neural_networks = TorchANIBatchedNN(model.species_converter, model.neural_networks, atomicNumbers, layout=nn_layout, trainable=trainable,
                                                 force_trainable=force_trainable)
        self.energy_shifter = TorchANIEnergyShifter(model.species_converter, model.energy_shifter, atomicNumbers)
        nets = self.neural_networks[0]
        if fused_step and isinstance(nets, _FusedSpeciesNN) and nets.fused_ok:
            nets.holder = self.aev_computer.holder        # the networks' fused_energy() drives the AEV kernels itself
            if live_columns:                               # ... and multiplies only the AEV blocks this molecule's species can fill
                nets.set_live_blocks(self.aev_computer.live_column_blocks())
            self.__class__ = (ForceTrainableOptimizedTorchANI if force_trainable else TrainableOptimizedTorchANI if trainable
                              else FusedOptimizedTorchANI)

    def forward(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        species_coordinates = self.species_converter(species_coordinates)
        species_aevs = self.aev_computer(species_coordinates, cell, pbc)
        species_energies = self.neural_networks(species_aevs)
        return self.energy_shifter(species_energies)

    @torch.jit.unused
    def _batch_arguments(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor], pbc: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
        """The argument errors of the batched methods; -> (species [B, N] of the module's molecule, coordinates [B, N, 3]).  A batch is
        non-periodic, or periodic with ``cell`` [B, 3, 3] -- one box per frame -- and ``pbc`` all True."""
        coordinates = species_coordinates[1]
        batch = self.aev_computer.check_batch_arguments(coordinates, cell, pbc)
        if batch < 1:
            raise ValueError('"positions" has to hold at least one conformer')
        return self.species_converter.species.expand(batch, -1), coordinates

    @torch.jit.unused
    def forward_batch(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                      pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        """Extension (the reference scores one molecule per call): B conformers of THE molecule this module was built for.
        (species[B, N], coordinates[B, N, 3]) -> SpeciesEnergies(species, energies[B]), one float64 energy per conformer, shifted by the
        molecule's self energy as ``forward`` returns it, differentiable with respect to the coordinates.  Here: the composition of
        ``aev_computer.forward_batch``, the networks and the shifter.

        Periodic batches: ``cell`` [B, 3, 3] with ``pbc`` all True scores B periodic frames, each in its own box (a minibatch of an
        NPT trajectory); a cell that requires a gradient gets ``cell.grad`` [B, 3, 3], from which each frame's stress follows as in
        ``forward``.  Every batched method takes the same two arguments."""
        species, coordinates = self._batch_arguments(species_coordinates, cell, pbc)
        species_aevs = self.aev_computer.forward_batch((species, coordinates), cell, pbc)
        species_energies = self.neural_networks(species_aevs)
        return self.energy_shifter(species_energies)

    @torch.jit.unused
    def members_energies(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                         pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        """Extension (TorchANI's ``members_energies``; the reference keeps only the mean): the energy of every ensemble member,
        SpeciesEnergies(species, energies [models, 1]), float64, each member shifted by the molecule's self energy as ``forward``
        shifts the mean -- differentiable with respect to the coordinates.  Arguments and checks of ``forward``."""
        species_coordinates = self.species_converter(species_coordinates)
        species_aevs = self.aev_computer(species_coordinates, cell, pbc)
        members = self.neural_networks.members_energies(species_aevs).energies
        return SpeciesEnergies(species_aevs[0], members + self.energy_shifter.self_energies)

    @torch.jit.unused
    def members_energies_batch(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                               pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        """``members_energies`` for B conformers of the module's molecule (arguments and checks of ``forward_batch``):
        SpeciesEnergies(species, energies [models, B])."""
        species, coordinates = self._batch_arguments(species_coordinates, cell, pbc)
        species_aevs = self.aev_computer.forward_batch((species, coordinates), cell, pbc)
        members = self.neural_networks.members_energies(species_aevs).energies
        return SpeciesEnergies(species, members + self.energy_shifter.self_energies)

    @staticmethod
    def _qbcs(species: Tensor, members: Tensor, unbiased: bool) -> Tuple[Tensor, Tensor, Tensor]:
        """members [models, molecules] float64 -> (species, mean over the models, std over the models / sqrt(atoms)): TorchANI's
        ``energies_qbcs``, both differentiable through the member energies"""
        members = members.double()
        qbcs = members.std(0, unbiased=unbiased) / (float(species.shape[1]) ** 0.5)
        return species, members.mean(0), qbcs

    @torch.jit.unused
    def energies_qbcs(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None, pbc: Optional[Tensor] = None,
                      unbiased: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
        """Extension (TorchANI's ``energies_qbcs``): (species, energies [1], qbcs [1]) -- the mean over the ensemble members and their
        query-by-committee factor ``std(members, unbiased) / sqrt(atoms)``, both from ``members_energies`` in float64 and
        differentiable through it (uncertainty-biased dynamics takes d qbcs / d coordinates from ONE backward)."""
        out = self.members_energies(species_coordinates, cell, pbc)
        return self._qbcs(out.species, out.energies, unbiased)

    @torch.jit.unused
    def energies_qbcs_batch(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None, pbc: Optional[Tensor] = None,
                            unbiased: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
        """``energies_qbcs`` for B conformers: (species [B, N], energies [B], qbcs [B])."""
        out = self.members_energies_batch(species_coordinates, cell, pbc)
        return self._qbcs(out.species, out.energies, unbiased)


class FusedOptimizedTorchANI(OptimizedTorchANI):
    """OptimizedTorchANI whose forward is ``torch.ops.NNPOpsANISymmetryFunctions.energy``: neighbour search + AEV + the four
    layers of every atomic network (+, when the positions require a gradient, the networks' input gradient and the AEV
    backward) issued back to back from one C++ call -- 7 kernel launches (the capacity check rides in the first network launch), one autograd node whose backward is a single
    multiplication -- instead of the ~45 launches the composition records.  Not constructed directly: ``OptimizedTorchANI(...)``
    turns into it.  Second derivatives are refused (use ``fused_step=False``).

    A ``cell`` that requires a gradient gets one (extension): the step then also runs the box-gradient pass of the AEV backward and
    keeps dE/dcell [3, 3] next to dE/dpositions -- the formal derivative with the minimum-image shifts held fixed, all nine entries
    -- so ``energy.backward()`` fills ``cell.grad`` and a stress / NPT driver needs nothing else.  Without it the step launches
    exactly what it always did.  ``energy_and_forces`` returns no virial."""

    @torch.jit.export
    def set_check_interval(self, interval: int) -> None:
        """Extension (cf. TorchANISymmetryFunctions.set_check_interval): verify the neighbour-buffer capacities only on every
        ``interval``-th call (0: only on the first).  Sets it on the AEV module's holder and on the one the fused step drives
        (the same object until the module has been through torch.jit.save / load, two copies after)."""
        self.aev_computer.set_check_interval(interval)
        self.neural_networks.set_check_interval(interval)

    @torch.jit.export
    def energy_and_forces(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                          pbc: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """Extension: (energies [1], forces [1, N, 3] = -dE/dpositions) from ONE call, outside autograd -- for MD drivers that take
        the forces as a model output instead of differentiating the energy (no autograd node, no ``.sum()`` / ``backward()``
        around the step: the same kernels as ``forward`` + ``backward``, three small launches and the autograd engine's host time
        fewer).  Same arguments, checks and energies as ``forward``."""
        converted = self.species_converter(species_coordinates)
        species, positions = converted.species, converted.coordinates
        self.aev_computer.check_arguments(species, cell, pbc)
        shift = self.energy_shifter.self_energies
        if shift.dtype == torch.float64 and shift.numel() == 1 and shift.device == positions.device:
            return self.neural_networks.fused_energy_forces(positions, cell, shift)
        energy, forces = self.neural_networks.fused_energy_forces(positions, cell)
        return energy + self.energy_shifter.self_energies, forces

    def forward(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        converted = self.species_converter(species_coordinates)
        species, positions = converted.species, converted.coordinates
        self.aev_computer.check_arguments(species, cell, pbc)
        # (positions go in as [1, N, 3] and the self-energy shift of EnergyShifter.py:52 is added by the kernel that takes the
        #  ensemble mean: no select / add / type-promotion kernels around the node, forward or backward)
        shift = self.energy_shifter.self_energies
        if shift.dtype == torch.float64 and shift.numel() == 1 and shift.device == positions.device:
            return SpeciesEnergies(species, self.neural_networks.fused_energy(positions, cell, shift))
        return self.energy_shifter((species, self.neural_networks.fused_energy(positions, cell)))

    @torch.jit.unused
    def forward_batch(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                      pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        """``OptimizedTorchANI.forward_batch`` as ONE autograd node (``torch.ops.NNPOpsANISymmetryFunctions.energy_batch``): the AEV
        kernels and the networks run once over all B x N atoms behind the batched holder of ``aev_computer`` -- the launches of a
        single-molecule step, not B times as many --, a mean per conformer, and a backward that scales every conformer's kept forces
        by its own upstream gradient.  An energy is the same bits wherever its conformer stands in whatever batch.  Second
        derivatives are refused, as in ``forward``."""
        species, coordinates = self._batch_arguments(species_coordinates, cell, pbc)
        holder = self.aev_computer.batch_holder(int(coordinates.shape[0]), cell is not None)
        shift = self.energy_shifter.self_energies
        if shift.dtype == torch.float64 and shift.numel() == 1 and shift.device == coordinates.device:
            return SpeciesEnergies(species, self.neural_networks.fused_energy_batch(holder, coordinates, shift, cell))
        return self.energy_shifter((species, self.neural_networks.fused_energy_batch(holder, coordinates, None, cell)))

    @torch.jit.unused
    def _shift_for(self, positions: Tensor) -> Optional[Tensor]:
        shift = self.energy_shifter.self_energies
        return shift if shift.dtype == torch.float64 and shift.numel() == 1 and shift.device == positions.device else None

    @torch.jit.unused
    def members_energies(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                         pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        """``OptimizedTorchANI.members_energies`` as TWO autograd nodes: the AEV op with its deferred backward and
        ``torch.ops.NNPOpsBatchedNN.FusedMLPMembers``, whose backward is one weighted launch of the networks' input gradient -- any
        function of the member energies costs one such launch and one AEV backward.  Second derivatives are refused."""
        converted = self.species_converter(species_coordinates)
        species, positions = converted.species, converted.coordinates
        self.aev_computer.check_arguments(species, cell, pbc)
        aev = torch.ops.NNPOpsANISymmetryFunctions.aev(self.aev_computer.holder, positions[0], cell)
        shift = self._shift_for(positions)
        members = self.neural_networks[0].fused_members(aev, shift).t()
        return SpeciesEnergies(species, members if shift is not None else members + self.energy_shifter.self_energies)

    @torch.jit.unused
    def members_energies_batch(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                               pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        """``OptimizedTorchANI.members_energies_batch`` on the same two nodes, over all B x N atoms behind the batched holder of
        ``aev_computer``: a conformer's member energies and its gradient are the same bits wherever it stands in whatever batch."""
        species, coordinates = self._batch_arguments(species_coordinates, cell, pbc)
        batch, atoms = int(coordinates.shape[0]), int(coordinates.shape[1])
        nets = self.neural_networks[0]
        holder, rows, sizes, places, offsets = nets._batch_plan(self.aev_computer.batch_holder(batch, cell is not None), batch, coordinates.device)
        aev = torch.ops.NNPOpsANISymmetryFunctions.aev(holder, coordinates.reshape(batch * atoms, 3), cell)
        shift = self._shift_for(coordinates)
        members = nets.fused_members(aev, shift, (rows, sizes, places, offsets)).t()
        return SpeciesEnergies(species, members if shift is not None else members + self.energy_shifter.self_energies)

    @torch.jit.unused
    def energy_and_forces_batch(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                                pbc: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """Extension: (energies [B], forces [B, N, 3] = -dE_b/dcoordinates) of B conformers from ONE call, outside autograd -- the
        counterpart of ``energy_and_forces``; the energies of ``forward_batch`` and the negated gradients, bit for bit."""
        _, coordinates = self._batch_arguments(species_coordinates, cell, pbc)
        holder = self.aev_computer.batch_holder(int(coordinates.shape[0]), cell is not None)
        shift = self.energy_shifter.self_energies
        if shift.dtype == torch.float64 and shift.numel() == 1 and shift.device == coordinates.device:
            return self.neural_networks.fused_energy_forces_batch(holder, coordinates, shift, cell)
        energies, forces = self.neural_networks.fused_energy_forces_batch(holder, coordinates, None, cell)
        return energies + self.energy_shifter.self_energies, forces


class TrainableOptimizedTorchANI(FusedOptimizedTorchANI):
    """``OptimizedTorchANI(..., trainable=True)`` on the fused layout.  ``forward``, ``forward_batch``, ``members_energies``,
    ``members_energies_batch``, ``energies_qbcs`` and ``energies_qbcs_batch`` run as TWO autograd nodes -- the AEV op and
    ``torch.ops.NNPOpsBatchedNN.FusedMLPMembersTrainable`` (``FusedMLPMeanTrainable`` for the mean) -- and are differentiable in the
    coordinates and in the networks' parameters (``neural_networks.parameters()``): one backward pass costs the networks' input
    gradient, one call of their weight gradient and the AEV backward, whatever function of the energies was differentiated.
    Energies and coordinate gradients are the bits of the default module at equal weights.  ``energy_and_forces`` /
    ``energy_and_forces_batch`` stay outside autograd and use the current weights.  Out of scope: scripting, second derivatives (a
    loss on forces trains ``nn_layout='grouped'``, see :class:`OptimizedTorchANI`; here ``create_graph=True`` is refused)."""

    def forward(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        converted = self.species_converter(species_coordinates)
        species, positions = converted.species, converted.coordinates
        self.aev_computer.check_arguments(species, cell, pbc)
        aev = torch.ops.NNPOpsANISymmetryFunctions.aev(self.aev_computer.holder, positions[0], cell)
        shift = self._shift_for(positions)
        energy = self.neural_networks[0].fused_mean(aev, shift)
        return SpeciesEnergies(species, energy) if shift is not None else self.energy_shifter((species, energy))

    @torch.jit.unused
    def forward_batch(self, species_coordinates: Tuple[Tensor, Tensor], cell: Optional[Tensor] = None,
                      pbc: Optional[Tensor] = None) -> SpeciesEnergies:
        species, coordinates = self._batch_arguments(species_coordinates, cell, pbc)
        batch, atoms = int(coordinates.shape[0]), int(coordinates.shape[1])
        nets = self.neural_networks[0]
        holder, rows, sizes, places, offsets = nets._batch_plan(self.aev_computer.batch_holder(batch, cell is not None), batch, coordinates.device)
        aev = torch.ops.NNPOpsANISymmetryFunctions.aev(holder, coordinates.reshape(batch * atoms, 3), cell)
        shift = self._shift_for(coordinates)
        energies = nets.fused_mean(aev, shift, (rows, sizes, places, offsets))
        return SpeciesEnergies(species, energies) if shift is not None else self.energy_shifter((species, energies))


class ForceTrainableOptimizedTorchANI(TrainableOptimizedTorchANI):
    """``OptimizedTorchANI(..., force_trainable=True)`` on the fused layout: :class:`TrainableOptimizedTorchANI` -- the same methods, two
    autograd nodes each, the same bits without ``create_graph`` -- on ``torch.ops.NNPOpsBatchedNN.FusedMLPMembersForceTrainable`` /
    ``FusedMLPMeanForceTrainable``.  Under ``create_graph=True`` both nodes record their backward pass: the force comes with a graph,
    and the parameter gradient of a loss with forces in it costs, next to the energy's own backward pass, the AEV tangent ``J.v`` and
    ONE call of ``nnpops_mlp_weight_grad_tangent``.  A force evaluation alone launches no weight gradient.  Take the gradient with
    ``loss.backward(inputs=parameters)`` or ``torch.autograd.grad(loss, parameters)``; refused with a message: the gradient of a force in
    the positions (``loss.backward()`` without ``inputs=``, Hessians), second derivatives in the parameters alone, third derivatives, a
    forward pass between a forward pass and its derivatives, and a cell that requires a gradient.  Out of scope: scripting."""
