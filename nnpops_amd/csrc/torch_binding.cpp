// torch_binding.cpp -- the PyTorch operator surface of the reference, re-implemented on top of the
// C ABI (include/nnpops_hip.h).  Plain C++ (no kernels here): every entry point hands raw device
// pointers of contiguous tensors to libnnpops_hip.so on the current HIP stream.
//
// Registrations mirror the reference one-for-one so that TorchScript modules and user code written
// against NNPOps keep working:
//   torch.classes.NNPOpsANISymmetryFunctions.Holder / torch.ops.NNPOpsANISymmetryFunctions.operation
//                                                         (reference src/pytorch/SymmetryFunctions.cpp:265-284)
//   torch.classes.NNPOpsCFConvNeighbors.Holder            (reference src/pytorch/CFConvNeighbors.cpp:77-85)
//   torch.classes.NNPOpsCFConv.Holder / torch.ops.NNPOpsCFConv.operation / operation_periodic (additive: dL/dbox)
//   torch.ops.NNPOpsCFConv.operation_twice / operation_periodic_twice (additive: the same ops, twice differentiable)
//   torch.ops.NNPOpsCFConv.operation_weights / operation_periodic_weights (additive: the same ops with trainable weights)
//   torch.ops.NNPOpsCFConv.operation_weights_twice / operation_periodic_weights_twice (additive: trainable weights under a force loss)
//                                                         (reference src/pytorch/CFConv.cpp:276-291)
//   torch.ops.neighbors.getNeighborPairs                  (reference src/pytorch/neighbors/neighbors.cpp:4)
//   torch.ops.NNPOpsBatchedNN.BatchedLinear               (reference src/pytorch/BatchedNN.cpp:48-50)
//
// Differences that are deliberate:
//   * the AEV / CFConv / BatchedNN ops have no CPU implementation: a CPU tensor raises (the reference's CPU path is the
//     oracle of this repository, not part of the product).  The three ops for which the reference itself registers a CPU
//     kernel at the dispatcher -- neighbors::getNeighborPairs, pme::pme_direct and pme::pme_reciprocal -- do have a CPU key here (plain C++
//     loops pinned to the reference's CPU ops by fixtures, tests/test_neighbors_cpu_key.py, tests/test_pme_cpu.py, tests/test_pme_reciprocal_cpu.py);
//   * outputs are fresh tensors on every call (the reference re-returns the same storage,
//     SymmetryFunctions.cpp:136-138,157) -- no caller can observe the difference except by aliasing bugs;
//   * CFConv honours the current stream (the reference leaves that commented out, CFConv.cpp:167-170).
#include <atomic>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/fft.h>
#include <torch/script.h>
#include <torch/serialize/archive.h>

#include <array>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nnpops_hip.h"

// hash of the sources this binding was compiled from (torch_binding.py embeds it and refuses a stale binary)
#ifndef NNPOPS_BINDING_HASH
#define NNPOPS_BINDING_HASH "unknown"
#endif
extern "C" __attribute__((used, visibility("default"))) const char nnpops_torch_binding_version[] =
    "nnpops_torch_binding src:" NNPOPS_BINDING_HASH;

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::tensor_list;

[[noreturn]] void raise_last(const char* what) {
    throw std::runtime_error(std::string(what) + ": " + nnpops_last_error());
}

void* current_stream(const torch::Device& device) {
    return (void*)c10::hip::getCurrentHIPStream(device.index()).stream();
}

bool stream_is_capturing(void* stream) {
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &status) != hipSuccess) return false;
    return status != hipStreamCaptureStatusNone;
}

// ---------------------------------------------------------------------------------------------
// The atomic networks of a frame on nnpops_mlp_forward / nnpops_mlp_input_grad (mlp_fused.hip).  The packed parameters
// travel as two flat buffers (what nnpops_amd/BatchedNN.py::_FusedSpeciesNN registers): per kind, one after the other,
//   planes (fp16): w0 (M members) | w2 (M) | w4 (M) | w4t (M) | w2t (M) | w0t          floats: b0 | b2 | b4 | w6 | b6
// with the packed widths h1, h2, h3 of every kind in `widths` (multiples of 32).  With x_blocks (the 16-column blocks of x
// the networks are packed over, nnpops_hip.h: x_groups) the first layer's planes are that narrow, and when they hold at most
// 256 columns every kind carries one more set, w0tm (M), behind w0t: the forward launch then forms the input gradient itself.
// ---------------------------------------------------------------------------------------------
struct MlpCall {
    nnpops_mlp_frame frame{};
    Tensor energies;                  // [atoms][members]
    std::vector<Tensor> keep;         // workspaces
};
// workspaces of a frame that a caller with a home for them (the AEV holder of the one-node step) keeps between the steps
struct MlpScratch {
    Tensor partial, energies;
    std::vector<Tensor> d1;           // (FusedMLPMembers: the node's own dE/dy1 planes, one per kind, handed back to its backward)
};

int64_t mlp_halves(int64_t rows, int64_t cols) { return nnpops_mlp_packed_halves((int)rows, (int)cols); }

MlpCall mlp_prepare(const Tensor& x, const Tensor& rows, const std::vector<int64_t>& kind_atoms, const std::vector<int64_t>& widths,
                    int64_t members, const Tensor& planes, const Tensor& floats, bool with_gradient,
                    const c10::optional<Tensor>& x_blocks = c10::nullopt, const c10::optional<Tensor>& dead_blocks = c10::nullopt,
                    int64_t act_scale_log2 = 4, MlpScratch* scratch = nullptr) {
    TORCH_CHECK(act_scale_log2 >= 4 && act_scale_log2 <= 12, "act_scale_log2: 4..12 (activations are scaled by 2^-k before the fp16 split)");
    TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.scalar_type() == torch::kFloat32 && x.is_contiguous(),
                "the fused networks take a contiguous [atoms, features] float32 device tensor");
    const bool narrow = x_blocks.has_value() && x_blocks->numel() > 0;
    const int64_t kinds = (int64_t)kind_atoms.size(), atoms = x.size(0), F = narrow ? 16 * x_blocks->numel() : x.size(1);
    if (narrow) {
        TORCH_CHECK(x.size(1) % 16 == 0 && F <= x.size(1), "x_blocks: blocks of 16 columns of a [atoms, multiple of 16] array");
        for (const Tensor* t : {&*x_blocks, dead_blocks.has_value() ? &*dead_blocks : &*x_blocks})
            TORCH_CHECK(t->scalar_type() == torch::kInt32 && t->is_contiguous() && t->device() == x.device(), "column block lists must be int32 on the device of x");
        TORCH_CHECK(dead_blocks.has_value() && x_blocks->numel() + dead_blocks->numel() == x.size(1) / 16,
                    "x_blocks and dead_blocks together must list every 16-column block of x once");
    }
    const bool in_forward = narrow && with_gradient && F <= 256;
    TORCH_CHECK(kinds >= 1 && kinds <= NNPOPS_MLP_MAX_KINDS && (int64_t)widths.size() == 3 * kinds, "1..", NNPOPS_MLP_MAX_KINDS, " kinds, three widths each");
    TORCH_CHECK(rows.scalar_type() == torch::kInt32 && rows.is_contiguous() && rows.device() == x.device() && rows.numel() == atoms,
                "rows must be an int32 permutation of the atoms on the device of x");
    TORCH_CHECK(planes.scalar_type() == torch::kFloat16 && planes.is_contiguous() && planes.device() == x.device() &&
                floats.scalar_type() == torch::kFloat32 && floats.is_contiguous() && floats.device() == x.device(),
                "packed network parameters must be contiguous fp16 / fp32 buffers on the device of x");
    MlpCall c;
    nnpops_mlp_frame& fr = c.frame;
    fr.num_kinds = (int)kinds; fr.num_features = (int)F; fr.num_members = (int)members;
    fr.x = x.data_ptr<float>(); fr.ldx = (int)x.size(1); fr.rows = rows.data_ptr<int32_t>(); fr.alpha = 0.1f; fr.act_scale_log2 = (int)act_scale_log2;       // BatchedNN.py:103
    if (narrow) {
        fr.x_groups = x_blocks->data_ptr<int32_t>();
        fr.dead_groups = dead_blocks->numel() ? dead_blocks->data_ptr<int32_t>() : nullptr;
        fr.num_dead_groups = (int)dead_blocks->numel();
    }
    auto fresh = [&](Tensor& kept, at::IntArrayRef shape) {      // (a kept workspace of the right shape on the right device, or a new one)
        if (!kept.defined() || kept.sizes() != shape || kept.device() != x.device()) kept = torch::empty(shape, x.options());
        return kept;
    };
    if (in_forward) {
        Tensor local;
        Tensor partial = fresh(scratch ? scratch->partial : local, {members, atoms, F});
        fr.dx_partial = partial.data_ptr<float>();
        c.keep.push_back(partial);
    }
    {
        Tensor local;
        c.energies = fresh(scratch ? scratch->energies : local, {atoms, members});
    }
    fr.energies = c.energies.data_ptr<float>();
    const at::Half* ph = planes.data_ptr<at::Half>();
    const float* pf = floats.data_ptr<float>();
    int64_t oh = 0, of = 0, total = 0;
    for (int64_t k = 0; k < kinds; k++) {
        const int64_t h1 = widths[3 * k], h2 = widths[3 * k + 1], h3 = widths[3 * k + 2], M = members;
        nnpops_mlp_kind& kd = fr.kinds[k];
        kd.num_atoms = (int)kind_atoms[k]; kd.h1 = (int)h1; kd.h2 = (int)h2; kd.h3 = (int)h3;
        total += kind_atoms[k];
        kd.w0 = ph + oh;  oh += M * mlp_halves(h1, F);
        kd.w2 = ph + oh;  oh += M * mlp_halves(h2, h1);
        kd.w4 = ph + oh;  oh += M * mlp_halves(h3, h2);
        kd.w4t = ph + oh; oh += M * mlp_halves(h2, h3);
        kd.w2t = ph + oh; oh += M * mlp_halves(h1, h2);
        kd.w0t = ph + oh; oh += mlp_halves(F, M * h1);
        if (narrow && F <= 256) { kd.w0tm = ph + oh; oh += M * mlp_halves(F, h1); }
        kd.b0 = pf + of; of += M * h1;
        kd.b2 = pf + of; of += M * h2;
        kd.b4 = pf + of; of += M * h3;
        kd.w6 = pf + of; of += M * h3;
        kd.b6 = pf + of; of += M;
        if (with_gradient && !in_forward) {
            const int64_t halves = std::max<int64_t>(nnpops_mlp_d1_halves((int)kind_atoms[k], (int)M, (int)h1), 1);
            Tensor d1 = scratch && k < (int64_t)scratch->d1.size() && scratch->d1[k].numel() == halves && scratch->d1[k].device() == x.device()
                ? scratch->d1[k] : torch::empty({halves}, planes.options());
            kd.d1 = d1.data_ptr();
            c.keep.push_back(d1);
        }
    }
    TORCH_CHECK(total == atoms, "the kinds hold ", total, " atoms, x has ", atoms);
    TORCH_CHECK(oh == planes.numel() && of == floats.numel(), "packed network parameters do not match the widths (", oh, " / ", planes.numel(),
                " fp16 values, ", of, " / ", floats.numel(), " floats)");
    return c;
}

// where the next nnpops_mlp_input_grad of the frame writes, and the factor on it
void mlp_point_gradient(nnpops_mlp_frame& fr, const Tensor& dx, float scale) {
    fr.dx = dx.data_ptr<float>(); fr.lddx = (int)dx.size(1); fr.dx_scale = scale;
}
// the upstream gradient of every (molecule, member) -- weights [B, M], float32, contiguous -- as the weights of the frame's gradient
// passes (nnpops_hip.h: member_weights), with the molecule offsets of a batch
void mlp_point_upstream(nnpops_mlp_frame& fr, const Tensor& weights, const c10::optional<Tensor>& offsets) {
    fr.member_weights = weights.data_ptr<float>(); fr.member_weights_ld = (int)weights.size(1);
    if (offsets.has_value()) { fr.segment_offsets = offsets->data_ptr<int32_t>(); fr.num_segments = (int)weights.size(0); }
}

// `shift`, the self energy added in double precision: who ("energy():") asks, and on whose device ("the positions")
void check_shift(const c10::optional<Tensor>& shift, const torch::Device& device, const char* who, const char* whose) {
    if (shift.has_value())
        TORCH_CHECK(shift->scalar_type() == torch::kFloat64 && shift->device() == device && shift->numel() == 1 && shift->is_contiguous(),
                    who, " the self-energy shift must be one float64 on the device of ", whose);
}

// The reduction of a frame's per-atom energies [atoms][members] into `out`, one small launch: every member's sum over the atoms of a
// molecule, out [B, M] (members); the ensemble mean of every molecule, out [B] (mean: the factor 1 / M); or the plain sum over atoms
// and members (total: the factor 1).  offsets / places: the tables of a batch, or NULL for one molecule.  With `shift`, out is float64.
enum class MlpReduce : int64_t { members = 0, mean = 1, total = 2 };

void mlp_reduce(void* stream, const MlpCall& call, int64_t members, const Tensor* offsets, const Tensor* places, MlpReduce mode,
                const c10::optional<Tensor>& shift, Tensor& out, const char* op) {
    const float* e = call.energies.data_ptr<float>();
    const int atoms = (int)call.energies.size(0), M = (int)members, count = (int)out.size(0);
    const int32_t* off = offsets ? offsets->data_ptr<int32_t>() : nullptr;
    const int32_t* plc = places ? places->data_ptr<int32_t>() : nullptr;
    const float scale = mode == MlpReduce::total ? 1.0f : 1.0f / (float)members;
    int rc;
    if (mode == MlpReduce::members)
        rc = shift.has_value() ? nnpops_mlp_member_sums_shifted(stream, e, atoms, M, off, count, plc, shift->data_ptr<double>(), out.data_ptr<double>())
                               : nnpops_mlp_member_sums(stream, e, atoms, M, off, count, plc, out.data_ptr<float>());
    else if (off)
        rc = shift.has_value() ? nnpops_mlp_energy_mean_segments_shifted(stream, e, atoms, M, off, count, plc, scale, shift->data_ptr<double>(), out.data_ptr<double>())
                               : nnpops_mlp_energy_mean_segments(stream, e, atoms, M, off, count, plc, scale, out.data_ptr<float>());
    else
        rc = shift.has_value() ? nnpops_mlp_energy_mean_shifted(stream, e, call.energies.numel(), scale, shift->data_ptr<double>(), out.data_ptr<double>())
                               : nnpops_mlp_energy_mean(stream, e, call.energies.numel(), scale, out.data_ptr<float>());
    if (rc != NNPOPS_OK) raise_last(op);
}

void require_device_tensor(const Tensor& t, const char* name) {
    if (!t.is_cuda())
        throw std::runtime_error(std::string("Unsupported device for \"") + name + "\": " + t.device().str() +
                                 " (this build of NNPOps runs on AMD GPUs only; there is no CPU path)");
}

}  // namespace

// =============================================================================================
// ANI symmetry functions
// =============================================================================================
namespace NNPOps {
namespace ANISymmetryFunctions {

class Holder;
using HolderPtr = torch::intrusive_ptr<Holder>;

class Holder : public torch::CustomClassHolder {
public:
    Holder(int64_t numSpecies, double Rcr, double Rca, const std::vector<double>& EtaR, const std::vector<double>& ShfR,
           const std::vector<double>& EtaA, const std::vector<double>& Zeta, const std::vector<double>& ShfA,
           const std::vector<double>& ShfZ, const std::vector<int64_t>& atomSpecies)
        : numSpecies(numSpecies), Rcr(Rcr), Rca(Rca), EtaR(EtaR), ShfR(ShfR), EtaA(EtaA), Zeta(Zeta), ShfA(ShfA), ShfZ(ShfZ),
          atomSpecies(atomSpecies) {}

    ~Holder() override {
        if (impl) nnpops_ani_destroy(impl);
    }

    // Additive: how often forward() pays the host round trip that verifies the neighbour capacities (and grows them).
    // 1 (default) = every call, k = every k-th call, 0 = only the first.  Between checks an overflow goes unnoticed, as
    // inside a captured graph -- for production loops whose densities are known (cf. getNeighborPairs' checkErrors).
    // Extension: the builders' sticky overflow word as an int32[1] DEVICE tensor (no copy, no synchronisation): non-zero when a
    // forward since the last capacity check overflowed a neighbour buffer -- what a caller replaying a captured graph, where no
    // check can run, looks at (nnpops_hip.h: nnpops_ani_overflow_word).  Needs one forward() first.
    Tensor overflowFlag() {
        if (!impl) throw std::runtime_error("overflow_flag() called before forward()");
        const int32_t* word = nullptr;
        if (nnpops_ani_overflow_word(impl, &word) != NNPOPS_OK) raise_last("NNPOpsANISymmetryFunctions::overflow_flag");
        // (the tensor keeps this Holder -- and with it the handle that owns the word -- alive: ADVICE r04; the word itself is cleared by
        //  every capacity check, so "sticky" means between two checks)
        auto self = c10::intrusive_ptr<Holder>::unsafe_reclaim_from_nonowning(this);
        return torch::from_blob(const_cast<int32_t*>(word), {1}, [self](void*) {}, torch::TensorOptions().device(device).dtype(torch::kInt32));
    }

    void setCheckInterval(int64_t interval) {
        if (interval < 0) throw std::runtime_error("The check interval has to be >= 0");
        checkInterval = interval;
    }

    // Additive (the reference has no batch dimension, SymmetryFunctions.py:110): the atoms of this Holder
    // are `offsets.size() - 1` independent molecules, molecule m = atoms [offsets[m], offsets[m+1]); atoms of
    // different molecules never see each other, forward/backward evaluate the whole batch in one launch sequence
    // (nnpops_ani_set_molecules).  A Holder first used with a cell evaluates a PERIODIC batch: the cell is then [molecules, 3, 3],
    // a box for every molecule, and so is its gradient.  An empty list restores the single-system behaviour.
    void setMolecules(const std::vector<int64_t>& offsets) {
        if (!offsets.empty() && (offsets.front() != 0 || offsets.back() != (int64_t)atomSpecies.size()))
            throw std::runtime_error("molecule offsets have to start at 0 and end at the number of atoms");
        moleculeOffsets = offsets;
        if (impl) applyMolecules();
    }

    tensor_list forward(const Tensor& positions, const c10::optional<Tensor>& cellOpt) { return forwardImpl(positions, cellOpt, false); }

    // fused = true: ONE output, aev [N, S*nR + S(S+1)/2*nA] = (radial | angular) per row -- what TorchANI's AEVComputer
    // returns and what the Python wrapper otherwise builds with torch.cat: the kernels write the two parts in place
    // (nnpops_ani_compute_strided), no concatenation copy forward, no split copy backward.
    // defer_check: a caller with more launches to queue behind the AEV (EnergyFunction) takes the capacity check in two halves --
    // the copy of the overflow word is queued here, finishDeferredCheck() reads it after those launches (nnpops_hip.h:
    // nnpops_ani_check_begin / _end), so the host round trip no longer stops the device between the AEV and its consumers.
    tensor_list forwardImpl(const Tensor& positions, const c10::optional<Tensor>& cellOpt, bool fused, bool defer_check = false) {
        // same checks, same messages as the reference (SymmetryFunctions.cpp:76-99)
        if (positions.scalar_type() != torch::kFloat32) throw std::runtime_error("The type of \"positions\" has to be float32");
        if (positions.dim() != 2) throw std::runtime_error("The shape of \"positions\" has to have 2 dimensions");
        if (positions.size(0) != (int64_t)atomSpecies.size())
            throw std::runtime_error("The size of the 1nd dimension of \"positions\" has to be " + std::to_string(atomSpecies.size()));
        if (positions.size(1) != 3) throw std::runtime_error("The size of the 2nd dimension of \"positions\" has to be 3");
        require_device_tensor(positions, "positions");
        Tensor cell;
        if (cellOpt) {
            cell = *cellOpt;
            if (cell.scalar_type() != torch::kFloat32) throw std::runtime_error("The type of \"cell\" has to be float32");
            if (!moleculeOffsets.empty()) {
                // a periodic batch (setMolecules): one box per molecule, [molecules, 3, 3] (nnpops_ani_set_molecules on a periodic handle)
                if (cell.dim() != 3 || cell.size(0) != moleculeCount() || cell.size(1) != 3 || cell.size(2) != 3)
                    throw std::runtime_error("The shape of \"cell\" has to be [" + std::to_string(moleculeCount()) +
                                             ", 3, 3]: this Holder evaluates a batch of molecules, one box for each");
            } else {
            if (cell.dim() != 2) throw std::runtime_error("The shape of \"cell\" has to have 2 dimensions");
            if (cell.size(0) != 3) throw std::runtime_error("The size of the 1nd dimension of \"cell\" has to be 3");
            if (cell.size(1) != 3) throw std::runtime_error("The size of the 2nd dimension of \"cell\" has to be 3");
            }
            if (cell.device() != positions.device()) throw std::runtime_error("\"cell\" has to be on the same device as \"positions\"");
            cell = cell.contiguous();
        }
        if (!impl) {
            device = positions.device();
            periodic = cellOpt.has_value();       // frozen at the first call, like the reference (:122)
            std::vector<float> radial, angular;
            for (double eta : EtaR)
                for (double rs : ShfR) { radial.push_back((float)eta); radial.push_back((float)rs); }              // :110-113
            for (double eta : EtaA)
                for (double zeta : Zeta)
                    for (double rs : ShfA)
                        for (double thetas : ShfZ) {                                                              // :115-120
                            angular.push_back((float)eta); angular.push_back((float)rs);
                            angular.push_back((float)zeta); angular.push_back((float)thetas);
                        }
            std::vector<int32_t> species(atomSpecies.begin(), atomSpecies.end());
            if (nnpops_ani_create(&impl, (int)species.size(), (int)numSpecies, (float)Rcr, (float)Rca, periodic ? 1 : 0,
                                  species.data(), (int)(radial.size() / 2), radial.data(), (int)(angular.size() / 4),
                                  angular.data(), /*torchani=*/1, device.index()) != NNPOPS_OK)
                raise_last("NNPOpsANISymmetryFunctions");
            numRadial = (int64_t)(radial.size() / 2);
            numAngular = (int64_t)(angular.size() / 4);
            if (!moleculeOffsets.empty()) applyMolecules();
        }
        if (positions.device() != device) throw std::runtime_error("The device of \"positions\" has changed");
        if (periodic && !cellOpt) throw std::runtime_error("\"cell\" is required: this Holder was first used with periodic box vectors");

        const Tensor pos = positions.contiguous();
        const int64_t n = (int64_t)atomSpecies.size();
        const auto opts = torch::TensorOptions().device(device).dtype(torch::kFloat32);
        const int64_t wr = numSpecies * numRadial, wa = numSpecies * (numSpecies + 1) / 2 * numAngular;
        Tensor radial, angular, aev;
        float *pr, *pa;
        int ld = 0;
        if (fused) {
            aev = torch::empty({n, wr + wa}, opts);
            pr = aev.data_ptr<float>(); pa = pr + wr; ld = (int)(wr + wa);
        } else {
            radial = torch::empty({n, wr}, opts);
            angular = torch::empty({n, wa}, opts);
            pr = radial.data_ptr<float>(); pa = angular.data_ptr<float>();
        }
        void* stream = current_stream(device);
        nnpops_ani_set_stream(impl, stream);
        const bool capturing = stream_is_capturing(stream);
        buildCount++;                                 // the lists are rebuilt: a recorded backward of an earlier forward is stale (AevBackwardFunction)
        for (int attempt = 0;; attempt++) {
            if (nnpops_ani_compute_strided(impl, pos.data_ptr<float>(), periodic ? cell.data_ptr<float>() : nullptr, pr, ld, pa, ld) !=
                NNPOPS_OK)
                raise_last("NNPOpsANISymmetryFunctions::forward");
            if (capturing) break;                     // no host synchronisation inside a graph capture
            // (additive knob, like getNeighborPairs' checkErrors: the capacity check costs a host round trip;
            // interval k checks every k-th call, 0 never again after the first)
            // (forceCheck: this is the re-issue of a step whose deferred check reported an overflow -- a second overflow, e.g. row
            //  capacity after the cell bins, must be caught now, whatever the interval; the re-issue is not a counted call)
            const bool due = forceCheck || calls == 0 || (checkInterval > 0 && calls % checkInterval == 0);
            if (!forceCheck) calls++;
            forceCheck = false;
            if (!due && attempt == 0) break;
            if (defer_check && publishInline) {                // (the caller's next launch publishes the word: energy_step)
                if (nnpops_ani_check_begin_with(impl, &publishWord, &publishTo, &publishStamp) == 1) { checkPending = true; break; }
                publishWord = nullptr;
            } else if (defer_check && nnpops_ani_check_begin(impl) == 1) { checkPending = true; break; }
            const int rc = nnpops_ani_check(impl, nullptr, nullptr);
            if (rc == NNPOPS_OK) break;
            if (rc != NNPOPS_ERR_CAPACITY || attempt > 8) raise_last("NNPOpsANISymmetryFunctions::forward");
        }
        if (fused) return {aev};
        return {radial, angular};
    }

    tensor_list backwardFused(const Tensor& aevGrad) {
        if (!impl) throw std::runtime_error("backward() called before forward()");
        const Tensor g = aevGrad.contiguous();
        const int64_t wr = numSpecies * numRadial, w = g.size(1);
        Tensor positionsGrad = torch::empty({(int64_t)atomSpecies.size(), 3},
                                            torch::TensorOptions().device(device).dtype(torch::kFloat32));
        nnpops_ani_set_stream(impl, current_stream(device));
        if (nnpops_ani_backprop_strided(impl, g.data_ptr<float>(), (int)w, g.data_ptr<float>() + wr, (int)w,
                                        positionsGrad.data_ptr<float>()) != NNPOPS_OK)
            raise_last("NNPOpsANISymmetryFunctions::backward");
        return {Tensor(), positionsGrad, Tensor()};
    }

    tensor_list backward(const tensor_list& grads) {
        if (!impl) throw std::runtime_error("backward() called before forward()");
        const Tensor radialGrad = grads[0].contiguous();     // the reference clones to force a dense buffer (:162-163)
        const Tensor angularGrad = grads[1].contiguous();
        Tensor positionsGrad = torch::empty({(int64_t)atomSpecies.size(), 3},
                                            torch::TensorOptions().device(device).dtype(torch::kFloat32));
        nnpops_ani_set_stream(impl, current_stream(device));
        if (nnpops_ani_backprop(impl, radialGrad.data_ptr<float>(), angularGrad.data_ptr<float>(),
                                positionsGrad.data_ptr<float>()) != NNPOPS_OK)
            raise_last("NNPOpsANISymmetryFunctions::backward");
        return {Tensor(), positionsGrad, Tensor()};          // no gradient for the holder and the box (:174)
    }

    // Additive: the tangent J.v of the AEV of the last forward along v [N, 3] (nnpops_ani_tangent_strided) -- the adjoint of backward(),
    // what the parameter gradient of a force loss needs of the AEV.  tangent(): the fused layout [N, W_r + W_a] of aev();
    // tangentSplit(): {radial [N, W_r], angular [N, W_a]} as operation() returns them.
    Tensor tangent(const Tensor& v) {
        const int64_t wr = numSpecies * numRadial, wa = numSpecies * (numSpecies + 1) / 2 * numAngular;
        Tensor out = torch::empty({(int64_t)atomSpecies.size(), wr + wa}, torch::TensorOptions().device(device).dtype(torch::kFloat32));
        tangentInto(v, out.data_ptr<float>(), (int)(wr + wa), out.data_ptr<float>() + wr, (int)(wr + wa));
        return out;
    }
    tensor_list tangentSplit(const Tensor& v) {
        const int64_t wr = numSpecies * numRadial, wa = numSpecies * (numSpecies + 1) / 2 * numAngular;
        const auto opts = torch::TensorOptions().device(device).dtype(torch::kFloat32);
        Tensor radial = torch::empty({(int64_t)atomSpecies.size(), wr}, opts), angular = torch::empty({(int64_t)atomSpecies.size(), wa}, opts);
        tangentInto(v, radial.data_ptr<float>(), 0, angular.data_ptr<float>(), 0);
        return {radial, angular};
    }
    int64_t getBuildCount() const { return buildCount; }

    // The two backward forms WITH the gradient of the box vectors (nnpops_ani_backprop_box_strided): `positions` and `cell` are the
    // tensors of the forward this backward belongs to -- the minimum-image shifts are recovered from them.  -> {none, dL/dpositions,
    // dL/dcell [3, 3] -- [molecules, 3, 3] for a periodic batch}; the position gradient is the one backward() / backwardFused() return, bit for bit.
    tensor_list backwardFusedCell(const Tensor& aevGrad, const Tensor& positions, const Tensor& cell) {
        const Tensor g = aevGrad.contiguous();
        const int64_t wr = numSpecies * numRadial, w = g.size(1);
        return backpropCell(g.data_ptr<float>(), (int)w, g.data_ptr<float>() + wr, (int)w, positions, cell);
    }
    tensor_list backwardCell(const tensor_list& grads, const Tensor& positions, const Tensor& cell) {
        const Tensor radialGrad = grads[0].contiguous(), angularGrad = grads[1].contiguous();
        return backpropCell(radialGrad.data_ptr<float>(), 0, angularGrad.data_ptr<float>(), 0, positions, cell);
    }

    static std::string serialize(const HolderPtr& self) {
        torch::serialize::OutputArchive archive;
        archive.write("numSpecies", self->numSpecies);
        archive.write("Rcr", self->Rcr);
        archive.write("Rca", self->Rca);
        archive.write("EtaR", self->EtaR);
        archive.write("ShfR", self->ShfR);
        archive.write("EtaA", self->EtaA);
        archive.write("Zeta", self->Zeta);
        archive.write("ShfA", self->ShfA);
        archive.write("ShfZ", self->ShfZ);
        archive.write("atomSpecies", self->atomSpecies);
        std::stringstream stream;
        archive.save_to(stream);
        return stream.str();
    }

    // -> true: the neighbour buffers had overflowed and have been grown; the caller issues forwardImpl() and its consumers again
    bool finishDeferredCheck() {
        if (!checkPending) return false;
        checkPending = false;
        const int rc = nnpops_ani_check_end(impl);
        if (rc == NNPOPS_OK) return false;
        if (rc != NNPOPS_ERR_CAPACITY) raise_last("NNPOpsANISymmetryFunctions::forward");
        forceCheck = true;              // the caller issues the step again: that build is verified whatever the check interval
        return true;
    }

    static HolderPtr deserialize(const std::string& state) {
        std::stringstream stream(state);
        torch::serialize::InputArchive archive;
        archive.load_from(stream, torch::kCPU);
        torch::IValue numSpecies, Rcr, Rca, EtaR, ShfR, EtaA, Zeta, ShfA, ShfZ, atomSpecies;
        archive.read("numSpecies", numSpecies);
        archive.read("Rcr", Rcr);
        archive.read("Rca", Rca);
        archive.read("EtaR", EtaR);
        archive.read("ShfR", ShfR);
        archive.read("EtaA", EtaA);
        archive.read("Zeta", Zeta);
        archive.read("ShfA", ShfA);
        archive.read("ShfZ", ShfZ);
        archive.read("atomSpecies", atomSpecies);
        return HolderPtr::make(numSpecies.toInt(), Rcr.toDouble(), Rca.toDouble(), EtaR.toDoubleVector(), ShfR.toDoubleVector(),
                               EtaA.toDoubleVector(), Zeta.toDoubleVector(), ShfA.toDoubleVector(), ShfZ.toDoubleVector(),
                               atomSpecies.toIntVector());
    }

private:
    tensor_list backpropCell(const float* radialGrad, int ldRadial, const float* angularGrad, int ldAngular, const Tensor& positions,
                             const Tensor& cell) {
        if (!impl) throw std::runtime_error("backward() called before forward()");
        const Tensor pos = positions.contiguous(), box = cell.contiguous();
        const auto opts = torch::TensorOptions().device(device).dtype(torch::kFloat32);
        Tensor positionsGrad = torch::empty({(int64_t)atomSpecies.size(), 3}, opts), cellGrad = torch::empty(box.sizes(), opts);
        nnpops_ani_set_stream(impl, current_stream(device));
        if (nnpops_ani_backprop_box_strided(impl, pos.data_ptr<float>(), box.data_ptr<float>(), radialGrad, ldRadial, angularGrad, ldAngular,
                                            positionsGrad.data_ptr<float>(), cellGrad.data_ptr<float>()) != NNPOPS_OK)
            raise_last("NNPOpsANISymmetryFunctions::backward");
        return {Tensor(), positionsGrad, cellGrad};
    }

    void tangentInto(const Tensor& v, float* radial, int ldRadial, float* angular, int ldAngular) {
        if (!impl) throw std::runtime_error("tangent() called before forward()");
        TORCH_CHECK(v.defined() && v.scalar_type() == torch::kFloat32 && v.dim() == 2 && v.size(0) == (int64_t)atomSpecies.size() && v.size(1) == 3,
                    "NNPOpsANISymmetryFunctions::tangent: the tangent has to be a float32 tensor of the shape of \"positions\"");
        TORCH_CHECK(v.device() == device, "NNPOpsANISymmetryFunctions::tangent: the tangent has to be on the device of \"positions\"");
        const Tensor t = v.contiguous();
        nnpops_ani_set_stream(impl, current_stream(device));
        if (nnpops_ani_tangent_strided(impl, t.data_ptr<float>(), radial, ldRadial, angular, ldAngular) != NNPOPS_OK)
            raise_last("NNPOpsANISymmetryFunctions::tangent");
    }

    void applyMolecules() {
        std::vector<int32_t> off(moleculeOffsets.begin(), moleculeOffsets.end());
        if (nnpops_ani_set_molecules(impl, off.empty() ? 0 : (int)off.size() - 1, off.empty() ? nullptr : off.data()) != NNPOPS_OK)
            raise_last("NNPOpsANISymmetryFunctions::set_molecules");
    }

    int64_t numSpecies;
    double Rcr, Rca;
    std::vector<double> EtaR, ShfR, EtaA, Zeta, ShfA, ShfZ;
    std::vector<int64_t> atomSpecies;
    std::vector<int64_t> moleculeOffsets;   // additive: batched molecules (setMolecules)
    torch::Device device = torch::kCPU;
    bool periodic = false;
    int64_t numRadial = 0, numAngular = 0;
    nnpops_ani_t impl = nullptr;
    int64_t checkInterval = 1;      // capacity check every k-th forward (0: only the first); see setCheckInterval
    bool forceCheck = false;        // the next forwardImpl() re-issues a step after a reported overflow: always checked
    int64_t calls = 0;
    int64_t buildCount = 0;         // forwardImpl() calls so far: which build of the lists a recorded backward belongs to
    bool checkPending = false;
public:
    // energy_step: the capacity check's word is published by nnpops_mlp_forward (frame.publish_*) instead of a launch of its own
    bool publishInline = false;
    const int32_t* publishWord = nullptr; int32_t* publishTo = nullptr; int32_t publishStamp = 0;
    // energy_step: dE/dAEV of the frame, kept between the steps.  The networks write only the column blocks the molecule's species
    // can fill (x_blocks); the others are zero and stay zero -- cleared once, when the buffer is made, instead of by every step
    // (7 of the 8 MB a step of the 2 001-atom water box used to write there).  Valid for one list of live blocks.
    Tensor gradCache;
    const void* gradCacheBlocks = nullptr;
    Tensor gradCacheKey;              // the list of live blocks itself, held: while the cache is valid its address cannot be freed and handed to
    uint32_t gradCacheVersion = 0;    //   another list, and an in-place edit of the list shows in its version counter
    MlpScratch mlpScratch;            // ... and the networks' workspaces of a step (per-member gradient shares, per-atom energies)
    void resetGradientCache() { gradCache = Tensor(); gradCacheBlocks = nullptr; gradCacheKey = Tensor(); }      // (the networks' live blocks have changed: BatchedNN.py)
    // energy_step over a batch: the device tables the per-molecule mean and the per-molecule backward walk (molecule offsets, place of
    // every row in the species-grouped order) are compared ONCE with what this holder was told (setMolecules) and with `rows` -- one
    // host round trip for a given triple of tensors, held here so that their addresses cannot be handed to other tensors meanwhile.
    int64_t moleculeCount() const { return moleculeOffsets.empty() ? 0 : (int64_t)moleculeOffsets.size() - 1; }
    int64_t atomCount() const { return (int64_t)atomSpecies.size(); }
    void verifyBatchTables(const Tensor& offsets, const Tensor& places, const Tensor& rows, bool capturing) {
        const Tensor* given[3] = {&offsets, &places, &rows};
        bool known = true;
        for (int i = 0; i < 3; i++)
            known = known && batchTables[i].defined() && batchTables[i].is_same(*given[i]) && batchTableVersions[i] == given[i]->_version();
        if (known) return;
        TORCH_CHECK(!capturing, "energy_batch(): the molecule tables of a batch are verified on their first use, which cannot happen inside a graph "
                                "capture: evaluate the batch once before capturing");
        const Tensor want = torch::tensor(moleculeOffsets, torch::TensorOptions().dtype(torch::kInt32));
        TORCH_CHECK(torch::equal(offsets.cpu(), want), "energy_batch(): the molecule offsets are not the ones of the holder (Holder.set_molecules)");
        const Tensor back = places.index_select(0, rows.to(torch::kLong));
        TORCH_CHECK(torch::equal(back.cpu(), torch::arange(rows.numel(), torch::TensorOptions().dtype(torch::kInt32))),
                    "energy_batch(): row_positions is not the inverse of rows");
        for (int i = 0; i < 3; i++) { batchTables[i] = *given[i]; batchTableVersions[i] = given[i]->_version(); }
    }
private:
    Tensor batchTables[3];
    uint32_t batchTableVersions[3] = {0, 0, 0};
};

// Both nodes: `cellGrad` (decided by the caller, where grad mode is what the user set) = the box vectors require a gradient.  The node
// then saves positions and cell, its backward runs the box-gradient pass behind the usual launches and fills the cell's slot; otherwise
// it does exactly what it always did -- nothing saved, no extra launch, no gradient for the box (reference :174).
bool wants_cell_gradient(const c10::optional<Tensor>& periodicBoxVectors) {
    return torch::GradMode::is_enabled() && periodicBoxVectors.has_value() && periodicBoxVectors->requires_grad();
}
void refuse_second_derivatives(const char* op) {
    TORCH_CHECK(!torch::GradMode::is_enabled(), "NNPOpsANISymmetryFunctions::", op,
                ": second derivatives are not implemented (backward was called with create_graph=True and the cell requires a gradient)");
}

// The backward of the two nodes below, RECORDED: dL/dpositions = J^T g as a function of the AEV cotangent(s) g -- it is linear in them,
// so its own backward, given the cotangent v of the position gradient, is the tangent J.v (Holder::tangent) in the slot(s) of g.  That is
// all the parameter gradient of a force loss needs: with F = -J^T g(theta, aev) it is (dg/dtheta)^T (J.v), and autograd carries J.v on
// through the networks that made g.  What it does NOT provide is refused, never dropped: the gradient of this node in the POSITIONS
// (second derivatives of the AEV: Hessians, a force loss differentiated in the coordinates), a third derivative, and a tangent on lists
// that a later forward of the same holder has rebuilt.  Tensor inputs: the cotangent(s) first, the positions last.
void check_same_build(const HolderPtr& holder, int64_t build, const char* op) {
    TORCH_CHECK(holder->getBuildCount() == build, "NNPOpsANISymmetryFunctions::", op, ": the holder has run another forward pass since the one "
                "this derivative belongs to; its neighbour lists were rebuilt and no longer belong to these positions (run the forward "
                "pass and take every derivative of it before the next forward pass on the same holder)");
}

class AevBackwardFunction : public torch::autograd::Function<AevBackwardFunction> {
public:
    // angularGrad: empty for the fused layout (aev), where `grad` is the whole [N, W_r + W_a] cotangent
    static Tensor forward(AutogradContext* ctx, const Tensor& grad, const c10::optional<Tensor>& angularGrad, const Tensor& positions,
                          const HolderPtr& holder, int64_t build) {
        const bool fused = !angularGrad.has_value();
        check_same_build(holder, build, fused ? "aev" : "operation");
        ctx->saved_data["holder"] = holder;
        ctx->saved_data["build"] = build;
        ctx->saved_data["fused"] = fused;
        // (exactly the call the unrecorded backward makes: the same bits)
        return fused ? holder->backwardFused(grad)[1] : holder->backward({grad, *angularGrad})[1];
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const bool fused = ctx->saved_data["fused"].toBool();
        const char* op = fused ? "aev" : "operation";
        const size_t ncot = fused ? 1 : 2;                 // (the node's edges count its tensor inputs only: the positions follow the cotangents)
        TORCH_CHECK(!ctx->needs_input_grad(ncot),"NNPOpsANISymmetryFunctions::", op, ": second derivatives with respect to the positions are not "
                    "implemented (the gradient of a force with respect to the positions was asked for: a Hessian, or loss.backward() on a "
                    "loss of forces, which also differentiates in the positions).  The parameter gradient of a force loss is obtained "
                    "with torch.autograd.grad(loss, parameters) or loss.backward(inputs=parameters)");
        const Tensor& v = grads[0];
        TORCH_CHECK(!(torch::GradMode::is_enabled() && v.defined() && v.requires_grad()), "NNPOpsANISymmetryFunctions::", op,
                    ": third derivatives are not implemented (the derivative of a force was taken with create_graph=True)");
        const auto holder = ctx->saved_data["holder"].toCustomClass<Holder>();
        check_same_build(holder, ctx->saved_data["build"].toInt(), op);
        tensor_list out(5);                                // {cotangent, angular cotangent, positions, holder, build}
        if (!v.defined()) return out;
        if (fused) {
            if (ctx->needs_input_grad(0)) out[0] = holder->tangent(v);
        } else if (ctx->needs_input_grad(0) || ctx->needs_input_grad(1)) {
            const tensor_list t = holder->tangentSplit(v);
            if (ctx->needs_input_grad(0)) out[0] = t[0];
            if (ctx->needs_input_grad(1)) out[1] = t[1];
        }
        return out;
    }
};

// Is the backward in progress one to record?  Grad mode on (create_graph=True) and a cotangent that carries a graph of its own --
// the energy came from networks whose parameters require a gradient.  Everything else takes the plain path: nothing more launched.
bool record_backward(const tensor_list& grads) {
    if (!torch::GradMode::is_enabled()) return false;
    for (const Tensor& g : grads)
        if (g.defined() && g.requires_grad()) return true;
    return false;
}

class AutogradFunctions : public torch::autograd::Function<AutogradFunctions> {
public:
    static tensor_list forward(AutogradContext* ctx, const HolderPtr& holder, const Tensor& positions,
                               const c10::optional<Tensor>& periodicBoxVectors, bool cellGrad) {
        ctx->saved_data["holder"] = holder;
        ctx->saved_data["cell_grad"] = cellGrad;
        if (cellGrad) ctx->save_for_backward({positions, *periodicBoxVectors});
        else ctx->save_for_backward({positions});          // (a reference to an input: what a recorded backward hangs its refusal on)
        tensor_list out = holder->forward(positions, periodicBoxVectors);
        ctx->saved_data["build"] = holder->getBuildCount();
        return out;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const auto holder = ctx->saved_data["holder"].toCustomClass<Holder>();
        tensor_list out;
        if (ctx->saved_data["cell_grad"].toBool()) {
            ctx->saved_data.erase("holder");
            refuse_second_derivatives("operation");
            const auto saved = ctx->get_saved_variables();
            out = holder->backwardCell(grads, saved[0], saved[1]);
        } else if (record_backward(grads)) {
            const Tensor positions = ctx->get_saved_variables()[0];
            out = {Tensor(), AevBackwardFunction::apply(grads[0], c10::optional<Tensor>(grads[1]), positions, holder,
                                                        ctx->saved_data["build"].toInt()), Tensor()};
        } else {
            ctx->saved_data.erase("holder");
            out = holder->backward(grads);
        }
        out.push_back(Tensor());
        return out;
    }
};

tensor_list operation(const c10::optional<HolderPtr>& holder, const Tensor& positions,
                      const c10::optional<Tensor>& periodicBoxVectors) {
    return AutogradFunctions::apply(*holder, positions, periodicBoxVectors, wants_cell_gradient(periodicBoxVectors));
}

class FusedAutogradFunction : public torch::autograd::Function<FusedAutogradFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const HolderPtr& holder, const Tensor& positions,
                          const c10::optional<Tensor>& periodicBoxVectors, bool cellGrad) {
        ctx->saved_data["holder"] = holder;
        ctx->saved_data["cell_grad"] = cellGrad;
        if (cellGrad) ctx->save_for_backward({positions, *periodicBoxVectors});
        else ctx->save_for_backward({positions});          // (a reference to an input: what a recorded backward hangs its refusal on)
        Tensor out = holder->forwardImpl(positions, periodicBoxVectors, true)[0];
        ctx->saved_data["build"] = holder->getBuildCount();
        return out;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const auto holder = ctx->saved_data["holder"].toCustomClass<Holder>();
        tensor_list out;
        if (ctx->saved_data["cell_grad"].toBool()) {
            ctx->saved_data.erase("holder");
            refuse_second_derivatives("aev");
            const auto saved = ctx->get_saved_variables();
            out = holder->backwardFusedCell(grads[0], saved[0], saved[1]);
        } else if (record_backward(grads)) {
            const Tensor positions = ctx->get_saved_variables()[0];
            out = {Tensor(), AevBackwardFunction::apply(grads[0], c10::optional<Tensor>(), positions, holder, ctx->saved_data["build"].toInt()),
                   Tensor()};
        } else {
            ctx->saved_data.erase("holder");
            out = holder->backwardFused(grads[0]);
        }
        out.push_back(Tensor());
        return out;
    }
};

// Additive: the whole AEV as one tensor (see Holder::forwardImpl).  operation() keeps the reference's two-tensor form.
Tensor aev(const c10::optional<HolderPtr>& holder, const Tensor& positions, const c10::optional<Tensor>& periodicBoxVectors) {
    return FusedAutogradFunction::apply(*holder, positions, periodicBoxVectors, wants_cell_gradient(periodicBoxVectors));
}

// ---------------------------------------------------------------------------------------------
// Additive: the whole OptimizedTorchANI step (reference OptimizedTorchANI.py:49-52: aev_computer -> neural_networks) as ONE
// autograd node.  forward: AEV kernels -> the fused networks (mlp_fused.hip) -> ensemble-mean energy; when the positions
// require a gradient the same call runs the networks' input-gradient pass and the AEV backward and keeps dE/dpositions, so
// that backward() is one multiplication -- no autograd graph over the ~20 small tensor ops the four-module composition
// records, no [N, 1008] gradient held by autograd between the passes.  (The reference's PME op keeps its derivatives
// the same way, pmeCPU.cpp:161-171.)
// ---------------------------------------------------------------------------------------------
// One energy (+ gradient) evaluation of the frame: AEV forward, networks, and -- with a gradient -- the networks' input gradient and
// the AEV backward.  Returns {energy [1], dE/dpositions * gradient_sign [N, 3] or undefined}.  (The capacity check of the AEV
// holder -- one host round trip per call unless set_check_interval says otherwise -- is taken in two halves: its word is published
// right behind the AEV forward, read after everything else has been launched.  A buffer that did overflow is grown there and the
// step issued again.  Before: the host waited for the AEV forward, then launched the networks into an idle device; waiting at the
// END of the step for the whole stream was worse still, 0.22 -> 0.28 ms.)
// A batch of molecules behind one step (energy_batch): the tables of nnpops_mlp_energy_mean_segments.  The step differs from the one of a
// single molecule in how the mean is taken -- one per molecule -- and in the shape of what comes back: energy [B], kept [B * N, 3].
struct BatchTables {
    Tensor offsets, places;           // int32 [B + 1], int32 [B * N]
    int64_t molecules;
};

std::pair<Tensor, Tensor> energy_step(const HolderPtr& holder, const Tensor& frame, const c10::optional<Tensor>& cell, const Tensor& rows,
                                      const std::vector<int64_t>& kind_atoms, const std::vector<int64_t>& widths, int64_t members,
                                      const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& shift,
                                      const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks, bool need_gradient,
                                      float gradient_sign, int64_t act_scale_log2, Tensor* kept_cell = nullptr,
                                      const BatchTables* batch = nullptr) {
    // (kept_cell != NULL, with need_gradient: the AEV backward also runs its box-gradient pass and dE/dcell * gradient_sign [3, 3] -- of a periodic batch [B, 3, 3] -- is kept there)
    TORCH_CHECK(batch != nullptr || frame.dim() == 2 || (frame.dim() == 3 && frame.size(0) == 1),
                "energy(): positions must be [atoms, 3] or [1, atoms, 3]");
    const Tensor positions = batch ? frame.reshape({-1, 3}) : frame.dim() == 3 ? frame[0] : frame;
    const int64_t count = batch ? batch->molecules : 1;
    Tensor energy, kept;
    for (int attempt = 0;; attempt++) {
        TORCH_CHECK(attempt <= 8, "NNPOpsANISymmetryFunctions::energy: neighbour buffers kept overflowing");
        holder->publishInline = true; holder->publishWord = nullptr;
        const Tensor aev = holder->forwardImpl(positions, cell, true, /*defer_check=*/true)[0];
        holder->publishInline = false;
        c10::hip::HIPGuard guard(aev.device().index());
        void* stream = current_stream(aev.device());
        MlpCall call = mlp_prepare(aev, rows, kind_atoms, widths, members, planes, floats, need_gradient, x_blocks, dead_blocks, act_scale_log2,
                                   &holder->mlpScratch);
        if (holder->publishWord) {                              // the deferred check's word goes out with the first network launch
            call.frame.publish_word = holder->publishWord; call.frame.publish_to = holder->publishTo; call.frame.publish_stamp = holder->publishStamp;
        }
        if (nnpops_mlp_forward(stream, &call.frame, need_gradient ? 1 : 0) != NNPOPS_OK) raise_last("NNPOpsANISymmetryFunctions::energy");
        // the ensemble mean (BatchedNN.py:109), shifted by the self energy when the caller hands it over: its own small launch,
        // or -- when the input gradient is only a sum over the members (dx_partial) -- a passenger of that launch
        const bool mean_rides = need_gradient && call.frame.dx_partial != nullptr;
        check_shift(shift, aev.device(), "energy():", "the positions");
        energy = torch::empty({count}, shift.has_value() ? aev.options().dtype(torch::kFloat64) : aev.options());
        if (mean_rides) {
            call.frame.mean_scale = 1.0f / (float)members;
            if (shift.has_value()) { call.frame.mean_shift = shift->data_ptr<double>(); call.frame.mean_out_shifted = energy.data_ptr<double>(); }
            else call.frame.mean_out = energy.data_ptr<float>();
            if (batch) {
                call.frame.segment_offsets = batch->offsets.data_ptr<int32_t>(); call.frame.segment_positions = batch->places.data_ptr<int32_t>();
                call.frame.num_segments = (int)count;
            }
        } else {
            mlp_reduce(stream, call, members, batch ? &batch->offsets : nullptr, batch ? &batch->places : nullptr, MlpReduce::mean, shift, energy,
                       batch ? "NNPOpsANISymmetryFunctions::energy_batch" : "NNPOpsANISymmetryFunctions::energy");
        }
        if (need_gradient) {
            Tensor daev;
            if (call.frame.dx_partial != nullptr && x_blocks.has_value()) {     // (the sum over the members writes the live blocks only)
                if (!holder->gradCache.defined() || holder->gradCache.sizes() != aev.sizes() || holder->gradCache.device() != aev.device() ||
                    holder->gradCacheBlocks != x_blocks->data_ptr() || holder->gradCacheVersion != x_blocks->_version()) {
                    holder->gradCache = torch::zeros_like(aev);
                    holder->gradCacheBlocks = x_blocks->data_ptr();
                    holder->gradCacheKey = *x_blocks;
                    holder->gradCacheVersion = x_blocks->_version();
                }
                daev = holder->gradCache;
                call.frame.num_dead_groups = 0;
            } else {
                daev = torch::empty_like(aev);
            }
            mlp_point_gradient(call.frame, daev, gradient_sign / (float)members);
            if (nnpops_mlp_input_grad(stream, &call.frame) != NNPOPS_OK) raise_last("NNPOpsANISymmetryFunctions::energy");
            if (kept_cell != nullptr) {
                TORCH_CHECK(cell.has_value(), "energy(): a gradient of the cell was requested without a cell");
                const tensor_list both = holder->backwardFusedCell(daev, positions, *cell);
                kept = both[1];
                *kept_cell = both[2];
            } else {
                kept = holder->backwardFused(daev)[1];
            }
        }
        if (!holder->finishDeferredCheck()) break;
    }
    return {energy, kept};
}

class EnergyFunction : public torch::autograd::Function<EnergyFunction> {
public:
    // `frame`: positions [N, 3], or [1, N, 3] as the torchani modules pass them (the gradient comes back in the same shape: no
    // select / select-backward kernels around the node).  `shift`: optional float64 device scalar, the molecule's self energy
    // (EnergyShifter.py:52); with it the energy comes back in double precision, promoted and shifted as the reference does it.
    static Tensor forward(AutogradContext* ctx, const HolderPtr& holder, const Tensor& frame, const c10::optional<Tensor>& cell,
                          const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                          const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& shift,
                          const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks, bool need_gradient,
                          int64_t act_scale_log2, bool need_cell) {
        Tensor energy, kept, kept_cell;
        std::tie(energy, kept) = energy_step(holder, frame, cell, rows, kind_atoms, widths, members, planes, floats, shift, x_blocks, dead_blocks,
                                             need_gradient, 1.0f, act_scale_log2, need_cell ? &kept_cell : nullptr);
        if (need_gradient) {
            if (need_cell) ctx->save_for_backward({kept, kept_cell});      // dE/dcell next to dE/dpositions: backward scales both
            else ctx->save_for_backward({kept});
            ctx->saved_data["lead"] = frame.dim() == 3;
        }
        return energy;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        TORCH_CHECK(!torch::GradMode::is_enabled(),
                    "NNPOpsANISymmetryFunctions::energy: second derivatives are not implemented (backward was called with create_graph=True); "
                    "use the four-module composition for that");
        const auto saved = ctx->get_saved_variables();
        TORCH_CHECK(!saved.empty(), "energy() was evaluated without a gradient request");
        const Tensor& kept = saved[0];                                       // dE/dpositions, [N, 3] float32
        const Tensor g = grads[0].contiguous();
        TORCH_CHECK(g.numel() == 1 && g.device() == kept.device() && (g.scalar_type() == torch::kFloat32 || g.scalar_type() == torch::kFloat64),
                    "energy(): unexpected gradient of the energy");
        c10::hip::HIPGuard guard(kept.device().index());
        Tensor out = torch::empty_like(kept);
        if (nnpops_scale_by_scalar(current_stream(kept.device()), kept.data_ptr<float>(), kept.numel(), g.data_ptr(),
                                   g.scalar_type() == torch::kFloat64 ? 1 : 0, out.data_ptr<float>()) != NNPOPS_OK)
            raise_last("NNPOpsANISymmetryFunctions::energy (backward)");
        if (ctx->saved_data["lead"].toBool()) out = out.unsqueeze(0);
        Tensor cell_out;
        if (saved.size() > 1) {                                              // dE/dcell, [3, 3] float32
            cell_out = torch::empty_like(saved[1]);
            if (nnpops_scale_by_scalar(current_stream(kept.device()), saved[1].data_ptr<float>(), saved[1].numel(), g.data_ptr(),
                                       g.scalar_type() == torch::kFloat64 ? 1 : 0, cell_out.data_ptr<float>()) != NNPOPS_OK)
                raise_last("NNPOpsANISymmetryFunctions::energy (backward)");
        }
        return {Tensor(), out, cell_out, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
                Tensor()};
    }
};

Tensor energy(const c10::optional<HolderPtr>& holder, const Tensor& positions, const c10::optional<Tensor>& cell, const Tensor& rows,
              std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members, const Tensor& planes, const Tensor& floats,
              const c10::optional<Tensor>& shift, const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks,
              int64_t act_scale_log2) {
    const bool need_cell = torch::GradMode::is_enabled() && cell.has_value() && cell->requires_grad();
    const bool need = (torch::GradMode::is_enabled() && positions.requires_grad()) || need_cell;
    return EnergyFunction::apply(*holder, positions, cell, rows, kind_atoms, widths, members, planes, floats, shift, x_blocks, dead_blocks, need,
                                 act_scale_log2, need_cell);
}

// Additive: energy AND forces (-dE/dpositions) of the frame from one call, outside autograd -- what an MD driver asks a model for
// when it takes the forces as an output instead of differentiating the energy (the step is the one of energy() with a gradient:
// the same launches; no autograd node, no sum / ones / scale kernels around it).
std::tuple<Tensor, Tensor> energy_forces(const c10::optional<HolderPtr>& holder, const Tensor& positions, const c10::optional<Tensor>& cell,
                                         const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                                         const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& shift,
                                         const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks,
                                         int64_t act_scale_log2) {
    torch::NoGradGuard no_grad;
    Tensor energy, forces;
    std::tie(energy, forces) = energy_step(*holder, positions.detach(), cell, rows, kind_atoms, widths, members, planes, floats, shift, x_blocks,
                                           dead_blocks, true, -1.0f, act_scale_log2);
    if (positions.dim() == 3) forces = forces.unsqueeze(0);
    return std::make_tuple(energy, forces);
}

// ---------------------------------------------------------------------------------------------
// Additive: the same step for a BATCH of molecules -- B conformers behind one holder with molecule offsets (Holder.set_molecules).
// positions [B, N, 3] -> energies [B]: one AEV launch sequence and one launch of the networks over all B * N atoms, one mean per
// molecule (nnpops_mlp_energy_mean_segments), dE_b/dpositions of every molecule kept from the forward [B * N, 3]; the backward scales
// each molecule's rows by its own upstream gradient (nnpops_scale_by_segment) and hands them back as [B, N, 3].
// A PERIODIC batch -- B frames, each in a box of its own -- passes cell [B, 3, 3] (the holder then was first used with such a cell:
// Holder::forwardImpl).  When the cell requires a gradient the step keeps dE_b/dcell_b [B, 3, 3] next to the position gradient, and
// the backward scales frame b's nine entries by frame b's upstream gradient: the same nnpops_scale_by_segment over the [3 B, 3] view
// with offsets 0, 3, 6, ...  A 2-D cell is what a single frame takes and stays refused.
// ---------------------------------------------------------------------------------------------
BatchTables batch_tables(const HolderPtr& holder, const Tensor& positions, const c10::optional<Tensor>& cell, const Tensor& rows,
                         const Tensor& molecule_offsets, const Tensor& row_positions) {
    TORCH_CHECK(!cell.has_value() || cell->dim() == 3, "energy_batch(): batches of molecules are non-periodic: a cell is not supported "
                "(a periodic batch takes one box per molecule, cell [molecules, 3, 3])");
    TORCH_CHECK(positions.dim() == 3 && positions.size(2) == 3 && positions.size(0) >= 1, "energy_batch(): positions must be [molecules, atoms, 3]");
    TORCH_CHECK(!cell.has_value() || (cell->size(0) == positions.size(0) && cell->size(1) == 3 && cell->size(2) == 3),
                "energy_batch(): the cell of a periodic batch must be [", positions.size(0), ", 3, 3], one box per molecule");
    require_device_tensor(positions, "positions");
    const int64_t B = positions.size(0), atoms = B * positions.size(1);
    TORCH_CHECK(holder->moleculeCount() > 0, "energy_batch(): the holder has no molecule offsets (Holder.set_molecules): it evaluates one molecule");
    TORCH_CHECK(holder->moleculeCount() == B && holder->atomCount() == atoms, "energy_batch(): positions hold ", B, " molecules of ", positions.size(1),
                " atoms, the holder ", holder->moleculeCount(), " molecules and ", holder->atomCount(), " atoms");
    for (const Tensor* t : {&molecule_offsets, &row_positions})
        TORCH_CHECK(t->scalar_type() == torch::kInt32 && t->is_contiguous() && t->device() == positions.device() && t->dim() == 1,
                    "energy_batch(): molecule_offsets and row_positions must be contiguous int32 vectors on the device of the positions");
    TORCH_CHECK(molecule_offsets.numel() == B + 1, "energy_batch(): ", B, " molecules need ", B + 1, " molecule offsets (got ", molecule_offsets.numel(), ")");
    TORCH_CHECK(row_positions.numel() == atoms && rows.numel() == atoms && rows.scalar_type() == torch::kInt32 && rows.device() == positions.device(),
                "energy_batch(): rows and row_positions must hold one int32 entry for each of the ", atoms, " atoms");
    holder->verifyBatchTables(molecule_offsets, row_positions, rows, stream_is_capturing(current_stream(positions.device())));
    return BatchTables{molecule_offsets, row_positions, B};
}

class EnergyBatchFunction : public torch::autograd::Function<EnergyBatchFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const HolderPtr& holder, const Tensor& positions, const c10::optional<Tensor>& cell, const Tensor& rows,
                          std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members, const Tensor& planes, const Tensor& floats,
                          const c10::optional<Tensor>& shift, const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks,
                          const Tensor& molecule_offsets, const Tensor& row_positions, bool need_gradient, int64_t act_scale_log2, bool need_cell) {
        const BatchTables batch = batch_tables(holder, positions, cell, rows, molecule_offsets, row_positions);
        Tensor energy, kept, kept_cell;
        std::tie(energy, kept) = energy_step(holder, positions, cell, rows, kind_atoms, widths, members, planes, floats, shift, x_blocks,
                                             dead_blocks, need_gradient, 1.0f, act_scale_log2, need_cell ? &kept_cell : nullptr, &batch);
        if (need_gradient) {
            if (need_cell) {      // dE_b/dcell_b [B, 3, 3] next to the position gradient, and the offsets 0, 3, 6, ... of its [3 B, 3] view
                const Tensor cell_offsets = torch::arange(0, 3 * batch.molecules + 1, 3, molecule_offsets.options());
                ctx->save_for_backward({kept, molecule_offsets, kept_cell, cell_offsets});
            } else {
                ctx->save_for_backward({kept, molecule_offsets});
            }
            ctx->saved_data["shape"] = positions.sizes().vec();
        }
        return energy;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        TORCH_CHECK(!torch::GradMode::is_enabled(),
                    "NNPOpsANISymmetryFunctions::energy_batch: second derivatives are not implemented (backward was called with create_graph=True); "
                    "use the four-module composition for that");
        const auto saved = ctx->get_saved_variables();
        TORCH_CHECK(!saved.empty(), "energy_batch() was evaluated without a gradient request");
        const Tensor& kept = saved[0];                                       // dE_b/dpositions of every molecule, [B * N, 3] float32
        const Tensor& offsets = saved[1];
        const Tensor g = grads[0].contiguous();
        TORCH_CHECK(g.numel() == offsets.numel() - 1 && g.device() == kept.device() &&
                    (g.scalar_type() == torch::kFloat32 || g.scalar_type() == torch::kFloat64), "energy_batch(): unexpected gradient of the energies");
        c10::hip::HIPGuard guard(kept.device().index());
        Tensor out = torch::empty_like(kept);
        if (nnpops_scale_by_segment(current_stream(kept.device()), kept.data_ptr<float>(), (int)kept.size(0), offsets.data_ptr<int32_t>(), (int)g.numel(),
                                    g.data_ptr(), g.scalar_type() == torch::kFloat64 ? 1 : 0, out.data_ptr<float>()) != NNPOPS_OK)
            raise_last("NNPOpsANISymmetryFunctions::energy_batch (backward)");
        out = out.view(ctx->saved_data["shape"].toIntVector());
        Tensor cell_out;
        if (saved.size() > 2) {                                              // frame b's nine entries by frame b's upstream gradient
            cell_out = torch::empty_like(saved[2]);
            if (nnpops_scale_by_segment(current_stream(kept.device()), saved[2].data_ptr<float>(), (int)(3 * g.numel()), saved[3].data_ptr<int32_t>(),
                                        (int)g.numel(), g.data_ptr(), g.scalar_type() == torch::kFloat64 ? 1 : 0, cell_out.data_ptr<float>()) != NNPOPS_OK)
                raise_last("NNPOpsANISymmetryFunctions::energy_batch (backward)");
        }
        return {Tensor(), out, cell_out, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
                Tensor(), Tensor(), Tensor()};
    }
};

Tensor energy_batch(const c10::optional<HolderPtr>& holder, const Tensor& positions, const c10::optional<Tensor>& cell, const Tensor& rows,
                    std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members, const Tensor& planes, const Tensor& floats,
                    const Tensor& molecule_offsets, const Tensor& row_positions, const c10::optional<Tensor>& shift,
                    const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2) {
    const bool need_cell = torch::GradMode::is_enabled() && cell.has_value() && cell->requires_grad();
    const bool need = (torch::GradMode::is_enabled() && positions.requires_grad()) || need_cell;
    return EnergyBatchFunction::apply(*holder, positions, cell, rows, kind_atoms, widths, members, planes, floats, shift, x_blocks, dead_blocks,
                                      molecule_offsets, row_positions, need, act_scale_log2, need_cell);
}

// energies [B] AND forces [B, N, 3] of the batch from one call, outside autograd (cf. energy_forces)
std::tuple<Tensor, Tensor> energy_forces_batch(const c10::optional<HolderPtr>& holder, const Tensor& positions, const c10::optional<Tensor>& cell,
                                               const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                                               const Tensor& planes, const Tensor& floats, const Tensor& molecule_offsets, const Tensor& row_positions,
                                               const c10::optional<Tensor>& shift, const c10::optional<Tensor>& x_blocks,
                                               const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2) {
    torch::NoGradGuard no_grad;
    const BatchTables batch = batch_tables(*holder, positions, cell, rows, molecule_offsets, row_positions);
    Tensor energy, forces;
    std::tie(energy, forces) = energy_step(*holder, positions.detach(), cell, rows, kind_atoms, widths, members, planes, floats, shift, x_blocks,
                                           dead_blocks, true, -1.0f, act_scale_log2, nullptr, &batch);
    return std::make_tuple(energy, forces.view(positions.sizes()));
}

TORCH_LIBRARY(NNPOpsANISymmetryFunctions, m) {
    m.class_<Holder>("Holder")
        .def(torch::init<int64_t, double, double, const std::vector<double>&, const std::vector<double>&,
                         const std::vector<double>&, const std::vector<double>&, const std::vector<double>&,
                         const std::vector<double>&, const std::vector<int64_t>&>())
        .def("forward", &Holder::forward)
        .def("backward", &Holder::backward)
        .def("tangent", &Holder::tangent)
        .def("tangent_split", &Holder::tangentSplit)
        .def("build_count", &Holder::getBuildCount)
        .def("set_check_interval", &Holder::setCheckInterval)
        .def("overflow_flag", &Holder::overflowFlag)
        .def("set_molecules", &Holder::setMolecules)
        .def("reset_gradient_cache", &Holder::resetGradientCache)
        .def_pickle([](const HolderPtr& self) -> std::string { return Holder::serialize(self); },
                    [](const std::string& state) -> HolderPtr { return Holder::deserialize(state); });
    m.def("operation", operation);
    m.def("aev", aev);
    m.def("energy(__torch__.torch.classes.NNPOpsANISymmetryFunctions.Holder? holder, Tensor positions, Tensor? cell, Tensor rows, int[] kind_atoms, "
          "int[] widths, int members, Tensor planes, Tensor floats, Tensor? shift=None, Tensor? x_blocks=None, Tensor? dead_blocks=None, int act_scale_log2=4) -> Tensor", energy);
    m.def("energy_forces(__torch__.torch.classes.NNPOpsANISymmetryFunctions.Holder? holder, Tensor positions, Tensor? cell, Tensor rows, int[] kind_atoms, "
          "int[] widths, int members, Tensor planes, Tensor floats, Tensor? shift=None, Tensor? x_blocks=None, Tensor? dead_blocks=None, int act_scale_log2=4) -> (Tensor, Tensor)",
          energy_forces);
    m.def("energy_batch(__torch__.torch.classes.NNPOpsANISymmetryFunctions.Holder? holder, Tensor positions, Tensor? cell, Tensor rows, int[] kind_atoms, "
          "int[] widths, int members, Tensor planes, Tensor floats, Tensor molecule_offsets, Tensor row_positions, Tensor? shift=None, "
          "Tensor? x_blocks=None, Tensor? dead_blocks=None, int act_scale_log2=4) -> Tensor", energy_batch);
    m.def("energy_forces_batch(__torch__.torch.classes.NNPOpsANISymmetryFunctions.Holder? holder, Tensor positions, Tensor? cell, Tensor rows, "
          "int[] kind_atoms, int[] widths, int members, Tensor planes, Tensor floats, Tensor molecule_offsets, Tensor row_positions, "
          "Tensor? shift=None, Tensor? x_blocks=None, Tensor? dead_blocks=None, int act_scale_log2=4) -> (Tensor, Tensor)", energy_forces_batch);
}

}  // namespace ANISymmetryFunctions

// =============================================================================================
// CFConv neighbours
// =============================================================================================
namespace CFConvNeighbors {

class Holder : public torch::CustomClassHolder {
public:
    explicit Holder(double cutoff) : cutoff(cutoff) {}
    ~Holder() override {
        if (impl) nnpops_cfconv_neighbors_destroy(impl);
    }

    void build(const Tensor& positions) { buildImpl(positions, nullptr); }

    // Additive to the reference (whose binding is non-periodic, CFConvNeighbors.cpp:52,57,74, although its core
    // supports a box, CFConv.h:57): the same list under periodic boundary conditions.  box: (3, 3), rows = vectors; on a holder
    // with frames (set_frames) [B, 3, 3], a box for every frame.
    void buildPeriodic(const Tensor& positions, const Tensor& box) {
        if (!molecules.empty())
            throw std::runtime_error("CFConvNeighbors::build: a list of batched molecules (set_molecules) is non-periodic and takes no \"box\"");
        if (box.scalar_type() != torch::kFloat32) throw std::runtime_error("The type of \"box\" has to be float32");
        checkBoxShape(box);
        require_device_tensor(box, "box");
        const Tensor b = box.detach().contiguous();
        buildImpl(positions, &b);
    }

    void buildImpl(const Tensor& positions, const Tensor* box) {
        if (positions.scalar_type() != torch::kFloat32) throw std::runtime_error("The type of \"positions\" has to be float32");
        if (positions.dim() != 2) throw std::runtime_error("The shape of \"positions\" has to have 2 dimensions");
        if (positions.size(1) != 3) throw std::runtime_error("The size of the 2nd dimension of \"positions\" has to be 3");
        require_device_tensor(positions, "positions");
        if (!impl) {
            numAtoms = positions.size(0);
            device = positions.device();
            periodic = box != nullptr;
            if (nnpops_cfconv_neighbors_create(&impl, (int)numAtoms, (float)cutoff, periodic ? 1 : 0, device.index()) != NNPOPS_OK)
                raise_last("NNPOpsCFConvNeighbors");
            if (!molecules.empty() || !frames.empty()) {
                try {
                    if (!molecules.empty()) applyMolecules();
                    if (!frames.empty()) applyFrames();
                } catch (...) {                                   // (offsets that do not fit these positions: no half-made handle stays behind)
                    nnpops_cfconv_neighbors_destroy(impl);
                    impl = nullptr;
                    throw;
                }
            }
        }
        if (positions.size(0) != numAtoms) throw std::runtime_error("The size of the 2nd dimension of \"positions\" has changed");
        if (positions.device() != device) throw std::runtime_error("The device of \"positions\" has changed");
        if (periodic != (box != nullptr)) throw std::runtime_error("The periodicity of \"neighbors\" has changed");
        if (box && box->device() != device) throw std::runtime_error("The device of \"box\" has changed");
        const Tensor pos = positions.detach().contiguous();
        void* stream = current_stream(device);
        nnpops_cfconv_neighbors_set_stream(impl, stream);
        const bool capturing = stream_is_capturing(stream);
        for (int attempt = 0;; attempt++) {
            if (nnpops_cfconv_neighbors_build(impl, pos.data_ptr<float>(), box ? box->data_ptr<float>() : nullptr) != NNPOPS_OK)
                raise_last("CFConvNeighbors::build");
            if (capturing) break;
            const int rc = nnpops_cfconv_neighbors_check(impl, nullptr);
            if (rc == NNPOPS_OK) break;
            if (rc != NNPOPS_ERR_CAPACITY || attempt > 8) raise_last("CFConvNeighbors::build");
        }
    }
    // Additive: the atoms are a batch of independent non-periodic molecules, atoms [offsets[m], offsets[m+1]) molecule m
    // (nnpops_cfconv_neighbors_set_molecules).  Kept here and applied when the handle is created (the first build) and on later calls;
    // an empty list restores the single-system behaviour.  The current build is invalidated.
    void setMolecules(std::vector<int64_t> offsets) {
        for (int64_t v : offsets)
            if (v < 0 || v > INT32_MAX) throw std::runtime_error("set_molecules: molecule offsets must lie in [0, num_atoms]");
        if (!offsets.empty() && offsets.size() < 2) throw std::runtime_error("set_molecules: molecule offsets hold B + 1 entries (or none: one system)");
        if (!offsets.empty() && !frames.empty())
            throw std::runtime_error("set_molecules: this list holds periodic frames (set_frames); batched molecules are non-periodic systems");
        if (!offsets.empty() && impl && periodic) throw std::runtime_error("set_molecules: batched molecules are non-periodic systems (this list was built with a box)");
        const std::vector<int64_t> before = molecules;
        molecules = std::move(offsets);
        if (!impl) return;
        try {
            applyMolecules();
        } catch (...) {
            molecules = before;                                   // (the handle kept its table: a refused call changes nothing)
            throw;
        }
    }
    std::vector<int64_t> getMolecules() const { return molecules; }
    int64_t moleculeCount() const { return molecules.empty() ? 0 : (int64_t)molecules.size() - 1; }
    // Additive: the atoms are a batch of PERIODIC frames, atoms [offsets[m], offsets[m+1]) frame m, every frame in its own box
    // (nnpops_cfconv_neighbors_set_frames): build_periodic and the periodic ops then take box [B, 3, 3].  Kept and applied like the
    // molecules; an empty list restores the single-system behaviour.  The current build is invalidated.
    void setFrames(std::vector<int64_t> offsets) {
        for (int64_t v : offsets)
            if (v < 0 || v > INT32_MAX) throw std::runtime_error("set_frames: frame offsets must lie in [0, num_atoms]");
        if (!offsets.empty() && offsets.size() < 2) throw std::runtime_error("set_frames: frame offsets hold B + 1 entries (or none: one system)");
        if (!offsets.empty() && !molecules.empty())
            throw std::runtime_error("set_frames: this list holds batched molecules (set_molecules), which are non-periodic; frames are periodic systems");
        if (!offsets.empty() && impl && !periodic)
            throw std::runtime_error("set_frames: frames are periodic systems, each in its own box (this list was built without a box)");
        const std::vector<int64_t> before = frames;
        frames = std::move(offsets);
        if (!impl) return;
        try {
            applyFrames();
        } catch (...) {
            frames = before;                                      // (the handle kept its tables: a refused call changes nothing)
            throw;
        }
    }
    std::vector<int64_t> getFrames() const { return frames; }
    int64_t frameCount() const { return frames.empty() ? 0 : (int64_t)frames.size() - 1; }
    // the box of a build or of a periodic op: (3, 3), or [B, 3, 3] on a holder with B frames
    void checkBoxShape(const Tensor& box) const {
        if (frames.empty()) {
            if (box.dim() != 2 || box.size(0) != 3 || box.size(1) != 3) throw std::runtime_error("The shape of \"box\" has to be (3, 3)");
        } else if (box.dim() != 3 || box.size(0) != frameCount() || box.size(1) != 3 || box.size(2) != 3) {
            throw std::runtime_error("The shape of \"box\" has to be [" + std::to_string(frameCount()) +
                                     ", 3, 3]: this list holds periodic frames (set_frames), one box for each");
        }
    }
    double getCutoff() const { return cutoff; }
    bool isPeriodic() const { return periodic; }
    nnpops_cfconv_neighbors_t getImpl() const { return impl; }
    // the number of the last build (0: never built): the twice-differentiable ops record it and refuse to differentiate on a later one
    int64_t getBuildCount() const {
        unsigned long long count = 0;
        if (impl && nnpops_cfconv_neighbors_build_count(impl, &count) != NNPOPS_OK) raise_last("NNPOpsCFConvNeighbors");
        return (int64_t)count;
    }

private:
    void applyMolecules() {
        const std::vector<int32_t> off(molecules.begin(), molecules.end());
        nnpops_cfconv_neighbors_set_stream(impl, current_stream(device));
        if (nnpops_cfconv_neighbors_set_molecules(impl, off.empty() ? 0 : (int)off.size() - 1, off.empty() ? nullptr : off.data()) != NNPOPS_OK)
            raise_last("NNPOpsCFConvNeighbors::set_molecules");
    }

    void applyFrames() {
        const std::vector<int32_t> off(frames.begin(), frames.end());
        nnpops_cfconv_neighbors_set_stream(impl, current_stream(device));
        if (nnpops_cfconv_neighbors_set_frames(impl, off.empty() ? 0 : (int)off.size() - 1, off.empty() ? nullptr : off.data()) != NNPOPS_OK)
            raise_last("NNPOpsCFConvNeighbors::set_frames");
    }

    double cutoff;
    int64_t numAtoms = 0;
    bool periodic = false;
    torch::Device device = torch::kCPU;
    nnpops_cfconv_neighbors_t impl = nullptr;
    std::vector<int64_t> molecules;      // B + 1 offsets; empty: one system
    std::vector<int64_t> frames;         // B + 1 offsets of periodic frames; empty: one system
};
using HolderPtr = torch::intrusive_ptr<Holder>;

TORCH_LIBRARY(NNPOpsCFConvNeighbors, m) {
    m.class_<Holder>("Holder")
        .def(torch::init<double>())
        .def("build", &Holder::build)
        .def("build_periodic", &Holder::buildPeriodic)
        .def("build_count", &Holder::getBuildCount)
        .def("set_molecules", &Holder::setMolecules)
        .def("molecules", &Holder::getMolecules)
        .def("set_frames", &Holder::setFrames)
        .def("frames", &Holder::getFrames)
        .def_pickle([](const HolderPtr& self) -> double { return self->getCutoff(); },
                    [](double cutoff) -> HolderPtr { return HolderPtr::make(cutoff); });
}

}  // namespace CFConvNeighbors

// =============================================================================================
// CFConv
// =============================================================================================
namespace CFConv {

using Neighbors = NNPOps::CFConvNeighbors::Holder;
using NeighborsPtr = torch::intrusive_ptr<Neighbors>;
class Holder;
using HolderPtr = torch::intrusive_ptr<Holder>;

class Holder : public torch::CustomClassHolder {
public:
    Holder(double gaussianWidth, const std::string& activation, const Tensor& weights1, const Tensor& biases1,
           const Tensor& weights2, const Tensor& biases2)
        : gaussianWidth(gaussianWidth), activation(activation),
          // host copies, as in the reference (CFConv.cpp:63-66)
          weights1(weights1.to(torch::kFloat32).cpu().clone()), biases1(biases1.to(torch::kFloat32).cpu().clone()),
          weights2(weights2.to(torch::kFloat32).cpu().clone()), biases2(biases2.to(torch::kFloat32).cpu().clone()) {}

    ~Holder() override {
        if (impl) nnpops_cfconv_destroy(impl);
    }

    Tensor forward(const c10::IValue& neighbors_, const Tensor& positions_, const Tensor& input_) {
        neighbors = neighbors_.toCustomClass<Neighbors>();      // kept, with positions and input, for the scripted backward() alone
        if (positions_.scalar_type() != torch::kFloat32) throw std::runtime_error("The type of \"positions\" has to be float32");
        if (positions_.dim() != 2) throw std::runtime_error("The shape of \"positions\" has to have 2 dimensions");
        if (positions_.size(1) != 3) throw std::runtime_error("The size of the 2nd dimension of \"positions\" has to be 3");
        if (input_.device() != positions_.device()) throw std::runtime_error("The device of \"input\" and \"positions\" has to be the same");
        if (input_.scalar_type() != torch::kFloat32) throw std::runtime_error("The type of \"input\" has to be float32");
        if (input_.dim() != 2) throw std::runtime_error("The shape of \"input\" has to have 2 dimensions");
        if (input_.size(0) != positions_.size(0))
            throw std::runtime_error("The size of the 1nd dimension of \"input\" has to be equal to the 1st dimension of \"positions\"");
        require_device_tensor(positions_, "positions");
        positions = positions_.detach().contiguous();
        input = input_.detach().contiguous();
        if (!impl) {
            device = positions.device();
            numAtoms = positions.size(0);
            numFilters = input.size(1);
            cutoff = neighbors->getCutoff();
            int act;
            if (activation == "ssp") act = 0;
            else if (activation == "tanh") act = 1;
            else throw std::invalid_argument("Invalid value of \"activation\"");
            // shape checks and messages of the reference (CFConv.cpp:106-127)
            if (weights1.dim() != 2) throw std::runtime_error("The shape of \"weights1\" has to have 2 dimensions");
            const int64_t numGaussians = weights1.size(0);
            if (weights1.size(1) != numFilters)
                throw std::runtime_error("The size of the 2nd dimension of \"weights1\" has to be equal to the 2st dimension of \"input\"");
            if (biases1.dim() != 1) throw std::runtime_error("The shape of \"biases1\" has to have 1 dimension");
            if (biases1.size(0) != numFilters) throw std::runtime_error("The size of \"biases1\" has to be equal to the 2st dimension of \"input\"");
            if (weights2.dim() != 2) throw std::runtime_error("The shape of \"weights2\" has to have 2 dimensions");
            if (weights2.size(0) != numFilters)
                throw std::runtime_error("The size of the 1nd dimension of \"weights2\" has to be equal to the 2st dimension of \"input\"");
            if (weights2.size(1) != numFilters)
                throw std::runtime_error("The size of the 2nd dimension of \"weights2\" has to be equal to the 2st dimension of \"input\"");
            if (biases2.dim() != 1) throw std::runtime_error("The shape of \"biases2\" has to have 1 dimension");
            if (biases2.size(0) != numFilters) throw std::runtime_error("The size of \"biases2\" has to be equal to the 2st dimension of \"input\"");
            // Layout note: the reference hands the contiguous [G, W] buffer of weights1 to a core that indexes it
            // as [W][G] (CFConv.cpp:131-132 -> CpuCFConv.cpp:163), i.e. a reinterpretation, not a transpose.  The
            // C ABI takes the core layout, so the same buffer is passed through unchanged.
            const Tensor w1 = weights1.contiguous(), w2 = weights2.contiguous();
            if (nnpops_cfconv_create(&impl, (int)numAtoms, (int)numFilters, (int)numGaussians, (float)cutoff, 0, (float)gaussianWidth,
                                     act, w1.data_ptr<float>(), biases1.data_ptr<float>(), w2.data_ptr<float>(),
                                     biases2.data_ptr<float>(), device.index()) != NNPOPS_OK)
                raise_last("NNPOpsCFConv");
        }
        if (neighbors->getCutoff() != cutoff) throw std::runtime_error("The cutoff of \"neighbors\" has changed");
        if (positions.size(0) != numAtoms) throw std::runtime_error("The size of the 1nd dimension of \"positions\" has changed");
        if (positions.device() != device) throw std::runtime_error("The device of \"positions\" has changed");
        if (input.size(0) != numAtoms) throw std::runtime_error("The size of the 1nd dimension of \"input\" has changed");
        if (input.size(1) != numFilters) throw std::runtime_error("The size of the 2nd dimension of \"input\" has changed");
        if (input.device() != device) throw std::runtime_error("The device of \"input\" has changed");
        if (!neighbors->getImpl()) throw std::runtime_error("\"neighbors\" has not been built");

        Tensor output = torch::empty({numAtoms, numFilters}, torch::TensorOptions().device(device).dtype(torch::kFloat32));
        nnpops_cfconv_set_stream(impl, current_stream(device));
        if (nnpops_cfconv_compute(impl, neighbors->getImpl(), positions.data_ptr<float>(), nullptr, input.data_ptr<float>(),
                                  output.data_ptr<float>()) != NNPOPS_OK)
            raise_last("NNPOpsCFConv::forward");
        return output;
    }

    // Additive (operation_periodic): the same forward, to the bit, on a list built with box vectors.  The box is checked here and kept by
    // the node that asked, for a backward pass that returns dL/dbox (the box vectors must be those of the list's last build).
    Tensor forwardPeriodic(const c10::IValue& neighbors_, const Tensor& positions_, const Tensor& box_, const Tensor& input_) {
        if (box_.scalar_type() != torch::kFloat32) throw std::runtime_error("The type of \"box\" has to be float32");
        const NeighborsPtr nb = neighbors_.toCustomClass<Neighbors>();
        nb->checkBoxShape(box_);                             // (3, 3), or [B, 3, 3] on a list of B frames
        require_device_tensor(box_, "box");
        if (box_.device() != positions_.device()) throw std::runtime_error("The device of \"box\" and \"positions\" has to be the same");
        if (nb->moleculeCount() > 0)
            throw std::runtime_error("\"neighbors\" holds batched molecules (set_molecules), which are non-periodic: the convolution takes no \"box\" with them");
        if (!nb->getImpl()) throw std::runtime_error("\"neighbors\" has not been built");
        if (!nb->isPeriodic()) throw std::runtime_error("\"neighbors\" has been built without a box: a \"box\" needs a periodic neighbour list");
        return forward(neighbors_, positions_, input_);
    }

    // The scripted backward() of the reference's surface: the gradients of the last direct forward() call, {holder, neighbours, positions,
    // input} (nothing for the first two, :189).  It is the only reader of the slot; the autograd nodes below keep the tensors of their own
    // forward pass in their own contexts and hand them to the four routines that follow.
    tensor_list backward(const tensor_list& grads) {
        if (!impl) throw std::runtime_error("backward() called before forward()");
        const tensor_list d = backwardOf(neighbors, positions, Tensor(), input, grads[0], false);
        return {Tensor(), Tensor(), d[1], d[0]};
    }

    // {inputGrad, positionsGrad, boxGrad} of one forward pass on the tensors the caller hands over: nnpops_cfconv_backprop, or, when the
    // box wants its gradient, nnpops_cfconv_backprop_box (the same launches and dL/dbox behind them); boxGrad is undefined otherwise
    tensor_list backwardOf(const NeighborsPtr& nb, const Tensor& positions_, const Tensor& box_ /* undefined: none */, const Tensor& input_,
                           const Tensor& outputGrad_, bool wantBox) {
        const auto opts = gradOptions();
        const Tensor pos = dense(positions_), in = dense(input_), outputGrad = dense(outputGrad_);
        Tensor inputGrad = torch::empty({numAtoms, numFilters}, opts), positionsGrad = torch::empty({numAtoms, 3}, opts), boxGrad;
        if (wantBox) {
            if (!box_.defined()) throw std::runtime_error("a box gradient needs the box vectors of the forward pass");
            const Tensor box = dense(box_);
            nb->checkBoxShape(box);
            boxGrad = torch::empty(box.sizes(), opts);        // (3, 3), or [B, 3, 3] on a list of B frames
            launch("NNPOpsCFConv::backward", [&] {
                return nnpops_cfconv_backprop_box(impl, nb->getImpl(), pos.data_ptr<float>(), box.data_ptr<float>(), in.data_ptr<float>(),
                                                  outputGrad.data_ptr<float>(), inputGrad.data_ptr<float>(), positionsGrad.data_ptr<float>(),
                                                  boxGrad.data_ptr<float>());
            });
        } else {
            launch("NNPOpsCFConv::backward", [&] {
                return nnpops_cfconv_backprop(impl, nb->getImpl(), pos.data_ptr<float>(), nullptr, in.data_ptr<float>(),
                                              outputGrad.data_ptr<float>(), inputGrad.data_ptr<float>(), positionsGrad.data_ptr<float>());
            });
        }
        return {inputGrad, positionsGrad, boxGrad};
    }

    // dL/d(weights1, biases1, weights2, biases2) of the same pass (nnpops_cfconv_backprop_weights).  weights1 keeps the module's
    // convention: the core's [W][G] result is the [G, W] tensor's buffer, reinterpreted and not transposed.
    tensor_list backwardWeightsOf(const NeighborsPtr& nb, const Tensor& input_, const Tensor& outputGrad_) {
        const tensor_list w = weightGrads(gradOptions());
        const Tensor in = dense(input_), outputGrad = dense(outputGrad_);
        launch("NNPOpsCFConv::backward (weights)", [&] {
            return nnpops_cfconv_backprop_weights(impl, nb->getImpl(), in.data_ptr<float>(), outputGrad.data_ptr<float>(), w[0].data_ptr<float>(),
                                                  w[1].data_ptr<float>(), w[2].data_ptr<float>(), w[3].data_ptr<float>());
        });
        return w;
    }

    // The backward of backwardOf() (nnpops_cfconv_double_backward): cotangents of its two gradients (either may be undefined = zero) to
    // the gradients with respect to {outputGrad, input, positions} ...
    tensor_list doubleBackward(const NeighborsPtr& nb, const Tensor& positions_, const Tensor& input_, const Tensor& outputGrad_,
                               const Tensor& ggInput_, const Tensor& ggPositions_) {
        const auto opts = gradOptions();
        const Tensor pos = dense(positions_), in = dense(input_), outputGrad = dense(outputGrad_);
        const Tensor ggInput = cotangent(ggInput_), ggPositions = cotangent(ggPositions_);
        Tensor dOutputGrad = torch::empty({numAtoms, numFilters}, opts), dInput = torch::empty({numAtoms, numFilters}, opts);
        Tensor dPositions = torch::empty({numAtoms, 3}, opts);
        launch("NNPOpsCFConv::double backward", [&] {
            return nnpops_cfconv_double_backward(impl, nb->getImpl(), pos.data_ptr<float>(), in.data_ptr<float>(), outputGrad.data_ptr<float>(),
                                                 data_or_null(ggInput), data_or_null(ggPositions), dOutputGrad.data_ptr<float>(),
                                                 dInput.data_ptr<float>(), dPositions.data_ptr<float>());
        });
        return {dOutputGrad, dInput, dPositions};
    }

    // ... and the weight gradients of what doubleBackward() differentiates (nnpops_cfconv_double_backward_weights), weights1 in the
    // module's convention as above
    tensor_list doubleBackwardWeights(const NeighborsPtr& nb, const Tensor& input_, const Tensor& outputGrad_, const Tensor& ggInput_,
                                      const Tensor& ggPositions_) {
        const tensor_list w = weightGrads(gradOptions());
        const Tensor in = dense(input_), outputGrad = dense(outputGrad_);
        const Tensor ggInput = cotangent(ggInput_), ggPositions = cotangent(ggPositions_);
        launch("NNPOpsCFConv::double backward (weights)", [&] {
            return nnpops_cfconv_double_backward_weights(impl, nb->getImpl(), in.data_ptr<float>(), outputGrad.data_ptr<float>(),
                                                         data_or_null(ggInput), data_or_null(ggPositions), w[0].data_ptr<float>(),
                                                         w[1].data_ptr<float>(), w[2].data_ptr<float>(), w[3].data_ptr<float>());
        });
        return w;
    }

    // Trainable filters (operation_weights / operation_periodic_weights): bring the handle up to date with four weight tensors the
    // caller owns.  What was last uploaded is remembered by storage and version counter, so a forward pass with unchanged parameters
    // copies nothing; after an optimizer step (an in-place update: a new version) the host copies are replaced and a live handle is
    // given them through nnpops_cfconv_set_weights, which plans again.  Shapes are those the holder was constructed with.
    void syncWeights(const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2) {
        const Tensor* given[4] = {&w1, &b1, &w2, &b2};
        const Tensor* kept[4] = {&weights1, &biases1, &weights2, &biases2};
        static const char* const names[4] = {"weights1", "biases1", "weights2", "biases2"};
        bool same = uploads > 0;
        for (int k = 0; k < 4; k++) {
            const Tensor& t = *given[k];
            if (t.scalar_type() != torch::kFloat32) throw std::runtime_error(std::string("The type of \"") + names[k] + "\" has to be float32");
            if (t.sizes() != kept[k]->sizes())
                throw std::runtime_error(std::string("The shape of \"") + names[k] + "\" has changed since the convolution was constructed");
            same = same && t.is_contiguous() && t.data_ptr() == uploadedData[k] && (int64_t)t._version() == uploadedVersion[k];
        }
        if (same) return;
        weights1 = w1.detach().cpu().contiguous().clone(); biases1 = b1.detach().cpu().contiguous().clone();
        weights2 = w2.detach().cpu().contiguous().clone(); biases2 = b2.detach().cpu().contiguous().clone();
        if (impl) {
            nnpops_cfconv_set_stream(impl, current_stream(device));
            if (nnpops_cfconv_set_weights(impl, weights1.data_ptr<float>(), biases1.data_ptr<float>(), weights2.data_ptr<float>(),
                                          biases2.data_ptr<float>()) != NNPOPS_OK)
                raise_last("NNPOpsCFConv::operation_weights (set_weights)");
        }                                                    // (no handle yet: the first forward pass creates it from these copies)
        for (int k = 0; k < 4; k++) { uploadedData[k] = given[k]->data_ptr(); uploadedVersion[k] = (int64_t)given[k]->_version(); }
        uploads++;
    }

    // how many times syncWeights() has replaced the weights (a forward pass with unchanged parameters does not count)
    int64_t getUploads() const { return uploads; }

    static std::string serialize(const HolderPtr& self) {
        torch::serialize::OutputArchive archive;
        archive.write("gaussianWidth", self->gaussianWidth);
        archive.write("activation", self->activation);
        archive.write("weights1", self->weights1);
        archive.write("biases1", self->biases1);
        archive.write("weights2", self->weights2);
        archive.write("biases2", self->biases2);
        std::stringstream stream;
        archive.save_to(stream);
        return stream.str();
    }

    static HolderPtr deserialize(const std::string& state) {
        std::stringstream stream(state);
        torch::serialize::InputArchive archive;
        archive.load_from(stream, torch::kCPU);
        torch::IValue gaussianWidth, activation;
        Tensor weights1, biases1, weights2, biases2;
        archive.read("gaussianWidth", gaussianWidth);
        archive.read("activation", activation);
        archive.read("weights1", weights1);
        archive.read("biases1", biases1);
        archive.read("weights2", weights2);
        archive.read("biases2", biases2);
        return HolderPtr::make(gaussianWidth.toDouble(), activation.toStringRef(), weights1, biases1, weights2, biases2);
    }

private:
    // what the four gradient routines share: float32 outputs on the handle's device (a handle there must be) ...
    torch::TensorOptions gradOptions() const {
        if (!impl) throw std::runtime_error("backward() called before forward()");
        return torch::TensorOptions().device(device).dtype(torch::kFloat32);
    }
    tensor_list weightGrads(const torch::TensorOptions& opts) const {
        return {torch::empty(weights1.sizes(), opts), torch::empty({numFilters}, opts), torch::empty({numFilters, numFilters}, opts),
                torch::empty({numFilters}, opts)};
    }
    // ... what the core reads: a tensor as it is, an optional cotangent as float32 or as nullptr ...
    static Tensor dense(const Tensor& t) { return t.is_contiguous() ? t : t.detach().contiguous(); }
    static Tensor cotangent(const Tensor& t) { return t.defined() ? t.detach().to(torch::kFloat32).contiguous() : Tensor(); }
    static const float* data_or_null(const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
    // ... and one call of the core on the current stream
    template <typename Call>
    void launch(const char* what, Call&& call) {
        nnpops_cfconv_set_stream(impl, current_stream(device));
        if (call() != NNPOPS_OK) raise_last(what);
    }

    double gaussianWidth;
    std::string activation;
    Tensor weights1, biases1, weights2, biases2;
    torch::Device device = torch::kCPU;
    int64_t numAtoms = 0, numFilters = 0;
    double cutoff = 0;
    // the slot: the tensors of the last forward() call, read by the scripted backward() and by nothing else
    NeighborsPtr neighbors;
    Tensor positions, input;
    nnpops_cfconv_t impl = nullptr;
    // syncWeights(): what the handle (or, before the first forward pass, the host copies) last received
    const void* uploadedData[4] = {nullptr, nullptr, nullptr, nullptr};
    int64_t uploadedVersion[4] = {0, 0, 0, 0};
    int64_t uploads = 0;
};

// ---------------------------------------------------------------------------------------------
// The eight ops are adaptors onto two families of autograd nodes.  Every node keeps the tensors of its own forward pass in its own
// context, so two calls of one CFConv before the first is differentiated do not disturb each other.
//   first order (CFConvFunction): operation, operation_periodic and, with the four weight arrays as inputs that take a gradient (trainable
//     filters), operation_weights, operation_periodic_weights.  Its backward is Holder::backwardOf -- with dL/dbox where
//     the box asked for it -- and, where a weight asks, Holder::backwardWeightsOf; it is not recorded.
//   recorded (CFConvTwiceFunction -> CFConvBackwardFunction -> CFConvDoubleBackwardFunction): operation_twice, operation_periodic_twice
//      and, with the weights, operation_weights_twice, operation_periodic_weights_twice (3.7f): the same forward and
//     first backward, to the bit, recorded so that the backward pass is itself differentiable:
//       CFConvBackwardFunction         (g, positions, input, weights) -> (gx, gp, the wanted weight gradients)
//       CFConvDoubleBackwardFunction   (V, Q, g, positions, input) -> (dM/dg, dM/dx, dM/dpositions, the wanted weight gradients)
//     Refused: third derivatives, a cotangent for the first-order weight gradients (weight-weight second derivatives), a box that
//     requires a gradient (the first-order ops have it).
// With weights the forward pass first brings the handle up to date (Holder::syncWeights).  Every node but that of the two default ops
// records the number of the list's build in the forward pass, the recorded ones with weights the holder's upload count too, and raises
// on another: the rows it would walk belong to other positions, the gradient to other weights.
// ---------------------------------------------------------------------------------------------
using MaybeTensor = c10::optional<Tensor>;

inline void check_same_state(const HolderPtr& holder, const NeighborsPtr& nb, int64_t build, int64_t uploads /* -1: not tracked */,
                             const char* op) {
    TORCH_CHECK(nb->getBuildCount() == build, "NNPOpsCFConv::", op, ": \"neighbors\" has been rebuilt since the forward pass; its rows no "
                "longer belong to the positions this gradient is taken at (build the list, run the forward pass and differentiate "
                "before building it again)");
    TORCH_CHECK(uploads < 0 || holder->getUploads() == uploads, "NNPOpsCFConv::", op, ": the weights have been uploaded again since the "
                "forward pass (an optimizer step or another forward pass with new values); this gradient would be taken at other "
                "weights than the output it belongs to (differentiate before the weights change)");
}

// the forward pass of every op: the weights, where they are inputs, reach the handle first
inline Tensor run_forward(const HolderPtr& holder, const c10::IValue& neighbors, const Tensor& positions, const MaybeTensor& box,
                          const Tensor& input, const MaybeTensor& weights1, const MaybeTensor& biases1, const MaybeTensor& weights2,
                          const MaybeTensor& biases2) {
    if (weights1) holder->syncWeights(*weights1, *biases1, *weights2, *biases2);
    return box ? holder->forwardPeriodic(neighbors, positions, *box, input) : holder->forward(neighbors, positions, input);
}

// bit k = weight k takes a gradient: what the engine asks of a node whose weights are its tensor inputs first, first + 1, ...
inline int64_t wanted_weights(AutogradContext* ctx, size_t first) {
    int64_t wants = 0;
    for (int k = 0; k < 4; k++) wants |= ctx->needs_input_grad(first + k) ? (int64_t)1 << k : 0;
    return wants;
}

// a weight gradient where its weight lives (a parameter kept on the CPU receives a CPU gradient)
inline Tensor weight_grad_for(const Tensor& grad, const Tensor& weight) { return weight.is_cpu() ? grad.cpu() : grad; }

// box: empty for the non-periodic ops; weights: empty for the default ops.  wants (decided by the caller, where grad mode is what the
// user set): bit k = weight k requires a gradient, bit 4 = the box does.
class CFConvFunction : public torch::autograd::Function<CFConvFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const HolderPtr& holder, const c10::IValue& neighbors, const Tensor& positions,
                          const MaybeTensor& box, const Tensor& input, const MaybeTensor& weights1, const MaybeTensor& biases1,
                          const MaybeTensor& weights2, const MaybeTensor& biases2, int64_t wants) {
        // (what the core reads is what the backward pass is handed: it copies nothing again)
        const Tensor pos = positions.detach().contiguous(), in = input.detach().contiguous();
        const Tensor output = run_forward(holder, neighbors, pos, box, in, weights1, biases1, weights2, biases2);
        int64_t on_cpu = 0;
        if (weights1) on_cpu = (weights1->is_cpu() ? 1 : 0) | (biases1->is_cpu() ? 2 : 0) | (weights2->is_cpu() ? 4 : 0) | (biases2->is_cpu() ? 8 : 0);
        ctx->saved_data["holder"] = holder;
        ctx->saved_data["neighbors"] = neighbors;
        ctx->saved_data["positions"] = pos;
        ctx->saved_data["input"] = in;
        if (wants & 16) ctx->saved_data["box"] = box->detach().contiguous();
        ctx->saved_data["build"] = weights1 ? neighbors.toCustomClass<Neighbors>()->getBuildCount() : (int64_t)-1;      // -1: a default op
        ctx->saved_data["wants"] = wants;
        ctx->saved_data["on_cpu"] = on_cpu;
        return output;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const int64_t build = ctx->saved_data["build"].toInt();
        TORCH_CHECK(build < 0 || !torch::GradMode::is_enabled(),
                    "NNPOpsCFConv::operation_weights: second derivatives are not implemented for the trainable convolution (create_graph=True): "
                    "mixed second derivatives with respect to the filter network's weights are missing; training on forces takes "
                    "CFConv(..., twice_differentiable=True) with fixed weights");
        const HolderPtr holder = ctx->saved_data["holder"].toCustomClass<Holder>();
        const NeighborsPtr nb = ctx->saved_data["neighbors"].toCustomClass<Neighbors>();
        if (build >= 0) check_same_state(holder, nb, build, -1, "operation_weights");
        const int64_t wants = ctx->saved_data["wants"].toInt();
        const Tensor input = ctx->saved_data["input"].toTensor();
        const Tensor box = wants & 16 ? ctx->saved_data["box"].toTensor() : Tensor();
        const tensor_list d = holder->backwardOf(nb, ctx->saved_data["positions"].toTensor(), box, input, grads[0], (wants & 16) != 0);
        tensor_list out = {Tensor(), Tensor(), d[1], d[2], d[0]};      // {holder, neighbours, positions, box, input, four weights, wants}
        out.resize(10);
        if (wants & 15) {
            const tensor_list w = holder->backwardWeightsOf(nb, input, grads[0]);
            const int64_t on_cpu = ctx->saved_data["on_cpu"].toInt();
            for (int k = 0; k < 4; k++)
                if (wants >> k & 1) out[5 + k] = on_cpu >> k & 1 ? w[k].cpu() : w[k];
        }
        return out;
    }
};

inline const char* twice_op(int64_t uploads) { return uploads < 0 ? "operation_twice" : "operation_weights_twice"; }

// uploads: the holder's count in the forward pass, -1 for the ops without weights.  wants: bit k = weight k takes a gradient (0 without).
class CFConvDoubleBackwardFunction : public torch::autograd::Function<CFConvDoubleBackwardFunction> {
public:
    // (a cotangent nobody asked for arrives undefined -- CFConvBackwardFunction does not materialise zeros -- and travels as nullopt)
    static tensor_list forward(AutogradContext* ctx, const MaybeTensor& ggInput, const MaybeTensor& ggPositions, const Tensor& g,
                               const Tensor& positions, const Tensor& input, const HolderPtr& holder, const c10::IValue& neighbors,
                               int64_t build, int64_t uploads, int64_t wants) {
        const NeighborsPtr nb = neighbors.toCustomClass<Neighbors>();
        check_same_state(holder, nb, build, uploads, twice_op(uploads));
        ctx->saved_data["uploads"] = uploads;
        const Tensor V = ggInput ? *ggInput : Tensor(), Q = ggPositions ? *ggPositions : Tensor();
        tensor_list out = holder->doubleBackward(nb, positions, input, g, V, Q);
        if (wants & 15) {                                    // (a recorded node has no undefined outputs: the wanted ones only, in order)
            const tensor_list w = holder->doubleBackwardWeights(nb, input, g, V, Q);
            for (int k = 0; k < 4; k++)
                if (wants >> k & 1) out.push_back(w[k]);
        }
        return out;
    }
    static tensor_list backward(AutogradContext* ctx, tensor_list) {
        TORCH_CHECK(false, "NNPOpsCFConv::", twice_op(ctx->saved_data["uploads"].toInt()), ": third derivatives are not implemented");
        return {};
    }
};

class CFConvBackwardFunction : public torch::autograd::Function<CFConvBackwardFunction> {
public:
    static tensor_list forward(AutogradContext* ctx, const Tensor& g, const Tensor& positions, const Tensor& input, const MaybeTensor& weights1,
                               const MaybeTensor& biases1, const MaybeTensor& weights2, const MaybeTensor& biases2, const HolderPtr& holder,
                               const c10::IValue& neighbors, int64_t build, int64_t uploads, int64_t wants) {
        const NeighborsPtr nb = neighbors.toCustomClass<Neighbors>();
        check_same_state(holder, nb, build, uploads, twice_op(uploads));
        ctx->set_materialize_grads(false);
        tensor_list kept = {g, positions, input};
        if (weights1) kept.insert(kept.end(), {*weights1, *biases1, *weights2, *biases2});
        ctx->save_for_backward(kept);
        ctx->saved_data["holder"] = holder;
        ctx->saved_data["neighbors"] = neighbors;
        ctx->saved_data["build"] = build;
        ctx->saved_data["uploads"] = uploads;
        tensor_list out = holder->backwardOf(nb, positions, Tensor(), input, g, false);
        out.resize(2);                                       // (a recorded node has no undefined outputs: the wanted ones only, in order)
        if (wants & 15) {
            const tensor_list w = holder->backwardWeightsOf(nb, input, g);
            for (int k = 0; k < 4; k++)
                if (wants >> k & 1) out.push_back(w[k]);
        }
        return out;
    }
    static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
        for (size_t k = 2; k < grads.size(); k++)
            TORCH_CHECK(!grads[k].defined(), "NNPOpsCFConv::operation_weights_twice: second derivatives of the weight gradients themselves "
                        "(weight-weight second derivatives: a cotangent arrived for the gradient of a weight) are not implemented; the "
                        "second derivatives of this op are those of the gradients with respect to positions and input");
        tensor_list out(12);
        if (!grads[0].defined() && !grads[1].defined()) return out;
        const auto s = ctx->get_saved_variables();           // {g, positions, input} and, with them, the four weights
        const int64_t wants = s.size() > 3 ? wanted_weights(ctx, 3) : 0;
        const auto given = [](const Tensor& t) { return t.defined() ? MaybeTensor(t) : MaybeTensor(); };
        const tensor_list d = CFConvDoubleBackwardFunction::apply(given(grads[0]), given(grads[1]), s[0], s[1], s[2],
                                                                  ctx->saved_data["holder"].toCustomClass<Holder>(),
                                                                  ctx->saved_data["neighbors"], ctx->saved_data["build"].toInt(),
                                                                  ctx->saved_data["uploads"].toInt(), wants);
        out[0] = d[0]; out[1] = d[2]; out[2] = d[1];
        size_t next = 3;
        for (int k = 0; k < 4; k++)
            if (wants >> k & 1) out[3 + k] = weight_grad_for(d[next++], s[3 + k]);
        return out;
    }
};

// (periodic: the box is an input only so that the ops have the schemas of the first-order ones; its slot stays empty)
class CFConvTwiceFunction : public torch::autograd::Function<CFConvTwiceFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const HolderPtr& holder, const c10::IValue& neighbors, const Tensor& positions,
                          const MaybeTensor& box, const Tensor& input, const MaybeTensor& weights1, const MaybeTensor& biases1,
                          const MaybeTensor& weights2, const MaybeTensor& biases2) {
        const Tensor output = run_forward(holder, neighbors, positions, box, input, weights1, biases1, weights2, biases2);
        tensor_list kept = {positions, input};
        if (weights1) kept.insert(kept.end(), {*weights1, *biases1, *weights2, *biases2});
        ctx->save_for_backward(kept);
        ctx->saved_data["holder"] = holder;
        ctx->saved_data["neighbors"] = neighbors;
        ctx->saved_data["build"] = neighbors.toCustomClass<Neighbors>()->getBuildCount();
        ctx->saved_data["uploads"] = weights1 ? holder->getUploads() : (int64_t)-1;
        ctx->saved_data["periodic"] = box.has_value();
        return output;
    }
    static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
        const auto s = ctx->get_saved_variables();           // {positions, input} and, with them, the four weights
        const bool weights = s.size() > 2;
        // (the node's edges count its tensor inputs only: positions, the box where there is one, input, four weights)
        const int64_t wants = weights ? wanted_weights(ctx, ctx->saved_data["periodic"].toBool() ? 3 : 2) : 0;
        const auto weight = [&](int k) { return weights ? MaybeTensor(s[2 + k]) : MaybeTensor(); };
        const tensor_list d = CFConvBackwardFunction::apply(grads[0], s[0], s[1], weight(0), weight(1), weight(2), weight(3),
                                                            ctx->saved_data["holder"].toCustomClass<Holder>(), ctx->saved_data["neighbors"],
                                                            ctx->saved_data["build"].toInt(), ctx->saved_data["uploads"].toInt(), wants);
        tensor_list out = {Tensor(), Tensor(), d[1], Tensor(), d[0]};
        out.resize(9);
        size_t next = 2;
        for (int k = 0; k < 4; k++)
            if (wants >> k & 1) out[5 + k] = weight_grad_for(d[next++], s[2 + k]);
        return out;
    }
};

inline int64_t weight_wants(const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2) {
    if (!torch::GradMode::is_enabled()) return 0;
    return (w1.requires_grad() ? 1 : 0) | (b1.requires_grad() ? 2 : 0) | (w2.requires_grad() ? 4 : 0) | (b2.requires_grad() ? 8 : 0);
}
inline int64_t box_wants(const Tensor& box) { return torch::GradMode::is_enabled() && box.requires_grad() ? 16 : 0; }
const MaybeTensor none;

Tensor operation(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions, const Tensor& input) {
    return CFConvFunction::apply(*holder, neighbors, positions, none, input, none, none, none, none, (int64_t)0);
}

Tensor operation_periodic(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions, const Tensor& box,
                          const Tensor& input) {
    return CFConvFunction::apply(*holder, neighbors, positions, MaybeTensor(box), input, none, none, none, none, box_wants(box));
}

Tensor operation_twice(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions, const Tensor& input) {
    return CFConvTwiceFunction::apply(*holder, neighbors, positions, none, input, none, none, none, none);
}

Tensor operation_periodic_twice(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions,
                                const Tensor& box, const Tensor& input) {
    TORCH_CHECK(!box_wants(box),
                "NNPOpsCFConv::operation_periodic_twice: box gradients need the default op (operation_periodic; CFConv without "
                "twice_differentiable=True): the twice-differentiable ops return no box gradient");
    return CFConvTwiceFunction::apply(*holder, neighbors, positions, MaybeTensor(box), input, none, none, none, none);
}

Tensor operation_weights(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions, const Tensor& input,
                         const Tensor& weights1, const Tensor& biases1, const Tensor& weights2, const Tensor& biases2) {
    return CFConvFunction::apply(*holder, neighbors, positions, none, input, MaybeTensor(weights1), MaybeTensor(biases1), MaybeTensor(weights2),
                                 MaybeTensor(biases2), weight_wants(weights1, biases1, weights2, biases2));
}

Tensor operation_periodic_weights(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions,
                                  const Tensor& box, const Tensor& input, const Tensor& weights1, const Tensor& biases1,
                                  const Tensor& weights2, const Tensor& biases2) {
    TORCH_CHECK(box.defined(), "NNPOpsCFConv::operation_periodic_weights: \"box\" is undefined");
    return CFConvFunction::apply(*holder, neighbors, positions, MaybeTensor(box), input, MaybeTensor(weights1), MaybeTensor(biases1),
                                 MaybeTensor(weights2), MaybeTensor(biases2), weight_wants(weights1, biases1, weights2, biases2) | box_wants(box));
}

Tensor operation_weights_twice(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions,
                               const Tensor& input, const Tensor& weights1, const Tensor& biases1, const Tensor& weights2,
                               const Tensor& biases2) {
    return CFConvTwiceFunction::apply(*holder, neighbors, positions, none, input, MaybeTensor(weights1), MaybeTensor(biases1),
                                      MaybeTensor(weights2), MaybeTensor(biases2));
}

Tensor operation_periodic_weights_twice(const c10::optional<HolderPtr>& holder, const c10::IValue& neighbors, const Tensor& positions,
                                        const Tensor& box, const Tensor& input, const Tensor& weights1, const Tensor& biases1,
                                        const Tensor& weights2, const Tensor& biases2) {
    TORCH_CHECK(box.defined(), "NNPOpsCFConv::operation_periodic_weights_twice: \"box\" is undefined");
    TORCH_CHECK(!box_wants(box),
                "NNPOpsCFConv::operation_periodic_weights_twice: box gradients need the default op or operation_periodic_weights (CFConv "
                "without force_trainable=True): the twice-differentiable ops return no box gradient");
    return CFConvTwiceFunction::apply(*holder, neighbors, positions, MaybeTensor(box), input, MaybeTensor(weights1), MaybeTensor(biases1),
                                      MaybeTensor(weights2), MaybeTensor(biases2));
}

TORCH_LIBRARY(NNPOpsCFConv, m) {
    m.class_<Holder>("Holder")
        .def(torch::init<double, const std::string&, const Tensor&, const Tensor&, const Tensor&, const Tensor&>())
        .def("forward", &Holder::forward)
        .def("backward", &Holder::backward)
        .def("uploads", &Holder::getUploads)
        .def_pickle([](const HolderPtr& self) -> std::string { return Holder::serialize(self); },
                    [](const std::string& state) -> HolderPtr { return Holder::deserialize(state); });
    m.def("operation", operation);
    m.def("operation_periodic", operation_periodic);
    m.def("operation_twice", operation_twice);
    m.def("operation_periodic_twice", operation_periodic_twice);
    m.def("operation_weights", operation_weights);
    m.def("operation_periodic_weights", operation_periodic_weights);
    m.def("operation_weights_twice", operation_weights_twice);
    m.def("operation_periodic_weights_twice", operation_periodic_weights_twice);
}

}  // namespace CFConv
}  // namespace NNPOps

// =============================================================================================
// getNeighborPairs
// =============================================================================================
namespace {

// The transposed index of the LAST list getNeighborPairs emitted on a device with an index (round 6): pme::pme_direct, the list's
// immediate consumer (src/pytorch/pme/pme.py:163-165), finds it here when it is handed that very list -- same storage, same version
// counter, held alive so that the address cannot be handed to another tensor -- and then runs without atomics
// (nnpops_pme_direct_indexed); any other list (edited, shuffled, built by the caller) takes the entry point that assumes nothing.
struct PairIndexCache {
    Tensor neighbors, index;
    uint32_t version = 0;
};
PairIndexCache& pair_index_cache(int device) {
    // (never destroyed: tensors released from a static destructor would reach the allocator after the runtime has shut down.  One entry per
    //  device, i.e. the last list and its index -- 36 bytes per slot -- stay allocated until the next differentiable getNeighborPairs call.)
    static std::mutex guard;
    static std::vector<PairIndexCache>* slots = new std::vector<PairIndexCache>(64);
    std::lock_guard<std::mutex> lock(guard);
    return (*slots)[(size_t)std::max(0, std::min(device, 63))];
}

// ---------------------------------------------------------------------------------------------
// Second order and the box.  The backward pass of getNeighborPairs is itself a differentiable function (both keys):
//     NeighborPairsBackwardFunction        Bwd(grad_deltas, grad_distances, deltas, distances) -> (grad_positions, grad_box)
// Its forward runs the first-order kernels of round 6 unchanged for grad_positions (the indexed gather when the forward op built an
// index, the fixed-point sums otherwise; plain loops on the host key) and adds the box reduction only when the box needs a gradient.
// deltas and distances reach it as the forward op's saved OUTPUTS, so autograd chains its own backward -- the per-slot
//     NeighborPairsDoubleBackwardFunction  (gg_positions, gg_box) -> d(grad_deltas, grad_distances, deltas, distances)
// (pairs_second_order.hip: derivation) -- back through the forward op's backward, which is Bwd again: Hessian-vector products with
// respect to positions and box.  A third derivative raises instead of dropping terms.  Without create_graph and without a box
// gradient nothing of this is recorded: the same kernels as before run, and nothing more is saved.
// ---------------------------------------------------------------------------------------------
template <typename T>
void neighbor_pairs_host_backward(const Tensor& neighbors, const Tensor& deltas, const Tensor& distances, const Tensor& gd,
                                  const Tensor& gr, Tensor& gpos);      // (host key, below)

// the slot's minimum-image shift n_k, recovered from positions, box and its delta (pairs_second_order.hip: image_shift)
template <typename T>
void host_image_shift(const T* pos, const T* box, int64_t i, int64_t j, const T* d, T (&n)[3]) {
    T D[3];
    for (int c = 0; c < 3; c++) D[c] = (pos[3 * i + c] - pos[3 * j + c]) - d[c];
    n[2] = std::round(D[2] / box[8]);
    n[1] = std::round((D[1] - n[2] * box[7]) / box[4]);
    n[0] = std::round((D[0] - n[2] * box[6] - n[1] * box[3]) / box[0]);
}

// grad_box[a][:] = - sum_k n_ka G_k, G_k as neighbor_pairs_host_backward forms it (float64 sums in slot order)
template <typename T>
void neighbor_pairs_host_box_backward(const Tensor& neighbors, const Tensor& positions, const Tensor& box, const Tensor& deltas,
                                      const Tensor& distances, const Tensor& gd, const Tensor& gr, Tensor& gbox) {
    const int64_t slots = distances.size(0), n_atoms = positions.size(0);
    const int32_t* nb = neighbors.data_ptr<int32_t>();
    const T* pos = positions.data_ptr<T>();
    const T* b = box.data_ptr<T>();
    const T* dl = deltas.data_ptr<T>();
    const T* ds = distances.data_ptr<T>();
    const T* pgd = gd.data_ptr<T>();
    const T* pgr = gr.data_ptr<T>();
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t k = 0; k < slots; k++) {
        const int32_t row = nb[k], col = nb[slots + k];
        if (row < 0 || col < 0 || row >= n_atoms || col >= n_atoms) continue;
        T G[3], n[3];
        for (int c = 0; c < 3; c++) G[c] = pgd[3 * k + c] + (ds[k] > 0 ? dl[3 * k + c] / ds[k] * pgr[k] : (T)0);
        host_image_shift<T>(pos, b, row, col, dl + 3 * k, n);
        for (int a = 0; a < 3; a++)
            for (int c = 0; c < 3; c++) acc[3 * a + c] -= (double)n[a] * (double)G[c];
    }
    T* out = gbox.data_ptr<T>();
    for (int q = 0; q < 9; q++) out[q] = (T)acc[q];
}

// the vector-Jacobian product of the backward pass (pairs_second_order.hip), r = 0 guarded as in neighbor_pairs_host_backward
template <typename T>
void neighbor_pairs_host_double_backward(const Tensor& neighbors, const Tensor& positions, const Tensor& box, const Tensor& deltas,
                                         const Tensor& distances, const Tensor& gr, const Tensor& hx, const Tensor& hb, tensor_list& out,
                                         int64_t n_atoms) {
    const int64_t slots = distances.size(0);
    const int32_t* nb = neighbors.data_ptr<int32_t>();
    const T* dl = deltas.data_ptr<T>();
    const T* ds = distances.data_ptr<T>();
    const T* pgr = gr.data_ptr<T>();
    const T* phx = hx.defined() ? hx.data_ptr<T>() : nullptr;
    const T* phb = hb.defined() ? hb.data_ptr<T>() : nullptr;
    const T* pos = phb ? positions.data_ptr<T>() : nullptr;
    const T* b = phb ? box.data_ptr<T>() : nullptr;
    T* o_gd = out[0].data_ptr<T>();
    T* o_gr = out[1].data_ptr<T>();
    T* o_dl = out[2].data_ptr<T>();
    T* o_ds = out[3].data_ptr<T>();
    for (int64_t k = 0; k < slots; k++) {
        const int32_t row = nb[k], col = nb[slots + k];
        T w[3] = {0, 0, 0};
        T a = 0, s = 0, c = 0;
        if (row >= 0 && col >= 0 && row < n_atoms && col < n_atoms) {
            if (phx)
                for (int q = 0; q < 3; q++) w[q] = phx[3 * row + q] - phx[3 * col + q];
            if (phb) {
                T n[3];
                host_image_shift<T>(pos, b, row, col, dl + 3 * k, n);
                for (int q = 0; q < 3; q++) w[q] -= n[0] * phb[q] + n[1] * phb[3 + q] + n[2] * phb[6 + q];
            }
            const T r = ds[k];
            if (r > 0) {
                const T dw = dl[3 * k] * w[0] + dl[3 * k + 1] * w[1] + dl[3 * k + 2] * w[2];
                a = dw / r;
                s = pgr[k] / r;
                c = -s * dw / r;
            }
        }
        for (int q = 0; q < 3; q++) { o_gd[3 * k + q] = w[q]; o_dl[3 * k + q] = s * w[q]; }
        o_gr[k] = a;
        o_ds[k] = c;
    }
}

// grad_positions of the first-order pass: exactly the kernels (host loops) that ran before the box and second order existed
Tensor pairs_grad_positions(const Tensor& neighbors, const Tensor& index, const Tensor& deltas, const Tensor& distances,
                            const Tensor& grad_deltas, const Tensor& grad_distances, int64_t num_atoms) {
    if (!deltas.is_cuda()) {
        Tensor gpos = torch::zeros({num_atoms, 3}, deltas.options());
        if (deltas.scalar_type() == torch::kFloat64) neighbor_pairs_host_backward<double>(neighbors, deltas, distances, grad_deltas, grad_distances, gpos);
        else neighbor_pairs_host_backward<float>(neighbors, deltas, distances, grad_deltas, grad_distances, gpos);
        return gpos;
    }
    Tensor grad_positions = torch::empty({num_atoms, 3}, deltas.options());
    const int dtype = deltas.scalar_type() == torch::kFloat64 ? 1 : 0;
    c10::hip::HIPGuard guard(deltas.device().index());
    if (index.defined()) {
        Tensor terms = torch::empty({nnpops_neighbor_pairs_backward_indexed_workspace_bytes(dtype, distances.size(0)) / 8 + 1},
                                    deltas.options().dtype(torch::kInt64));
        if (nnpops_neighbor_pairs_backward_indexed(dtype, (int)num_atoms, distances.size(0), neighbors.data_ptr<int32_t>(), deltas.data_ptr(),
                                                   distances.data_ptr(), grad_deltas.data_ptr(), grad_distances.data_ptr(),
                                                   index.data_ptr<int32_t>(), grad_positions.data_ptr(), terms.data_ptr(),
                                                   current_stream(deltas.device())) != NNPOPS_OK)
            raise_last("neighbors::getNeighborPairs backward");
        return grad_positions;
    }
    // (scratch for the order-independent fixed-point sums of the backward pass: no float atomics, nnpops_hip.h)
    Tensor workspace = torch::empty({nnpops_neighbor_pairs_backward_workspace_bytes((int)num_atoms) / 8}, deltas.options().dtype(torch::kInt64));
    if (nnpops_neighbor_pairs_backward_ws(dtype, (int)num_atoms, distances.size(0), neighbors.data_ptr<int32_t>(), deltas.data_ptr(),
                                          distances.data_ptr(), grad_deltas.data_ptr(), grad_distances.data_ptr(),
                                          grad_positions.data_ptr(), workspace.data_ptr(), current_stream(deltas.device())) != NNPOPS_OK)
        raise_last("neighbors::getNeighborPairs backward");
    return grad_positions;
}

// grad_box [3, 3] in deltas' dtype; positions and box as the forward op used them (box cast to the positions' dtype)
Tensor pairs_grad_box(const Tensor& neighbors, const Tensor& positions, const Tensor& box, const Tensor& deltas, const Tensor& distances,
                      const Tensor& grad_deltas, const Tensor& grad_distances) {
    Tensor gbox = torch::empty({3, 3}, deltas.options());
    if (!deltas.is_cuda()) {
        if (deltas.scalar_type() == torch::kFloat64)
            neighbor_pairs_host_box_backward<double>(neighbors, positions, box, deltas, distances, grad_deltas, grad_distances, gbox);
        else
            neighbor_pairs_host_box_backward<float>(neighbors, positions, box, deltas, distances, grad_deltas, grad_distances, gbox);
        return gbox;
    }
    const int dtype = deltas.scalar_type() == torch::kFloat64 ? 1 : 0;
    const int64_t slots = distances.size(0);
    c10::hip::HIPGuard guard(deltas.device().index());
    Tensor workspace = torch::empty({nnpops_neighbor_pairs_box_backward_workspace_bytes(slots) / 8}, deltas.options().dtype(torch::kFloat64));
    if (nnpops_neighbor_pairs_box_backward(dtype, (int)positions.size(0), slots, neighbors.data_ptr<int32_t>(), positions.data_ptr(), box.data_ptr(),
                                           deltas.data_ptr(), distances.data_ptr(), grad_deltas.data_ptr(), grad_distances.data_ptr(),
                                           gbox.data_ptr(), workspace.data_ptr(), current_stream(deltas.device())) != NNPOPS_OK)
        raise_last("neighbors::getNeighborPairs backward (box)");
    return gbox;
}

std::optional<Tensor> opt(const Tensor& t) { return t.defined() ? std::optional<Tensor>(t) : std::nullopt; }

class NeighborPairsDoubleBackwardFunction : public torch::autograd::Function<NeighborPairsDoubleBackwardFunction> {
public:
    // (optional tensors: autograd records no input for an absent one)
    static tensor_list forward(AutogradContext* ctx, const std::optional<Tensor>& gg_positions_opt, const std::optional<Tensor>& gg_box_opt,
                               const Tensor& deltas, const Tensor& distances, const Tensor& grad_distances, const Tensor& neighbors,
                               const std::optional<Tensor>& positions_opt, const std::optional<Tensor>& box_opt, int64_t num_atoms) {
        const Tensor gg_positions = gg_positions_opt.value_or(Tensor()), gg_box = gg_box_opt.value_or(Tensor());
        const Tensor positions = positions_opt.value_or(Tensor()), box = box_opt.value_or(Tensor());
        const int64_t slots = distances.size(0);
        tensor_list out = {torch::empty({slots, 3}, deltas.options()), torch::empty({slots}, deltas.options()),
                           torch::empty({slots, 3}, deltas.options()), torch::empty({slots}, deltas.options())};
        const Tensor hb = box.defined() ? gg_box : Tensor();
        if (!deltas.is_cuda()) {
            if (deltas.scalar_type() == torch::kFloat64)
                neighbor_pairs_host_double_backward<double>(neighbors, positions, box, deltas, distances, grad_distances, gg_positions, hb, out, num_atoms);
            else
                neighbor_pairs_host_double_backward<float>(neighbors, positions, box, deltas, distances, grad_distances, gg_positions, hb, out, num_atoms);
            return out;
        }
        auto ptr = [](const Tensor& t) -> const void* { return t.defined() ? t.data_ptr() : nullptr; };
        c10::hip::HIPGuard guard(deltas.device().index());
        if (nnpops_neighbor_pairs_double_backward(deltas.scalar_type() == torch::kFloat64 ? 1 : 0, (int)num_atoms, slots, neighbors.data_ptr<int32_t>(),
                                                  hb.defined() ? positions.data_ptr() : nullptr, hb.defined() ? box.data_ptr() : nullptr,
                                                  deltas.data_ptr(), distances.data_ptr(), grad_distances.data_ptr(), ptr(gg_positions), ptr(hb),
                                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                                  current_stream(deltas.device())) != NNPOPS_OK)
            raise_last("neighbors::getNeighborPairs double backward");
        return out;
    }

    static tensor_list backward(AutogradContext*, tensor_list) {
        TORCH_CHECK(false, "neighbors::getNeighborPairs: third derivatives are not implemented");
        return {};
    }
};

class NeighborPairsBackwardFunction : public torch::autograd::Function<NeighborPairsBackwardFunction> {
public:
    // positions / box: defined (detached, box in the positions' dtype) only when want_box
    static tensor_list forward(AutogradContext* ctx, const Tensor& grad_deltas, const Tensor& grad_distances, const Tensor& deltas,
                               const Tensor& distances, const Tensor& neighbors, const std::optional<Tensor>& index_opt,
                               const std::optional<Tensor>& positions_opt, const std::optional<Tensor>& box_opt, int64_t num_atoms,
                               bool want_positions, bool want_box) {
        const Tensor index = index_opt.value_or(Tensor()), positions = positions_opt.value_or(Tensor()), box = box_opt.value_or(Tensor());
        // -> {grad_positions if want_positions, grad_box if want_box} (no undefined outputs: autograd cannot describe them)
        ctx->set_materialize_grads(false);
        tensor_list out;
        if (want_positions) out.push_back(pairs_grad_positions(neighbors, index, deltas, distances, grad_deltas, grad_distances, num_atoms));
        if (want_box) out.push_back(pairs_grad_box(neighbors, positions, box, deltas, distances, grad_deltas, grad_distances));
        ctx->save_for_backward({deltas, distances, grad_distances, neighbors, positions, box});
        ctx->saved_data["num_atoms"] = num_atoms;
        ctx->saved_data["want_positions"] = want_positions;
        return out;
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
        const auto saved = ctx->get_saved_variables();
        const Tensor deltas = saved[0], distances = saved[1], grad_distances = saved[2], neighbors = saved[3], positions = saved[4], box = saved[5];
        const bool want_positions = ctx->saved_data["want_positions"].toBool();
        const Tensor gx = want_positions ? grads[0] : Tensor();
        const Tensor gb = box.defined() ? grads[want_positions ? 1 : 0] : Tensor();
        const Tensor hx = gx.defined() ? gx.contiguous() : Tensor();
        const Tensor hb = gb.defined() ? gb.contiguous() : Tensor();
        tensor_list out(11);
        if (!hx.defined() && !hb.defined()) return out;
        const tensor_list d = NeighborPairsDoubleBackwardFunction::apply(opt(hx), opt(hb), deltas, distances, grad_distances, neighbors, opt(positions),
                                                                         opt(box), ctx->saved_data["num_atoms"].toInt());
        for (int q = 0; q < 4; q++) out[q] = d[q];
        return out;
    }
};

// the forward ops' backward: Bwd, and the box gradient back in box_vectors' own dtype
tensor_list neighbor_pairs_backward_entry(AutogradContext* ctx, const tensor_list& grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    const Tensor neighbors = saved[0], deltas = saved[1], distances = saved[2], index = saved[3], positions = saved[4], box = saved[5];
    const int64_t num_atoms = ctx->saved_data["num_atoms"].toInt();
    const Tensor grad_deltas = grad_outputs[1].defined() ? grad_outputs[1].contiguous() : torch::zeros_like(deltas);
    const Tensor grad_distances = grad_outputs[2].defined() ? grad_outputs[2].contiguous() : torch::zeros_like(distances);
    const bool want_box = ctx->needs_input_grad(1) && box.defined();
    const tensor_list g = NeighborPairsBackwardFunction::apply(grad_deltas, grad_distances, deltas, distances, neighbors, opt(index),
                                                               opt(want_box ? positions : Tensor()), opt(want_box ? box : Tensor()), num_atoms,
                                                               ctx->needs_input_grad(0), want_box);
    const bool want_positions = ctx->needs_input_grad(0);
    const Tensor grad_positions = want_positions ? g[0] : Tensor();
    const Tensor grad_box = want_box ? g[want_positions ? 1 : 0].to((torch::ScalarType)ctx->saved_data["box_dtype"].toInt()) : Tensor();
    return {grad_positions, Tensor(), Tensor(), grad_box, Tensor()};
}

class NeighborPairsFunction : public torch::autograd::Function<NeighborPairsFunction> {
public:
    static tensor_list forward(AutogradContext* ctx, const Tensor& positions, const torch::Scalar& cutoff,
                               const torch::Scalar& max_num_pairs, const Tensor& box_vectors, bool checkErrors) {
        // checks and messages of the reference (getNeighborPairsCUDA.cu:112-126,145-146)
        TORCH_CHECK(positions.dim() == 2, "Expected \"positions\" to have two dimensions");
        TORCH_CHECK(positions.size(0) > 0, "Expected the 1nd dimension size of \"positions\" to be more than 0");
        TORCH_CHECK(positions.size(1) == 3, "Expected the 2nd dimension size of \"positions\" to be 3");
        TORCH_CHECK(positions.is_contiguous(), "Expected \"positions\" to be contiguous");
        TORCH_CHECK(positions.scalar_type() == torch::kFloat32 || positions.scalar_type() == torch::kFloat64,
                    "Expected \"positions\" to be float32 or float64");
        const int64_t max_pairs = max_num_pairs.toLong();
        TORCH_CHECK(max_pairs > 0 || max_pairs == -1, "Expected \"max_num_pairs\" to be positive or equal to -1");
        TORCH_CHECK(cutoff.toDouble() > 0, "Expected \"cutoff\" to be positive");
        const bool use_periodic = box_vectors.size(0) != 0;
        Tensor box;
        if (use_periodic) {
            TORCH_CHECK(box_vectors.dim() == 2, "Expected \"box_vectors\" to have two dimensions");
            TORCH_CHECK(box_vectors.size(0) == 3 && box_vectors.size(1) == 3, "Expected \"box_vectors\" to have shape (3, 3)");
            box = box_vectors.to(positions.options()).contiguous();
        }
        const int64_t num_atoms = positions.size(0);
        // (argument limits of the C ABI, checked before anything is allocated)
        TORCH_CHECK(num_atoms <= std::numeric_limits<int32_t>::max(), "Too many atoms for getNeighborPairs");
        TORCH_CHECK(max_pairs != -1 || num_atoms <= 65536,
                    "max_num_pairs == -1 needs one slot per pair; beyond 65536 atoms use a compacted list");
        const int64_t slots = max_pairs == -1 ? num_atoms * (num_atoms - 1) / 2 : max_pairs;
        const auto options = positions.options();
        Tensor neighbors = torch::empty({2, slots}, options.dtype(torch::kInt32));
        Tensor deltas = torch::empty({slots, 3}, options);
        Tensor distances = torch::empty({slots}, options);
        Tensor num_pairs = torch::empty({1}, options.dtype(torch::kInt32));
        Tensor workspace = torch::empty({nnpops_neighbor_pairs_workspace_bytes((int)num_atoms)}, options.dtype(torch::kUInt8));
        const int dtype = positions.scalar_type() == torch::kFloat64 ? 1 : 0;
        c10::hip::HIPGuard guard(positions.device().index());
        void* stream = current_stream(positions.device());
        if (nnpops_neighbor_pairs_forward(dtype, (int)num_atoms, positions.data_ptr(), use_periodic ? box.data_ptr() : nullptr,
                                          cutoff.toDouble(), max_pairs, neighbors.data_ptr<int32_t>(), deltas.data_ptr(),
                                          distances.data_ptr(), num_pairs.data_ptr<int32_t>(), workspace.data_ptr(), stream) != NNPOPS_OK)
            raise_last("neighbors::getNeighborPairs");
        if (checkErrors) {      // synchronises: incompatible with graph capture, as documented by the reference (:156-160)
            const int found = num_pairs.item<int32_t>();
            TORCH_CHECK(found <= slots, "Too many neighbor pairs found. Maximum is " + std::to_string(slots),
                        " but found " + std::to_string(found));
        }
        // Round 6: the backward pass of a COMPACTED list is an owner-computes gather over the list's transposed index (no atomics,
        // include/nnpops_hip.h: nnpops_neighbor_pairs_build_index).  The index is a function of `neighbors` alone and the list is
        // grouped by row as this op emits it, so it is built here, once, when a gradient can be asked for, and travels with the saved
        // tensors (which autograd protects against in-place edits).  max_num_pairs == -1 (one slot per candidate pair, small systems)
        // and $NNPOPS_PAIRS_BACKWARD=fixed keep the order-independent fixed-point sums, which assume nothing about the list.
        Tensor index;
        const char* bwd_env = std::getenv("NNPOPS_PAIRS_BACKWARD");
        const bool fixed_point_only = bwd_env && std::string(bwd_env) == "fixed";
        if (positions.requires_grad() && max_pairs > 0 && !fixed_point_only && num_atoms <= NNPOPS_PAIRS_INDEX_MAX_ATOMS) {
            index = torch::empty({nnpops_neighbor_pairs_index_ints((int)num_atoms, slots)}, options.dtype(torch::kInt32));
            Tensor iws = torch::empty({nnpops_neighbor_pairs_index_workspace_bytes((int)num_atoms, slots) / 8 + 1}, options.dtype(torch::kInt64));
            if (nnpops_neighbor_pairs_build_index((int)num_atoms, slots, neighbors.data_ptr<int32_t>(), index.data_ptr<int32_t>(), iws.data_ptr(),
                                                  stream) != NNPOPS_OK)
                raise_last("neighbors::getNeighborPairs (transposed index)");
            PairIndexCache& cache = pair_index_cache(positions.device().index());
            cache.neighbors = neighbors; cache.index = index; cache.version = neighbors._version();
        }
        // (positions and the cast box only when the box needs a gradient: its n_k are recovered from them, pairs_second_order.hip)
        const bool box_grad = use_periodic && box_vectors.requires_grad();
        ctx->save_for_backward({neighbors, deltas, distances, index, box_grad ? positions.detach() : Tensor(), box_grad ? box.detach() : Tensor()});
        ctx->saved_data["num_atoms"] = num_atoms;
        ctx->saved_data["box_dtype"] = (int64_t)box_vectors.scalar_type();
        return {neighbors, deltas, distances, num_pairs};
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) { return neighbor_pairs_backward_entry(ctx, grad_outputs); }
};

TORCH_LIBRARY(neighbors, m) {
    m.def("getNeighborPairs(Tensor positions, Scalar cutoff, Scalar max_num_neighbors, Tensor box_vectors, bool checkErrors) -> "
          "(Tensor neighbors, Tensor deltas, Tensor distances, Tensor num_pairs)");
}

std::tuple<Tensor, Tensor, Tensor, Tensor> neighbor_pairs_device_entry(const Tensor& positions, const torch::Scalar& cutoff,
                                                                       const torch::Scalar& max_num_pairs, const Tensor& box_vectors,
                                                                       bool checkErrors) {
    const tensor_list r = NeighborPairsFunction::apply(positions, cutoff, max_num_pairs, box_vectors, checkErrors);
    return std::make_tuple(r[0], r[1], r[2], r[3]);
}
TORCH_LIBRARY_IMPL(neighbors, AutogradCUDA, m) { m.impl("getNeighborPairs", neighbor_pairs_device_entry); }
// (the backend key itself: what runs below autograd -- torch.inference_mode(), AutoDispatchBelowAutograd)
TORCH_LIBRARY_IMPL(neighbors, CUDA, m) { m.impl("getNeighborPairs", neighbor_pairs_device_entry); }

// ---------------------------------------------------------------------------------------------
// Host tensors.  The reference registers a CPU kernel of this op next to the device one (reference
// src/pytorch/neighbors/getNeighborPairsCPU.cpp:19-108, a composition of differentiable ATen calls that materialises
// all N(N-1)/2 candidate pairs); a drop-in keeps that dispatch key alive.  This is NOT a fallback of the device path --
// device tensors never come here, and a missing HIP library still fails at import -- it is what `positions.cpu()`
// callers of the reference get.  Written as plain loops over the pairs (no N^2 temporaries), same results:
//   * pair k <-> (row, column < row) in the reference's tril order, delta = positions[row] - positions[column],
//     triclinic wrap z, y, x with one round() each (:66-68), distance in the positions' dtype;
//   * max_num_pairs == -1: every slot kept, pairs beyond the cutoff masked with -1 / NaN (:72-78);
//   * otherwise: pairs with distance <= cutoff in tril order, padded with -1 / NaN up to max_num_pairs and NOT
//     truncated beyond it; num_pairs reports the length after padding, as the reference's CPU kernel does (:97-98).
// ---------------------------------------------------------------------------------------------
template <typename T>
void neighbor_pairs_host(const Tensor& positions, const Tensor& box, double cutoff, int64_t max_pairs, bool check,
                         Tensor& neighbors, Tensor& deltas, Tensor& distances) {
    const int64_t n = positions.size(0);
    const T* pos = positions.data_ptr<T>();
    const bool periodic = box.defined();
    T b[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (periodic) {
        const Tensor bc = box.to(positions.scalar_type()).contiguous();
        for (int i = 0; i < 9; i++) b[i / 3][i % 3] = bc.data_ptr<T>()[i];
    }
    const T cut = (T)cutoff;
    auto pair = [&](int64_t row, int64_t col, T (&d)[3]) -> T {
        for (int c = 0; c < 3; c++) d[c] = pos[3 * row + c] - pos[3 * col + c];
        if (periodic)
            for (int axis = 2; axis >= 0; axis--) {
                const T s = std::round(d[axis] / b[axis][axis]);
                for (int c = 0; c < 3; c++) d[c] -= s * b[axis][c];
            }
        return std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    };
    const T nan = std::numeric_limits<T>::quiet_NaN();
    const auto iopt = positions.options().dtype(torch::kInt32);
    if (max_pairs == -1) {
        const int64_t slots = n * (n - 1) / 2;
        neighbors = torch::empty({2, slots}, iopt);
        deltas = torch::empty({slots, 3}, positions.options());
        distances = torch::empty({slots}, positions.options());
        int32_t* nb = neighbors.data_ptr<int32_t>();
        T* dl = deltas.data_ptr<T>();
        T* ds = distances.data_ptr<T>();
        int64_t k = 0;
        for (int64_t row = 1; row < n; row++)
            for (int64_t col = 0; col < row; col++, k++) {
                T d[3];
                const T r = pair(row, col, d);
                const bool keep = !(r > cut);                  // the reference masks `distances > cutoff`
                nb[k] = keep ? (int32_t)row : -1;
                nb[slots + k] = keep ? (int32_t)col : -1;
                for (int c = 0; c < 3; c++) dl[3 * k + c] = keep ? d[c] : nan;
                ds[k] = keep ? r : nan;
            }
        return;
    }
    int64_t found = 0;
    for (int64_t row = 1; row < n; row++)
        for (int64_t col = 0; col < row; col++) {
            T d[3];
            found += pair(row, col, d) <= cut ? 1 : 0;
        }
    if (check)
        TORCH_CHECK(found <= max_pairs, "The maximum number of pairs has been exceed! Increase \"max_num_pairs\"");
    const int64_t slots = std::max(found, max_pairs);
    neighbors = torch::full({2, slots}, -1, iopt);
    deltas = torch::full({slots, 3}, nan, positions.options());
    distances = torch::full({slots}, nan, positions.options());
    int32_t* nb = neighbors.data_ptr<int32_t>();
    T* dl = deltas.data_ptr<T>();
    T* ds = distances.data_ptr<T>();
    int64_t k = 0;
    for (int64_t row = 1; row < n; row++)
        for (int64_t col = 0; col < row; col++) {
            T d[3];
            const T r = pair(row, col, d);
            if (!(r <= cut)) continue;
            nb[k] = (int32_t)row;
            nb[slots + k] = (int32_t)col;
            for (int c = 0; c < 3; c++) dl[3 * k + c] = d[c];
            ds[k++] = r;
        }
}

template <typename T>
void neighbor_pairs_host_backward(const Tensor& neighbors, const Tensor& deltas, const Tensor& distances, const Tensor& gd,
                                  const Tensor& gr, Tensor& gpos) {
    const int64_t slots = distances.size(0);
    const int32_t* nb = neighbors.data_ptr<int32_t>();
    const T* dl = deltas.data_ptr<T>();
    const T* ds = distances.data_ptr<T>();
    const T* pgd = gd.data_ptr<T>();
    const T* pgr = gr.data_ptr<T>();
    T* out = gpos.data_ptr<T>();
    for (int64_t k = 0; k < slots; k++) {
        const int32_t row = nb[k], col = nb[slots + k];
        if (row < 0) continue;                                 // masked / padding slot: no gradient (as the device kernel)
        for (int c = 0; c < 3; c++) {
            const T g = pgd[3 * k + c] + (ds[k] > 0 ? dl[3 * k + c] / ds[k] * pgr[k] : (T)0);
            out[3 * row + c] += g;
            out[3 * col + c] -= g;
        }
    }
}

class NeighborPairsHostFunction : public torch::autograd::Function<NeighborPairsHostFunction> {
public:
    static tensor_list forward(AutogradContext* ctx, const Tensor& positions, const torch::Scalar& cutoff,
                               const torch::Scalar& max_num_pairs, const Tensor& box_vectors, bool checkErrors) {
        // checks and messages of the reference's CPU kernel (getNeighborPairsCPU.cpp:25-53)
        TORCH_CHECK(positions.dim() == 2, "Expected \"positions\" to have two dimensions");
        TORCH_CHECK(positions.size(0) > 0, "Expected the 1nd dimension size of \"positions\" to be more than 0");
        TORCH_CHECK(positions.size(1) == 3, "Expected the 2nd dimension size of \"positions\" to be 3");
        TORCH_CHECK(positions.is_contiguous(), "Expected \"positions\" to be contiguous");
        TORCH_CHECK(positions.scalar_type() == torch::kFloat32 || positions.scalar_type() == torch::kFloat64,
                    "Expected \"positions\" to be float32 or float64");
        const double c = cutoff.toDouble();
        TORCH_CHECK(c > 0, "Expected \"cutoff\" to be positive");
        Tensor box;
        if (box_vectors.size(0) != 0) {
            TORCH_CHECK(box_vectors.dim() == 2, "Expected \"box_vectors\" to have two dimensions");
            TORCH_CHECK(box_vectors.size(0) == 3 && box_vectors.size(1) == 3, "Expected \"box_vectors\" to have shape (3, 3)");
            const Tensor v64 = box_vectors.to(torch::kFloat64).contiguous();
            const double* v = v64.data_ptr<double>();
            TORCH_CHECK(v[1] == 0, "Invalid box vectors: box_vectors[0][1] != 0");
            TORCH_CHECK(v[2] == 0, "Invalid box vectors: box_vectors[0][2] != 0");
            TORCH_CHECK(v[5] == 0, "Invalid box vectors: box_vectors[1][2] != 0");
            TORCH_CHECK(v[0] >= 2 * c, "Invalid box vectors: box_vectors[0][0] < 2*cutoff");
            TORCH_CHECK(v[4] >= 2 * c, "Invalid box vectors: box_vectors[1][1] < 2*cutoff");
            TORCH_CHECK(v[8] >= 2 * c, "Invalid box vectors: box_vectors[2][2] < 2*cutoff");
            TORCH_CHECK(v[0] >= 2 * v[3], "Invalid box vectors: box_vectors[0][0] < 2*box_vectors[1][0]");
            TORCH_CHECK(v[0] >= 2 * v[6], "Invalid box vectors: box_vectors[0][0] < 2*box_vectors[2][0]");
            TORCH_CHECK(v[4] >= 2 * v[7], "Invalid box vectors: box_vectors[1][1] < 2*box_vectors[2][1]");
            box = box_vectors;
        }
        const int64_t max_pairs = max_num_pairs.toLong();
        TORCH_CHECK(max_pairs > 0 || max_pairs == -1, "Expected \"max_num_pairs\" to be positive or equal to -1");
        Tensor neighbors, deltas, distances;
        if (positions.scalar_type() == torch::kFloat64)
            neighbor_pairs_host<double>(positions, box, c, max_pairs, checkErrors, neighbors, deltas, distances);
        else
            neighbor_pairs_host<float>(positions, box, c, max_pairs, checkErrors, neighbors, deltas, distances);
        Tensor num_pairs = torch::empty({1}, positions.options().dtype(torch::kInt32));
        num_pairs.data_ptr<int32_t>()[0] = (int32_t)distances.size(0);
        const bool box_grad = box.defined() && box_vectors.requires_grad();
        ctx->save_for_backward({neighbors, deltas, distances, Tensor(), box_grad ? positions.detach() : Tensor(),
                                box_grad ? box_vectors.detach().to(positions.scalar_type()).contiguous() : Tensor()});
        ctx->saved_data["num_atoms"] = positions.size(0);
        ctx->saved_data["box_dtype"] = (int64_t)box_vectors.scalar_type();
        return {neighbors, deltas, distances, num_pairs};
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) { return neighbor_pairs_backward_entry(ctx, grad_outputs); }
};

std::tuple<Tensor, Tensor, Tensor, Tensor> neighbor_pairs_host_entry(const Tensor& positions, const torch::Scalar& cutoff,
                                                                     const torch::Scalar& max_num_pairs, const Tensor& box_vectors,
                                                                     bool checkErrors) {
    const tensor_list r = NeighborPairsHostFunction::apply(positions, cutoff, max_num_pairs, box_vectors, checkErrors);
    return std::make_tuple(r[0], r[1], r[2], r[3]);
}
TORCH_LIBRARY_IMPL(neighbors, AutogradCPU, m) { m.impl("getNeighborPairs", neighbor_pairs_host_entry); }
// the reference registers under the CPU key (getNeighborPairsCPU.cpp:102-108): reachable below autograd too
TORCH_LIBRARY_IMPL(neighbors, CPU, m) { m.impl("getNeighborPairs", neighbor_pairs_host_entry); }

// =============================================================================================
// PME, direct-space part (reference src/pytorch/pme/pme.cpp:4, pmeCUDA.cu:30-100,236-290, pmeCPU.cpp:75-175): same op
// name and schema; the energy's autograd backward scales the derivatives computed in the forward pass, exactly as the
// reference does.  The reciprocal-space op (pme_reciprocal) follows it below.
// =============================================================================================
// the energy and its derivatives, and the inputs as the kernels read them
struct PmeDirectForward {
    Tensor energy, pos_deriv, charge_deriv;
    Tensor pos, q, nb, dl, ds, ex;
    Tensor index;      // the list's cached transposed index when the indexed kernels ran (pme_direct_twice keeps it)
};

class PmeDirectFunction : public torch::autograd::Function<PmeDirectFunction> {
public:
    // the forward pass on either key, shared with pme_direct_box
    static PmeDirectForward run(const Tensor& positions, const Tensor& charges, const Tensor& neighbors, const Tensor& deltas,
                                const Tensor& distances, const Tensor& exclusions, const torch::Scalar& alpha, const torch::Scalar& coulomb) {
        TORCH_CHECK(positions.dim() == 2 && positions.size(1) == 3, "positions must have shape (atoms, 3)");
        TORCH_CHECK(charges.dim() == 1 && charges.size(0) == positions.size(0), "charges must be 1D, one per atom");
        TORCH_CHECK(neighbors.dim() == 2 && neighbors.size(0) == 2, "neighbors must have shape (2, pairs)");
        TORCH_CHECK(exclusions.dim() == 2 && exclusions.size(0) == positions.size(0), "exclusions must have shape (atoms, max_exclusions)");
        TORCH_CHECK(positions.scalar_type() == torch::kFloat32 && charges.scalar_type() == torch::kFloat32 &&
                    deltas.scalar_type() == torch::kFloat32 && distances.scalar_type() == torch::kFloat32, "pme_direct computes in float32");
        const int64_t n = positions.size(0), pairs = neighbors.size(1), max_excl = exclusions.size(1);
        TORCH_CHECK(deltas.dim() == 2 && deltas.size(0) == pairs && deltas.size(1) == 3, "deltas must have shape (pairs, 3)");
        TORCH_CHECK(distances.dim() == 1 && distances.size(0) == pairs, "distances must have shape (pairs)");
        TORCH_CHECK(at::isIntegralType(neighbors.scalar_type(), false) && at::isIntegralType(exclusions.scalar_type(), false),
                    "neighbors and exclusions must hold integer indices");
        for (const Tensor* t : {&charges, &neighbors, &deltas, &distances, &exclusions})
            TORCH_CHECK(t->device() == positions.device(), "pme_direct: every tensor must be on the device of positions (",
                        positions.device(), "), got ", t->device());
        const Tensor pos = positions.contiguous(), q = charges.contiguous(), nb = neighbors.to(torch::kInt32).contiguous(),
                     dl = deltas.contiguous(), ds = distances.contiguous(), ex = exclusions.to(torch::kInt32).contiguous();
        const auto opts = positions.options();
        Tensor energy = torch::empty({}, opts), pos_deriv = torch::empty({n, 3}, opts), charge_deriv = torch::empty({n}, opts);
        const float a = (float)alpha.toDouble(), k = (float)coulomb.toDouble();
        Tensor used_index;
        if (positions.is_cuda()) {
            c10::hip::HIPGuard guard(positions.device().index());
            const PairIndexCache& cache = pair_index_cache(positions.device().index());
            const bool indexed = cache.index.defined() && cache.neighbors.defined() && nb.data_ptr() == cache.neighbors.data_ptr() &&
                                 nb.sizes() == cache.neighbors.sizes() && nb._version() == cache.version &&
                                 cache.index.numel() == nnpops_neighbor_pairs_index_ints((int)n, pairs);
            if (indexed) {
                used_index = cache.index;
                Tensor workspace = torch::empty({nnpops_pme_direct_indexed_workspace_bytes(pairs, (int)n)}, opts.dtype(torch::kUInt8));
                if (nnpops_pme_direct_indexed((int)n, pairs, (int)max_excl, pos.data_ptr<float>(), q.data_ptr<float>(), nb.data_ptr<int32_t>(),
                                              dl.data_ptr<float>(), ds.data_ptr<float>(), max_excl ? ex.data_ptr<int32_t>() : nullptr,
                                              cache.index.data_ptr<int32_t>(), a, k, energy.data_ptr<float>(), pos_deriv.data_ptr<float>(),
                                              charge_deriv.data_ptr<float>(), workspace.data_ptr(), current_stream(positions.device())) != NNPOPS_OK)
                    raise_last("pme::pme_direct");
            } else {
            Tensor workspace = torch::empty({nnpops_pme_direct_workspace_bytes(pairs, (int)n, (int)max_excl)}, opts.dtype(torch::kUInt8));
            if (nnpops_pme_direct((int)n, pairs, (int)max_excl, pos.data_ptr<float>(), q.data_ptr<float>(), nb.data_ptr<int32_t>(),
                                  dl.data_ptr<float>(), ds.data_ptr<float>(), max_excl ? ex.data_ptr<int32_t>() : nullptr, a, k,
                                  energy.data_ptr<float>(), pos_deriv.data_ptr<float>(), charge_deriv.data_ptr<float>(),
                                  workspace.data_ptr(), current_stream(positions.device())) != NNPOPS_OK)
                raise_last("pme::pme_direct");
            }
        } else {
            // host tensors: the reference registers a CPU kernel too (pmeCPU.cpp:75-163); plain loops, double energy
            pos_deriv.zero_();
            charge_deriv.zero_();
            const float* P = pos.data_ptr<float>(); const float* Q = q.data_ptr<float>();
            const int32_t* N0 = nb.data_ptr<int32_t>(); const int32_t* N1 = N0 + pairs; const int32_t* E = ex.data_ptr<int32_t>();
            float* PD = pos_deriv.data_ptr<float>(); float* CD = charge_deriv.data_ptr<float>();
            const float* DL = dl.data_ptr<float>(); const float* DS = ds.data_ptr<float>();
            const float two_over_sqrt_pi = 1.12837916709551257390f;
            double e = 0.0;
            for (int64_t i = 0; i < pairs; i++) {
                const int a1 = N0[i], a2 = N1[i];
                TORCH_CHECK(a1 < n && a2 < n && (a1 < 0 || a2 >= 0), "pme_direct: neighbor index out of range at pair ", i);
                bool include = a1 > -1;
                for (int64_t j = 0; include && j < max_excl && E[a1 * max_excl + j] >= a2; j++)
                    if (E[a1 * max_excl + j] == a2) include = false;
                if (!include) continue;
                const float r = DS[i], inv_r = 1 / r, ar = a * r, pre = k * inv_r, er = std::erfc(ar);
                e += pre * er * Q[a1] * Q[a2];
                CD[a1] += pre * er * Q[a2];
                CD[a2] += pre * er * Q[a1];
                const float dedr = pre * Q[a1] * Q[a2] * (er + ar * std::exp(-ar * ar) * two_over_sqrt_pi) * inv_r * inv_r;
                for (int c = 0; c < 3; c++) { PD[3 * a1 + c] -= dedr * DL[3 * i + c]; PD[3 * a2 + c] += dedr * DL[3 * i + c]; }
            }
            for (int64_t a1 = 0; a1 < n; a1++)
                for (int64_t j = 0; j < max_excl && E[a1 * max_excl + j] > a1; j++) {
                    const int a2 = E[a1 * max_excl + j];
                    TORCH_CHECK(a2 < n, "pme_direct: exclusion index out of range for atom ", a1);
                    float d[3];
                    for (int c = 0; c < 3; c++) d[c] = P[3 * a1 + c] - P[3 * a2 + c];
                    const float r = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), inv_r = 1 / r, ar = a * r, pre = k * inv_r, er = std::erf(ar);
                    e -= pre * er * Q[a1] * Q[a2];
                    CD[a1] -= pre * er * Q[a2];
                    CD[a2] -= pre * er * Q[a1];
                    const float dedr = pre * Q[a1] * Q[a2] * (er - ar * std::exp(-ar * ar) * two_over_sqrt_pi) * inv_r * inv_r;
                    for (int c = 0; c < 3; c++) { PD[3 * a1 + c] += dedr * d[c]; PD[3 * a2 + c] -= dedr * d[c]; }
                }
            energy.fill_((float)e);
        }
        return {energy, pos_deriv, charge_deriv, pos, q, nb, dl, ds, ex, used_index};
    }

    static Tensor forward(AutogradContext* ctx, const Tensor& positions, const Tensor& charges, const Tensor& neighbors,
                          const Tensor& deltas, const Tensor& distances, const Tensor& exclusions, const torch::Scalar& alpha,
                          const torch::Scalar& coulomb) {
        const PmeDirectForward f = run(positions, charges, neighbors, deltas, distances, exclusions, alpha, coulomb);
        ctx->save_for_backward({f.pos_deriv, f.charge_deriv});
        return f.energy;
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
        // The derivatives were computed (and detached) in the forward pass: a backward pass that is itself being recorded
        // (create_graph=True: force matching, Hessians) would silently see d(force)/d(positions, charges) = 0 from here.
        TORCH_CHECK(!torch::GradMode::is_enabled(),
                    "pme_direct: second derivatives are not implemented (backward was called with create_graph=True)");
        const auto saved = ctx->get_saved_variables();
        return {saved[0] * grad_outputs[0], saved[1] * grad_outputs[0], Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

// pme_direct_box: pme_direct's forward (same kernels, same bits, the indexed path included) and, when box_vectors needs a gradient,
// dE/dB = - sum_k n_k (x) G_k over the included pairs (nnpops_pme_direct_box / the host loop below), computed in the forward pass
// like the other derivatives.  No gradient flows into deltas or distances, as with pme_direct: a list whose deltas depend on the box
// is not counted twice.
class PmeDirectBoxFunction : public torch::autograd::Function<PmeDirectBoxFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& positions, const Tensor& charges, const Tensor& neighbors,
                          const Tensor& deltas, const Tensor& distances, const Tensor& exclusions, const Tensor& box_vectors,
                          const torch::Scalar& alpha, const torch::Scalar& coulomb, bool box_grad) {
        TORCH_CHECK(box_vectors.dim() == 2 && box_vectors.size(0) == 3 && box_vectors.size(1) == 3, "box_vectors must have shape (3, 3)");
        TORCH_CHECK(box_vectors.scalar_type() == torch::kFloat32, "pme_direct_box computes in float32");
        TORCH_CHECK(box_vectors.device() == positions.device(), "pme_direct_box: every tensor must be on the device of positions (",
                    positions.device(), "), got ", box_vectors.device());
        const PmeDirectForward f = PmeDirectFunction::run(positions, charges, neighbors, deltas, distances, exclusions, alpha, coulomb);
        Tensor grad_box;
        if (box_grad) {
            const Tensor box = box_vectors.contiguous();
            const int64_t n = f.pos.size(0), pairs = f.nb.size(1), max_excl = f.ex.size(1);
            const float a = (float)alpha.toDouble(), k = (float)coulomb.toDouble();
            grad_box = torch::empty({3, 3}, f.pos.options());
            if (positions.is_cuda()) {
                c10::hip::HIPGuard guard(positions.device().index());
                Tensor workspace = torch::empty({nnpops_pme_direct_box_workspace_bytes(pairs) / 8}, f.pos.options().dtype(torch::kFloat64));
                if (nnpops_pme_direct_box((int)n, pairs, (int)max_excl, f.pos.data_ptr<float>(), f.q.data_ptr<float>(), f.nb.data_ptr<int32_t>(),
                                          f.dl.data_ptr<float>(), f.ds.data_ptr<float>(), max_excl ? f.ex.data_ptr<int32_t>() : nullptr,
                                          box.data_ptr<float>(), a, k, grad_box.data_ptr<float>(), workspace.data_ptr(),
                                          current_stream(positions.device())) != NNPOPS_OK)
                    raise_last("pme::pme_direct_box");
            } else {
                // the same inclusion test, dedr and shift recovery as the device pass; double sums
                const float* P = f.pos.data_ptr<float>(); const float* Q = f.q.data_ptr<float>(); const float* B = box.data_ptr<float>();
                const int32_t* N0 = f.nb.data_ptr<int32_t>(); const int32_t* N1 = N0 + pairs; const int32_t* E = f.ex.data_ptr<int32_t>();
                const float* DL = f.dl.data_ptr<float>(); const float* DS = f.ds.data_ptr<float>();
                const float two_over_sqrt_pi = 1.12837916709551257390f;
                double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                for (int64_t i = 0; i < pairs; i++) {
                    const int a1 = N0[i], a2 = N1[i];
                    if (a1 < 0) continue;
                    float D[3], sh[3];
                    for (int c = 0; c < 3; c++) D[c] = (P[3 * a1 + c] - P[3 * a2 + c]) - DL[3 * i + c];
                    sh[2] = std::round(D[2] / B[8]);
                    sh[1] = std::round((D[1] - sh[2] * B[7]) / B[4]);
                    sh[0] = std::round((D[0] - sh[2] * B[6] - sh[1] * B[3]) / B[0]);
                    if (sh[0] == 0 && sh[1] == 0 && sh[2] == 0) continue;         // (adds exactly nothing)
                    bool include = true;
                    for (int64_t j = 0; include && j < max_excl && E[a1 * max_excl + j] >= a2; j++)
                        if (E[a1 * max_excl + j] == a2) include = false;
                    if (!include) continue;
                    const float r = DS[i], inv_r = 1 / r, ar = a * r, pre = k * inv_r, er = std::erfc(ar);
                    const float dedr = pre * Q[a1] * Q[a2] * (er + ar * std::exp(-ar * ar) * two_over_sqrt_pi) * inv_r * inv_r;
                    for (int c = 0; c < 3; c++)
                        for (int d = 0; d < 3; d++) acc[3 * c + d] += (double)sh[c] * (double)(dedr * DL[3 * i + d]);
                }
                float* GB = grad_box.data_ptr<float>();
                for (int c = 0; c < 9; c++) GB[c] = (float)acc[c];
            }
        }
        ctx->save_for_backward({f.pos_deriv, f.charge_deriv, grad_box});
        return f.energy;
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
        TORCH_CHECK(!torch::GradMode::is_enabled(),
                    "pme_direct_box: second derivatives are not implemented (backward was called with create_graph=True)");
        const auto saved = ctx->get_saved_variables();
        return {saved[0] * grad_outputs[0], saved[1] * grad_outputs[0], Tensor(), Tensor(), Tensor(), Tensor(),
                saved[2].defined() ? saved[2] * grad_outputs[0] : Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

// ---------------------------------------------------------------------------------------------
// pme_direct_twice: pme_direct's forward and first-order backward (PmeDirectFunction::run, the same kernels and bits), recorded so that
// the backward pass is itself differentiable with respect to positions and charges (force matching).  As with the
// pair list: the backward is a Function (PmeDirectBackwardFunction: g -> g P, g C) whose own backward is the double backward
// (PmeDirectDoubleBackwardFunction: pme_second_order.hip on the device, plain loops on the host); a third derivative raises.
// pme_direct and pme_direct_box keep their refusal of create_graph=True: this op is the opt-in.
// ---------------------------------------------------------------------------------------------
// transposed index (pairs_index.hip) of a [2, pairs] int32 list whose unused entries have been replaced by num_atoms
Tensor pme_build_pair_index(const Tensor& nb, int64_t n) {
    const int64_t pairs = nb.size(1);
    Tensor index = torch::empty({nnpops_neighbor_pairs_index_ints((int)n, pairs)}, nb.options());
    Tensor iws = torch::empty({nnpops_neighbor_pairs_index_workspace_bytes((int)n, pairs) / 8 + 1}, nb.options().dtype(torch::kInt64));
    if (nnpops_neighbor_pairs_build_index((int)n, pairs, nb.data_ptr<int32_t>(), index.data_ptr<int32_t>(), iws.data_ptr(),
                                          current_stream(nb.device())) != NNPOPS_OK)
        raise_last("pme::pme_direct_twice (double backward: the owner-computes gather needs the pair list's transposed index)");
    return index;
}

class PmeDirectDoubleBackwardFunction : public torch::autograd::Function<PmeDirectDoubleBackwardFunction> {
public:
    // (v, w: cotangents of g P and g C) -> d/dpositions, d/dcharges, d/dg of g (sum v . P + sum w C)
    static tensor_list forward(AutogradContext*, const Tensor& v_in, const Tensor& w_in, const Tensor& g, const Tensor& positions,
                               const Tensor& charges, const Tensor& pos_deriv, const Tensor& charge_deriv, const Tensor& nb, const Tensor& dl,
                               const Tensor& ds, const Tensor& ex, const std::optional<Tensor>& index_opt, double alpha, double coulomb) {
        const Tensor v = v_in.contiguous(), w = w_in.contiguous(), pos = positions.contiguous(), q = charges.contiguous();
        const int64_t n = pos.size(0), pairs = nb.size(1), max_excl = ex.size(1);
        const auto opts = pos.options();
        Tensor gx = torch::empty({n, 3}, opts), gq = torch::empty({n}, opts);
        const float a = (float)alpha, k = (float)coulomb;
        if (pos.is_cuda()) {
            c10::hip::HIPGuard guard(pos.device().index());
            Tensor index = index_opt.value_or(Tensor()), first_index;
            if (!index.defined()) {
                // a list of unknown origin: any order, -1 slots anywhere -- both sides through column segments (nnpops_hip.h)
                const Tensor clean = torch::where(nb < 0, torch::full({}, n, nb.options()), nb).contiguous();
                index = pme_build_pair_index(clean, n);
                first_index = pme_build_pair_index(clean.flip(0).contiguous(), n);
            }
            Tensor workspace = torch::empty({nnpops_pme_direct_double_backward_workspace_bytes(pairs, (int)n)}, opts.dtype(torch::kUInt8));
            if (nnpops_pme_direct_double_backward((int)n, pairs, (int)max_excl, pos.data_ptr<float>(), q.data_ptr<float>(), nb.data_ptr<int32_t>(),
                                                  dl.data_ptr<float>(), ds.data_ptr<float>(), max_excl ? ex.data_ptr<int32_t>() : nullptr,
                                                  index.data_ptr<int32_t>(), first_index.defined() ? first_index.data_ptr<int32_t>() : nullptr,
                                                  v.data_ptr<float>(), w.data_ptr<float>(), a, k, gx.data_ptr<float>(), gq.data_ptr<float>(),
                                                  workspace.data_ptr(), current_stream(pos.device())) != NNPOPS_OK)
                raise_last("pme::pme_direct_twice (double backward)");
        } else {
            // the device pass's expressions per pair, double sums per atom
            const float* P = pos.data_ptr<float>(); const float* Q = q.data_ptr<float>();
            const float* V = v.data_ptr<float>(); const float* W = w.data_ptr<float>();
            const int32_t* N0 = nb.data_ptr<int32_t>(); const int32_t* N1 = N0 + pairs; const int32_t* E = ex.data_ptr<int32_t>();
            const float* DL = dl.data_ptr<float>(); const float* DS = ds.data_ptr<float>();
            const float two_over_sqrt_pi = 1.12837916709551257390f;
            std::vector<double> ax(3 * n, 0.0), aq(n, 0.0);
            // one pair (i, j) with delta d, distance r and f, f', f'' of its kind
            auto pair = [&](int64_t i, int64_t j, const float* d, float r, float f, float fp, float fpp) {
                const float inv_r = 1 / r;
                float u[3], dv[3], s = 0;
                for (int c = 0; c < 3; c++) { u[c] = d[c] * inv_r; dv[c] = V[3 * i + c] - V[3 * j + c]; s += u[c] * dv[c]; }
                const float qq = Q[i] * Q[j], cw = W[i] * Q[j] + W[j] * Q[i];
                const float A = qq * (fpp - fp * inv_r) * s + cw * fp, Bv = qq * fp * inv_r;
                for (int c = 0; c < 3; c++) {
                    const float t = A * u[c] + Bv * dv[c];
                    ax[3 * i + c] += t; ax[3 * j + c] -= t;
                }
                aq[i] += Q[j] * fp * s + W[j] * f;
                aq[j] += Q[i] * fp * s + W[i] * f;
            };
            for (int64_t i = 0; i < pairs; i++) {
                const int a1 = N0[i], a2 = N1[i];
                bool include = a1 > -1 && a2 > -1;
                for (int64_t j = 0; include && j < max_excl && E[a1 * max_excl + j] >= a2; j++)
                    if (E[a1 * max_excl + j] == a2) include = false;
                if (!include) continue;
                const float r = DS[i], inv_r = 1 / r, ar = a * r, pre = k * inv_r, er = std::erfc(ar), ex_ = std::exp(-ar * ar) * two_over_sqrt_pi;
                pair(a1, a2, DL + 3 * i, r, pre * er, -pre * (er + ar * ex_) * inv_r, 2 * pre * (er + ar * ex_ + ar * ar * ar * ex_) * inv_r * inv_r);
            }
            for (int64_t a1 = 0; a1 < n; a1++)
                for (int64_t j = 0; j < max_excl && E[a1 * max_excl + j] > a1; j++) {
                    const int a2 = E[a1 * max_excl + j];
                    float d[3];
                    for (int c = 0; c < 3; c++) d[c] = P[3 * a1 + c] - P[3 * a2 + c];
                    const float r = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), inv_r = 1 / r, ar = a * r, pre = k * inv_r;
                    const float er = std::erf(ar), ex_ = std::exp(-ar * ar) * two_over_sqrt_pi;
                    pair(a1, a2, d, r, -pre * er, pre * (er - ar * ex_) * inv_r, 2 * pre * (ar * ex_ + ar * ar * ar * ex_ - er) * inv_r * inv_r);
                }
            float* GX = gx.data_ptr<float>(); float* GQ = gq.data_ptr<float>();
            for (int64_t i = 0; i < 3 * n; i++) GX[i] = (float)ax[i];
            for (int64_t i = 0; i < n; i++) GQ[i] = (float)aq[i];
        }
        return {gx * g, gq * g, ((v * pos_deriv).sum() + (w * charge_deriv).sum()).reshape(g.sizes())};
    }

    static tensor_list backward(AutogradContext*, tensor_list) {
        TORCH_CHECK(false, "pme_direct_twice: third derivatives are not implemented");
        return {};
    }
};

class PmeDirectBackwardFunction : public torch::autograd::Function<PmeDirectBackwardFunction> {
public:
    static tensor_list forward(AutogradContext* ctx, const Tensor& g, const Tensor& positions, const Tensor& charges, const Tensor& pos_deriv,
                               const Tensor& charge_deriv, const Tensor& nb, const Tensor& dl, const Tensor& ds, const Tensor& ex,
                               const std::optional<Tensor>& index_opt, double alpha, double coulomb) {
        ctx->save_for_backward({g, positions, charges, pos_deriv, charge_deriv, nb, dl, ds, ex, index_opt.value_or(Tensor())});
        ctx->saved_data["alpha"] = alpha;
        ctx->saved_data["coulomb"] = coulomb;
        return {pos_deriv * g, charge_deriv * g};
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
        const auto s = ctx->get_saved_variables();
        const tensor_list d = PmeDirectDoubleBackwardFunction::apply(grads[0], grads[1], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], opt(s[9]),
                                                                     ctx->saved_data["alpha"].toDouble(), ctx->saved_data["coulomb"].toDouble());
        return {d[2], d[0], d[1], Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

class PmeDirectTwiceFunction : public torch::autograd::Function<PmeDirectTwiceFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& positions, const Tensor& charges, const Tensor& neighbors,
                          const Tensor& deltas, const Tensor& distances, const Tensor& exclusions, const torch::Scalar& alpha,
                          const torch::Scalar& coulomb) {
        const PmeDirectForward f = PmeDirectFunction::run(positions, charges, neighbors, deltas, distances, exclusions, alpha, coulomb);
        // (the index the forward pass found in the cache travels with the saved tensors: a later getNeighborPairs call replaces the cache)
        ctx->save_for_backward({positions, charges, f.pos_deriv, f.charge_deriv, f.nb, f.dl, f.ds, f.ex, f.index});
        ctx->saved_data["alpha"] = alpha.toDouble();
        ctx->saved_data["coulomb"] = coulomb.toDouble();
        return f.energy;
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
        const auto s = ctx->get_saved_variables();
        const tensor_list d = PmeDirectBackwardFunction::apply(grad_outputs[0], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], opt(s[8]),
                                                               ctx->saved_data["alpha"].toDouble(), ctx->saved_data["coulomb"].toDouble());
        return {d[0], d[1], Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

// =============================================================================================
// PME, reciprocal-space part (reference src/pytorch/pme/pme.cpp:5, pmeCUDA.cu:102-430, pmeCPU.cpp:174-364): same op name and
// schema.  Device: spread -> torch::fft::rfftn -> convolve (in place) -> [backward] irfftn(norm "forward") -> interpolate, the
// splines kept in the workspace between forward and backward, the box read on the device.  Host: plain loops + torch::fft on CPU.
// The energy is 0.5 sum_k; the self energy is the Python class's (as in the reference).
// =============================================================================================
namespace pme_recip_host {

struct Recip { float m[3][3]; };

Recip invert_box(const float* b) {
    Recip r{};
    const float scale = 1.0f / (b[0] * b[4] * b[8]);
    r.m[0][0] = b[4] * b[8] * scale;
    r.m[1][0] = -b[3] * b[8] * scale;
    r.m[1][1] = b[0] * b[8] * scale;
    r.m[2][0] = (b[3] * b[7] - b[4] * b[6]) * scale;
    r.m[2][1] = -b[0] * b[7] * scale;
    r.m[2][2] = b[0] * b[4] * scale;
    return r;
}

// base grid index, B-spline weights th[i][axis] and derivatives dth[i][axis] of one atom (order >= 2)
// (d2th, optional: the second derivatives d2th[i][axis] -- the order-(n-2) weights differenced twice, order >= 4)
void spline(const float* p_in, const float* b, const Recip& r, const int K[3], int order, int base[3], std::vector<float>& th,
            std::vector<float>& dth, std::vector<float>* d2th = nullptr) {
    float p[3] = {p_in[0], p_in[1], p_in[2]};
    for (int i = 2; i >= 0; i--) {
        const float s = std::floor(p[i] * r.m[i][i]);
        for (int j = 0; j < 3; j++) p[j] -= s * b[3 * i + j];
    }
    for (int i = 0; i < 3; i++) {
        float t = p[0] * r.m[0][i] + p[1] * r.m[1][i] + p[2] * r.m[2][i];
        t = (t - std::floor(t)) * K[i];
        const int ti = (int)t;
        const float dr = t - ti;
        base[i] = std::min(std::max(ti % K[i], 0), K[i] - 1);
        auto w = [&](int j) -> float& { return th[3 * j + i]; };
        w(order - 1) = 0;
        w(1) = dr;
        w(0) = 1 - dr;
        for (int j = 3; j < order; j++) {
            const float div = 1.0f / (j - 1);
            w(j - 1) = div * dr * w(j - 2);
            for (int k = 1; k < j - 1; k++) w(j - k - 1) = div * ((dr + k) * w(j - k - 2) + (j - k - dr) * w(j - k - 1));
            w(0) = div * (1 - dr) * w(0);
        }
        dth[i] = -w(0);
        for (int j = 1; j < order; j++) dth[3 * j + i] = w(j - 1) - w(j);
        const float scale = 1.0f / (order - 1);
        w(order - 1) = scale * dr * w(order - 2);
        for (int j = 1; j < order - 1; j++) w(order - j - 1) = scale * ((dr + j) * w(order - j - 2) + (order - j - dr) * w(order - j - 1));
        w(0) = scale * (1 - dr) * w(0);
        if (d2th) {
            std::vector<float> u(order + 2, 0.0f);       // order-(n-2) weights in u[0 .. n-3], zeros behind
            u[1] = dr;
            u[0] = 1 - dr;
            for (int j = 3; j <= order - 2; j++) {
                const float div = 1.0f / (j - 1);
                u[j - 1] = div * dr * u[j - 2];
                for (int k = 1; k < j - 1; k++) u[j - k - 1] = div * ((dr + k) * u[j - k - 2] + (j - k - dr) * u[j - k - 1]);
                u[0] = div * (1 - dr) * u[0];
            }
            for (int j = 0; j < order; j++) (*d2th)[3 * j + i] = (j >= 2 ? u[j - 2] : 0.0f) - 2.0f * (j >= 1 ? u[j - 1] : 0.0f) + u[j];
        }
    }
}

// the complex grid times the Ewald kernel, in place: the float expressions of pme_reciprocal's host loop, without its sums
void convolve(c10::complex<float>* C, const int64_t K[3], const float* B, const Recip& r, double alpha, const float* XM, const float* YM,
              const float* ZM) {
    const int64_t zsize = K[2] / 2 + 1;
    const float scale_factor = (float)(M_PI * B[0] * B[4] * B[8]);
    const float exp_factor = (float)(M_PI * M_PI / (alpha * alpha));
    for (int64_t kx = 0; kx < K[0]; kx++) {
        const int64_t mx = kx < (K[0] + 1) / 2 ? kx : kx - K[0];
        for (int64_t ky = 0; ky < K[1]; ky++) {
            const int64_t my = ky < (K[1] + 1) / 2 ? ky : ky - K[1];
            for (int64_t kz = 0; kz < zsize; kz++) {
                const int64_t mz = kz < (K[2] + 1) / 2 ? kz : kz - K[2];
                const int64_t idx = (kx * K[1] + ky) * zsize + kz;
                const float mhx = mx * r.m[0][0], mhy = mx * r.m[1][0] + my * r.m[1][1];
                const float mhz = mx * r.m[2][0] + my * r.m[2][1] + mz * r.m[2][2];
                const float m2 = mhx * mhx + mhy * mhy + mhz * mhz;
                const float denom = m2 * (scale_factor * XM[kx]) * YM[ky] * ZM[kz];
                C[idx] *= idx == 0 ? 0.f : std::exp(-exp_factor * m2) / denom;
            }
        }
    }
}

// dE/dB = - B^-T (Pi + X): pi = the six sums of the convolution loop (without their 1/2), X = sum_j x_j (x) g_j; as
// pme_recip_box_finish, in double with the general 3 x 3 inverse
void box_gradient(int64_t n, const float* pos, const float* pos_deriv, const double* pi, const float* box, float* grad_box) {
    double X[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t j = 0; j < n; j++)
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) X[3 * a + b] += (double)pos[3 * j + a] * (double)pos_deriv[3 * j + b];
    const double M[9] = {0.5 * pi[0] + X[0], 0.5 * pi[3] + X[1], 0.5 * pi[4] + X[2], 0.5 * pi[3] + X[3], 0.5 * pi[1] + X[4],
                         0.5 * pi[5] + X[5], 0.5 * pi[4] + X[6], 0.5 * pi[5] + X[7], 0.5 * pi[2] + X[8]};
    double B[9];
    for (int c = 0; c < 9; c++) B[c] = box[c];
    const double c00 = B[4] * B[8] - B[5] * B[7], c01 = B[5] * B[6] - B[3] * B[8], c02 = B[3] * B[7] - B[4] * B[6];
    const double det = B[0] * c00 + B[1] * c01 + B[2] * c02;
    const double inv[9] = {c00 / det, (B[2] * B[7] - B[1] * B[8]) / det, (B[1] * B[5] - B[2] * B[4]) / det,
                           c01 / det, (B[0] * B[8] - B[2] * B[6]) / det, (B[2] * B[3] - B[0] * B[5]) / det,
                           c02 / det, (B[1] * B[6] - B[0] * B[7]) / det, (B[0] * B[4] - B[1] * B[3]) / det};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) grad_box[3 * a + b] = (float)-(inv[a] * M[b] + inv[3 + a] * M[3 + b] + inv[6 + a] * M[6 + b]);
}

}  // namespace pme_recip_host

// the energy, what the backward passes need, and the inputs as the kernels read them
struct PmeRecipForward {
    Tensor energy, q, box, recip, workspace, pos, pi, xm, ym, zm;
    std::vector<int64_t> grid;
    int64_t order;
    double alpha, coulomb;
};

class PmeReciprocalFunction : public torch::autograd::Function<PmeReciprocalFunction> {
public:
    // the forward pass on either key, shared with pme_reciprocal_twice
    static PmeRecipForward run(const Tensor& positions, const Tensor& charges, const Tensor& box_vectors,
                          const torch::Scalar& gridx, const torch::Scalar& gridy, const torch::Scalar& gridz, const torch::Scalar& order,
                          const torch::Scalar& alpha, const torch::Scalar& coulomb, const Tensor& xmoduli, const Tensor& ymoduli,
                          const Tensor& zmoduli, bool box_grad) {
        TORCH_CHECK(positions.dim() == 2 && positions.size(1) == 3, "positions must have shape (atoms, 3)");
        TORCH_CHECK(charges.dim() == 1 && charges.size(0) == positions.size(0), "charges must be 1D, one per atom");
        TORCH_CHECK(box_vectors.dim() == 2 && box_vectors.size(0) == 3 && box_vectors.size(1) == 3, "box_vectors must have shape (3, 3)");
        TORCH_CHECK(positions.scalar_type() == torch::kFloat32 && charges.scalar_type() == torch::kFloat32 &&
                    box_vectors.scalar_type() == torch::kFloat32, "pme_reciprocal computes in float32");
        const int64_t K[3] = {gridx.toLong(), gridy.toLong(), gridz.toLong()};
        TORCH_CHECK(K[0] >= 1 && K[1] >= 1 && K[2] >= 1, "pme_reciprocal: the grid dimensions must be positive");
        TORCH_CHECK(K[0] * K[1] * K[2] <= std::numeric_limits<int32_t>::max(), "pme_reciprocal: the grid is too large");
        const int64_t pme_order = order.toLong();
        TORCH_CHECK(pme_order >= 2, "pme_reciprocal: order must be at least 2");
        const double a = alpha.toDouble(), k = coulomb.toDouble();
        TORCH_CHECK(a > 0 && k > 0, "pme_reciprocal: alpha and coulomb must be positive");
        const Tensor* mods[3] = {&xmoduli, &ymoduli, &zmoduli};
        for (int i = 0; i < 3; i++)
            TORCH_CHECK(mods[i]->dim() == 1 && mods[i]->size(0) == K[i] && mods[i]->scalar_type() == torch::kFloat32,
                        "pme_reciprocal: the moduli must be float32 tensors of the grid's sizes");
        for (const Tensor* t : {&charges, &box_vectors, &xmoduli, &ymoduli, &zmoduli})
            TORCH_CHECK(t->device() == positions.device(), "pme_reciprocal: every tensor must be on the device of positions (",
                        positions.device(), "), got ", t->device());
        const Tensor pos = positions.contiguous(), q = charges.contiguous(), box = box_vectors.contiguous();
        const Tensor xm = xmoduli.contiguous(), ym = ymoduli.contiguous(), zm = zmoduli.contiguous();
        const int64_t n = positions.size(0);
        const auto opts = positions.options();
        // box_grad: the box gradient -B^-T (Pi + X) (pme_recip.hip): Pi is summed here, X in the backward from the position derivatives
        Tensor energy, recip, workspace, pi;
        if (positions.is_cuda()) {
            TORCH_CHECK(pme_order == 4 || pme_order == 5, "pme_reciprocal: Only pmeOrder 4 or 5 is supported on the device (got ", pme_order, ")");
            c10::hip::HIPGuard guard(positions.device().index());
            void* stream = current_stream(positions.device());
            const int gx = (int)K[0], gy = (int)K[1], gz = (int)K[2], o = (int)pme_order;
            workspace = torch::empty({nnpops_pme_reciprocal_workspace_bytes((int)n, gx, gy, gz, o)}, opts.dtype(torch::kUInt8));
            Tensor real = torch::empty({K[0], K[1], K[2]}, opts);
            if (nnpops_pme_reciprocal_spread((int)n, gx, gy, gz, o, pos.data_ptr<float>(), q.data_ptr<float>(), box.data_ptr<float>(), (float)k,
                                             real.data_ptr<float>(), workspace.data_ptr(), stream) != NNPOPS_OK)
                raise_last("pme::pme_reciprocal");
            recip = torch::fft::rfftn(real).contiguous();
            energy = torch::empty({}, opts);
            if (box_grad) {
                pi = torch::empty({nnpops_pme_reciprocal_box_workspace_bytes((int)n, gx, gy, gz, o)}, opts.dtype(torch::kUInt8));
                if (nnpops_pme_reciprocal_convolve_box((int)n, gx, gy, gz, o, box.data_ptr<float>(), (float)a, xm.data_ptr<float>(),
                                                       ym.data_ptr<float>(), zm.data_ptr<float>(), recip.data_ptr(), energy.data_ptr<float>(),
                                                       workspace.data_ptr(), pi.data_ptr(), stream) != NNPOPS_OK)
                    raise_last("pme::pme_reciprocal");
            } else if (nnpops_pme_reciprocal_convolve((int)n, gx, gy, gz, o, box.data_ptr<float>(), (float)a, xm.data_ptr<float>(), ym.data_ptr<float>(),
                                               zm.data_ptr<float>(), recip.data_ptr(), energy.data_ptr<float>(), workspace.data_ptr(),
                                               stream) != NNPOPS_OK)
                raise_last("pme::pme_reciprocal");
        } else {
            // host tensors: the reference registers a CPU kernel (pmeCPU.cpp:174-364); plain loops, double energy
            using namespace pme_recip_host;
            const float* B = box.data_ptr<float>();
            const Recip r = invert_box(B);
            const int Ki[3] = {(int)K[0], (int)K[1], (int)K[2]};
            const float sqrt_k = (float)std::sqrt(k);
            Tensor real = torch::zeros({K[0], K[1], K[2]}, opts);
            float* G = real.data_ptr<float>();
            const float* P = pos.data_ptr<float>(); const float* Q = q.data_ptr<float>();
            std::vector<float> th(3 * pme_order), dth(3 * pme_order);
            for (int64_t atom = 0; atom < n; atom++) {
                int b0[3];
                spline(P + 3 * atom, B, r, Ki, (int)pme_order, b0, th, dth);
                for (int ix = 0; ix < pme_order; ix++) {
                    const int64_t xi = (b0[0] + ix) % Ki[0];
                    const float dx = Q[atom] * sqrt_k * th[3 * ix];
                    for (int iy = 0; iy < pme_order; iy++) {
                        const int64_t yi = (b0[1] + iy) % Ki[1];
                        const float dxdy = dx * th[3 * iy + 1];
                        for (int iz = 0; iz < pme_order; iz++) G[(xi * K[1] + yi) * K[2] + (b0[2] + iz) % Ki[2]] += dxdy * th[3 * iz + 2];
                    }
                }
            }
            recip = torch::fft::rfftn(real).contiguous();
            auto* C = reinterpret_cast<c10::complex<float>*>(recip.data_ptr());
            const int64_t zsize = K[2] / 2 + 1;
            const float scale_factor = (float)(M_PI * B[0] * B[4] * B[8]);
            const float exp_factor = (float)(M_PI * M_PI / (a * a));
            const float* XM = xm.data_ptr<float>(); const float* YM = ym.data_ptr<float>(); const float* ZM = zm.data_ptr<float>();
            double e = 0.0, PS[6] = {0, 0, 0, 0, 0, 0};    // (Pi without its 1/2: xx, yy, zz, xy, xz, yz)
            for (int64_t kx = 0; kx < K[0]; kx++) {
                const int64_t mx = kx < (K[0] + 1) / 2 ? kx : kx - K[0];
                for (int64_t ky = 0; ky < K[1]; ky++) {
                    const int64_t my = ky < (K[1] + 1) / 2 ? ky : ky - K[1];
                    for (int64_t kz = 0; kz < zsize; kz++) {
                        const int64_t mz = kz < (K[2] + 1) / 2 ? kz : kz - K[2];
                        const int64_t idx = (kx * K[1] + ky) * zsize + kz;
                        const float mhx = mx * r.m[0][0], mhy = mx * r.m[1][0] + my * r.m[1][1];
                        const float mhz = mx * r.m[2][0] + my * r.m[2][1] + mz * r.m[2][2];
                        const float m2 = mhx * mhx + mhy * mhy + mhz * mhz;
                        const float denom = m2 * (scale_factor * XM[kx]) * YM[ky] * ZM[kz];
                        const float eterm = idx == 0 ? 0.f : std::exp(-exp_factor * m2) / denom;
                        const float w = (kz > 0 && kz <= (K[2] - 1) / 2) ? 2.f : 1.f;
                        const float term = w * eterm * std::norm(C[idx]);
                        e += term;
                        if (box_grad && idx != 0) {
                            const double t = term, c = 2.0 * ((double)exp_factor + 1.0 / (double)m2);
                            const double hx = mhx, hy = mhy, hz = mhz;
                            PS[0] += t * (1.0 - c * hx * hx); PS[1] += t * (1.0 - c * hy * hy); PS[2] += t * (1.0 - c * hz * hz);
                            PS[3] -= t * c * hx * hy;         PS[4] -= t * c * hx * hz;         PS[5] -= t * c * hy * hz;
                        }
                        C[idx] *= eterm;
                    }
                }
            }
            energy = torch::full({}, (float)(0.5 * e), opts);
            if (box_grad) pi = torch::tensor(std::vector<double>(PS, PS + 6), opts.dtype(torch::kFloat64));
        }
        return {energy, q, box, recip, workspace, pos, pi, xm, ym, zm, std::vector<int64_t>{K[0], K[1], K[2]}, pme_order, a, k};
    }

    static Tensor forward(AutogradContext* ctx, const Tensor& positions, const Tensor& charges, const Tensor& box_vectors,
                          const torch::Scalar& gridx, const torch::Scalar& gridy, const torch::Scalar& gridz, const torch::Scalar& order,
                          const torch::Scalar& alpha, const torch::Scalar& coulomb, const Tensor& xmoduli, const Tensor& ymoduli,
                          const Tensor& zmoduli, bool box_grad) {
        const PmeRecipForward f = run(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli, zmoduli, box_grad);
        // (the device path keeps the splines in the workspace and does not need the positions again, unless for the box gradient)
        const Tensor none = torch::empty({0}, positions.options());
        if (box_grad)
            ctx->save_for_backward({f.q, f.box, f.recip, f.workspace.defined() ? f.workspace : none, f.pos, f.pi});
        else
            ctx->save_for_backward({f.q, f.box, f.recip, f.workspace.defined() ? f.workspace : none, positions.is_cuda() ? none : f.pos});
        ctx->saved_data["grid"] = f.grid;
        ctx->saved_data["order"] = f.order;
        ctx->saved_data["coulomb"] = f.coulomb;
        return f.energy;
    }

    // dE/dpositions, dE/dcharges (unscaled) from the potential grid: the first-order backward on either key
    static void interpolate(const Tensor& grid, const Tensor& q, const Tensor& box, const Tensor& workspace, const Tensor& pos,
                            const std::vector<int64_t>& K, int64_t pme_order, double k, Tensor& pos_deriv, Tensor& charge_deriv) {
        const int64_t n = q.size(0);
        if (q.is_cuda()) {
            c10::hip::HIPGuard guard(q.device().index());
            if (nnpops_pme_reciprocal_interpolate((int)n, (int)K[0], (int)K[1], (int)K[2], (int)pme_order, q.data_ptr<float>(),
                                                  box.data_ptr<float>(), (float)k, grid.data_ptr<float>(), pos_deriv.data_ptr<float>(),
                                                  charge_deriv.data_ptr<float>(), workspace.data_ptr(), current_stream(q.device())) != NNPOPS_OK)
                raise_last("pme::pme_reciprocal");
        } else {
            using namespace pme_recip_host;
            const float* B = box.data_ptr<float>();
            const Recip r = invert_box(B);
            const int Ki[3] = {(int)K[0], (int)K[1], (int)K[2]};
            const float sqrt_k = (float)std::sqrt(k);
            const float* G = grid.data_ptr<float>(); const float* P = pos.data_ptr<float>(); const float* Q = q.data_ptr<float>();
            float* PD = pos_deriv.data_ptr<float>(); float* CD = charge_deriv.data_ptr<float>();
            std::vector<float> th(3 * pme_order), dth(3 * pme_order);
            for (int64_t atom = 0; atom < n; atom++) {
                int b0[3];
                spline(P + 3 * atom, B, r, Ki, (int)pme_order, b0, th, dth);
                float d[3] = {0, 0, 0}, dq = 0;
                for (int ix = 0; ix < pme_order; ix++) {
                    const int64_t xi = (b0[0] + ix) % Ki[0];
                    for (int iy = 0; iy < pme_order; iy++) {
                        const int64_t yi = (b0[1] + iy) % Ki[1];
                        for (int iz = 0; iz < pme_order; iz++) {
                            const float g = G[(xi * K[1] + yi) * K[2] + (b0[2] + iz) % Ki[2]];
                            const float tx = th[3 * ix], ty = th[3 * iy + 1], tz = th[3 * iz + 2];
                            d[0] += dth[3 * ix] * ty * tz * g;
                            d[1] += tx * dth[3 * iy + 1] * tz * g;
                            d[2] += tx * ty * dth[3 * iz + 2] * g;
                            dq += tx * ty * tz * g;
                        }
                    }
                }
                const float s = Q[atom] * sqrt_k;
                const float fx = d[0] * Ki[0], fy = d[1] * Ki[1], fz = d[2] * Ki[2];
                PD[3 * atom] = s * (fx * r.m[0][0]);
                PD[3 * atom + 1] = s * (fx * r.m[1][0] + fy * r.m[1][1]);
                PD[3 * atom + 2] = s * (fx * r.m[2][0] + fy * r.m[2][1] + fz * r.m[2][2]);
                CD[atom] = dq * sqrt_k;
            }
        }
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
        TORCH_CHECK(!torch::GradMode::is_enabled(),
                    "pme_reciprocal: second derivatives are not implemented (backward was called with create_graph=True)");
        const auto saved = ctx->get_saved_variables();
        const Tensor q = saved[0], box = saved[1], recip = saved[2], workspace = saved[3], pos = saved[4];
        const std::vector<int64_t> K = ctx->saved_data["grid"].toIntVector();
        const int64_t pme_order = ctx->saved_data["order"].toInt();
        const double k = ctx->saved_data["coulomb"].toDouble();
        const int64_t n = q.size(0);
        const Tensor grid = torch::fft::irfftn(recip, torch::IntArrayRef(K), c10::nullopt, "forward").contiguous();
        const auto opts = q.options();
        Tensor pos_deriv = torch::empty({n, 3}, opts), charge_deriv = torch::empty({n}, opts);
        interpolate(grid, q, box, workspace, pos, K, pme_order, k, pos_deriv, charge_deriv);
        Tensor grad_box;
        if (saved.size() > 5) {
            const Tensor pi = saved[5];
            grad_box = torch::empty({3, 3}, opts);
            if (q.is_cuda()) {
                c10::hip::HIPGuard guard(q.device().index());
                if (nnpops_pme_reciprocal_box_gradient((int)n, (int)K[0], (int)K[1], (int)K[2], (int)pme_order, pos.data_ptr<float>(),
                                                       box.data_ptr<float>(), pos_deriv.data_ptr<float>(), grad_box.data_ptr<float>(),
                                                       pi.data_ptr(), current_stream(q.device())) != NNPOPS_OK)
                    raise_last("pme::pme_reciprocal");
            } else {
                pme_recip_host::box_gradient(n, pos.data_ptr<float>(), pos_deriv.data_ptr<float>(), pi.data_ptr<double>(),
                                             box.data_ptr<float>(), grad_box.data_ptr<float>());
            }
            grad_box = grad_box * grad_outputs[0];
        }
        return {pos_deriv * grad_outputs[0], charge_deriv * grad_outputs[0], grad_box, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(),
                Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

// ---------------------------------------------------------------------------------------------
// pme_reciprocal_twice: pme_reciprocal's forward and first-order backward (PmeReciprocalFunction::run / ::interpolate, the same kernels
// and bits), recorded so that the backward pass is itself differentiable with respect to positions and charges.
//     PmeRecipBackwardFunction        g -> g P, g C; keeps the potential grid phi (the irfftn it needed anyway) for the next pass
//     PmeRecipDoubleBackwardFunction  (v, w) -> spread of Q' -> rfftn -> the existing convolution -> irfftn = phi' -> two-grid
//                                     interpolation (pme_recip.hip); plain loops on the host
// No box gradient (the default ops have it) and no third derivative: both raise.
// ---------------------------------------------------------------------------------------------
class PmeRecipDoubleBackwardFunction : public torch::autograd::Function<PmeRecipDoubleBackwardFunction> {
public:
    static tensor_list forward(AutogradContext*, const Tensor& v_in, const Tensor& w_in, const Tensor& g, const Tensor& positions,
                               const Tensor& charges, const Tensor& box, const Tensor& workspace, const Tensor& xm, const Tensor& ym,
                               const Tensor& zm, const Tensor& phi, const Tensor& pos_deriv, const Tensor& charge_deriv,
                               std::vector<int64_t> K, int64_t pme_order, double alpha, double k) {
        const Tensor v = v_in.contiguous(), w = w_in.contiguous(), pos = positions.contiguous(), q = charges.contiguous();
        const int64_t n = q.size(0);
        const auto opts = q.options();
        Tensor gx = torch::empty({n, 3}, opts), gq = torch::empty({n}, opts);
        if (q.is_cuda()) {
            c10::hip::HIPGuard guard(q.device().index());
            void* stream = current_stream(q.device());
            const int kx = (int)K[0], ky = (int)K[1], kz = (int)K[2], o = (int)pme_order;
            Tensor second = torch::empty({nnpops_pme_reciprocal_second_workspace_bytes((int)n, kx, ky, kz, o)}, opts.dtype(torch::kUInt8));
            Tensor real = torch::empty({K[0], K[1], K[2]}, opts);
            if (nnpops_pme_reciprocal_spread_directional((int)n, kx, ky, kz, o, pos.data_ptr<float>(), q.data_ptr<float>(), box.data_ptr<float>(),
                                                         (float)k, v.data_ptr<float>(), w.data_ptr<float>(), real.data_ptr<float>(),
                                                         workspace.data_ptr(), second.data_ptr(), stream) != NNPOPS_OK)
                raise_last("pme::pme_reciprocal_twice (double backward)");
            Tensor recip = torch::fft::rfftn(real).contiguous();
            Tensor unused = torch::empty({}, opts);
            if (nnpops_pme_reciprocal_convolve((int)n, kx, ky, kz, o, box.data_ptr<float>(), (float)alpha, xm.data_ptr<float>(), ym.data_ptr<float>(),
                                               zm.data_ptr<float>(), recip.data_ptr(), unused.data_ptr<float>(), workspace.data_ptr(),
                                               stream) != NNPOPS_OK)
                raise_last("pme::pme_reciprocal_twice (double backward)");
            // (the inverse transform in double, as for phi: PmeRecipBackwardFunction::backward)
            const Tensor phi2 = torch::fft::irfftn(recip.to(torch::kComplexDouble), torch::IntArrayRef(K), c10::nullopt, "forward")
                                    .to(torch::kFloat).contiguous();
            if (nnpops_pme_reciprocal_interpolate_second((int)n, kx, ky, kz, o, q.data_ptr<float>(), box.data_ptr<float>(), (float)k,
                                                         w.data_ptr<float>(), phi.data_ptr<float>(), phi2.data_ptr<float>(), gx.data_ptr<float>(),
                                                         gq.data_ptr<float>(), workspace.data_ptr(), second.data_ptr(), stream) != NNPOPS_OK)
                raise_last("pme::pme_reciprocal_twice (double backward)");
        } else {
            using namespace pme_recip_host;
            const float* B = box.data_ptr<float>();
            const Recip r = invert_box(B);
            const int Ki[3] = {(int)K[0], (int)K[1], (int)K[2]};
            const int64_t Kl[3] = {K[0], K[1], K[2]};
            const int od = (int)pme_order;
            const float sqrt_k = (float)std::sqrt(k);
            const float* P = pos.data_ptr<float>(); const float* Q = q.data_ptr<float>();
            const float* V = v.data_ptr<float>(); const float* W = w.data_ptr<float>();
            std::vector<float> th(3 * od), dth(3 * od), d2th(3 * od);
            // s_a = K_a (v . B^-1 column a): the direction in grid units
            auto direction = [&](int64_t atom, float (&s)[3]) {
                for (int a = 0; a < 3; a++) s[a] = Ki[a] * (V[3 * atom] * r.m[0][a] + V[3 * atom + 1] * r.m[1][a] + V[3 * atom + 2] * r.m[2][a]);
            };
            Tensor real = torch::zeros({K[0], K[1], K[2]}, opts);
            float* G2 = real.data_ptr<float>();
            for (int64_t atom = 0; atom < n; atom++) {
                int b0[3];
                float s[3];
                spline(P + 3 * atom, B, r, Ki, od, b0, th, dth);
                direction(atom, s);
                const float qs = Q[atom] * sqrt_k, ws = W[atom] * sqrt_k;
                for (int ix = 0; ix < od; ix++) {
                    const int64_t xi = (b0[0] + ix) % Ki[0];
                    const float ax = ws * th[3 * ix] + qs * s[0] * dth[3 * ix], qx = qs * th[3 * ix];
                    for (int iy = 0; iy < od; iy++) {
                        const int64_t yi = (b0[1] + iy) % Ki[1];
                        const float ty = th[3 * iy + 1], dy = s[1] * dth[3 * iy + 1];
                        for (int iz = 0; iz < od; iz++) {
                            const float tz = th[3 * iz + 2], dz = s[2] * dth[3 * iz + 2];
                            G2[(xi * K[1] + yi) * K[2] + (b0[2] + iz) % Ki[2]] += ax * ty * tz + qx * (dy * tz + ty * dz);
                        }
                    }
                }
            }
            Tensor recip = torch::fft::rfftn(real).contiguous();
            convolve(reinterpret_cast<c10::complex<float>*>(recip.data_ptr()), Kl, B, r, alpha, xm.data_ptr<float>(), ym.data_ptr<float>(),
                     zm.data_ptr<float>());
            const Tensor phi2 = torch::fft::irfftn(recip, torch::IntArrayRef(K), c10::nullopt, "forward").contiguous();
            const float* G = phi.data_ptr<float>(); const float* H = phi2.data_ptr<float>();
            float* GX = gx.data_ptr<float>(); float* GQ = gq.data_ptr<float>();
            for (int64_t atom = 0; atom < n; atom++) {
                int b0[3];
                float s[3];
                spline(P + 3 * atom, B, r, Ki, od, b0, th, dth, &d2th);
                direction(atom, s);
                double h[3] = {0, 0, 0}, hh[6] = {0, 0, 0, 0, 0, 0}, a2 = 0, g2[3] = {0, 0, 0};      // hh: xx, yy, zz, xy, xz, yz
                for (int ix = 0; ix < od; ix++) {
                    const int64_t xi = (b0[0] + ix) % Ki[0];
                    const double tx = th[3 * ix], dx = dth[3 * ix], cx = d2th[3 * ix];
                    for (int iy = 0; iy < od; iy++) {
                        const int64_t yi = (b0[1] + iy) % Ki[1];
                        const double ty = th[3 * iy + 1], dy = dth[3 * iy + 1], cy = d2th[3 * iy + 1];
                        for (int iz = 0; iz < od; iz++) {
                            const int64_t at = (xi * K[1] + yi) * K[2] + (b0[2] + iz) % Ki[2];
                            const double tz = th[3 * iz + 2], dz = dth[3 * iz + 2], cz = d2th[3 * iz + 2];
                            const double f = G[at], f2 = H[at];
                            h[0] += dx * ty * tz * f; h[1] += tx * dy * tz * f; h[2] += tx * ty * dz * f;
                            hh[0] += cx * ty * tz * f; hh[1] += tx * cy * tz * f; hh[2] += tx * ty * cz * f;
                            hh[3] += dx * dy * tz * f; hh[4] += dx * ty * dz * f; hh[5] += tx * dy * dz * f;
                            a2 += tx * ty * tz * f2;
                            g2[0] += dx * ty * tz * f2; g2[1] += tx * dy * tz * f2; g2[2] += tx * ty * dz * f2;
                        }
                    }
                }
                const double qs = (double)Q[atom] * sqrt_k, ws = (double)W[atom] * sqrt_k;
                GQ[atom] = (float)(sqrt_k * (a2 + s[0] * h[0] + s[1] * h[1] + s[2] * h[2]));
                const double fx = (qs * (g2[0] + s[0] * hh[0] + s[1] * hh[3] + s[2] * hh[4]) + ws * h[0]) * Ki[0];
                const double fy = (qs * (g2[1] + s[0] * hh[3] + s[1] * hh[1] + s[2] * hh[5]) + ws * h[1]) * Ki[1];
                const double fz = (qs * (g2[2] + s[0] * hh[4] + s[1] * hh[5] + s[2] * hh[2]) + ws * h[2]) * Ki[2];
                GX[3 * atom] = (float)(fx * r.m[0][0]);
                GX[3 * atom + 1] = (float)(fx * r.m[1][0] + fy * r.m[1][1]);
                GX[3 * atom + 2] = (float)(fx * r.m[2][0] + fy * r.m[2][1] + fz * r.m[2][2]);
            }
        }
        return {gx * g, gq * g, ((v * pos_deriv).sum() + (w * charge_deriv).sum()).reshape(g.sizes())};
    }

    static tensor_list backward(AutogradContext*, tensor_list) {
        TORCH_CHECK(false, "pme_reciprocal_twice: third derivatives are not implemented");
        return {};
    }
};

class PmeRecipBackwardFunction : public torch::autograd::Function<PmeRecipBackwardFunction> {
public:
    static tensor_list forward(AutogradContext* ctx, const Tensor& g, const Tensor& positions, const Tensor& charges, const Tensor& box,
                               const Tensor& recip, const Tensor& workspace, const Tensor& xm, const Tensor& ym, const Tensor& zm,
                               std::vector<int64_t> K, int64_t pme_order, double alpha, double k) {
        const Tensor pos = positions.contiguous(), q = charges.contiguous();
        const int64_t n = q.size(0);
        const Tensor phi = torch::fft::irfftn(recip, torch::IntArrayRef(K), c10::nullopt, "forward").contiguous();
        Tensor pos_deriv = torch::empty({n, 3}, q.options()), charge_deriv = torch::empty({n}, q.options());
        PmeReciprocalFunction::interpolate(phi, q, box, workspace, pos, K, pme_order, k, pos_deriv, charge_deriv);
        ctx->save_for_backward({g, positions, charges, box, workspace, xm, ym, zm, phi, pos_deriv, charge_deriv, recip});
        ctx->saved_data["grid"] = K;
        ctx->saved_data["order"] = pme_order;
        ctx->saved_data["alpha"] = alpha;
        ctx->saved_data["coulomb"] = k;
        return {pos_deriv * g, charge_deriv * g};
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grads) {
        const auto s = ctx->get_saved_variables();
        // On the device the second-order interpolation reads a potential grid transformed back in double and rounded once: it
        // differences phi twice, and the float transform's error, white across the grid, grew there with the square of the grid size
        // (DESIGN.md s8b).  The first-order outputs keep the float transform and their bits.
        const std::vector<int64_t> K = ctx->saved_data["grid"].toIntVector();
        const Tensor phi = s[1].is_cuda() ? torch::fft::irfftn(s[11].to(torch::kComplexDouble), torch::IntArrayRef(K), c10::nullopt, "forward")
                                                .to(torch::kFloat).contiguous()
                                          : s[8];
        const tensor_list d = PmeRecipDoubleBackwardFunction::apply(grads[0], grads[1], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], phi, s[9], s[10],
                                                                    K, ctx->saved_data["order"].toInt(),
                                                                    ctx->saved_data["alpha"].toDouble(), ctx->saved_data["coulomb"].toDouble());
        return {d[2], d[0], d[1], Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

class PmeReciprocalTwiceFunction : public torch::autograd::Function<PmeReciprocalTwiceFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& positions, const Tensor& charges, const Tensor& box_vectors,
                          const torch::Scalar& gridx, const torch::Scalar& gridy, const torch::Scalar& gridz, const torch::Scalar& order,
                          const torch::Scalar& alpha, const torch::Scalar& coulomb, const Tensor& xmoduli, const Tensor& ymoduli,
                          const Tensor& zmoduli) {
        TORCH_CHECK(order.toLong() >= 4, "pme_reciprocal_twice: order must be at least 4 (below that the second derivatives of the B-spline "
                    "weights are not continuous), got ", order.toLong());
        const PmeRecipForward f = PmeReciprocalFunction::run(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli,
                                                             ymoduli, zmoduli, false);
        const Tensor none = torch::empty({0}, positions.options());
        ctx->save_for_backward({positions, charges, f.box, f.recip, f.workspace.defined() ? f.workspace : none, f.xm, f.ym, f.zm});
        ctx->saved_data["grid"] = f.grid;
        ctx->saved_data["order"] = f.order;
        ctx->saved_data["alpha"] = f.alpha;
        ctx->saved_data["coulomb"] = f.coulomb;
        return f.energy;
    }

    static tensor_list backward(AutogradContext* ctx, tensor_list grad_outputs) {
        const auto s = ctx->get_saved_variables();
        const tensor_list d = PmeRecipBackwardFunction::apply(grad_outputs[0], s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7],
                                                              ctx->saved_data["grid"].toIntVector(), ctx->saved_data["order"].toInt(),
                                                              ctx->saved_data["alpha"].toDouble(), ctx->saved_data["coulomb"].toDouble());
        return {d[0], d[1], Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

TORCH_LIBRARY(pme, m) {
    m.def("pme_direct(Tensor positions, Tensor charges, Tensor neighbors, Tensor deltas, Tensor distances, Tensor exclusions, "
          "Scalar alpha, Scalar coulomb) -> Tensor");
    m.def("pme_reciprocal(Tensor positions, Tensor charges, Tensor box_vectors, Scalar gridx, Scalar gridy, Scalar gridz, "
          "Scalar order, Scalar alpha, Scalar coulomb, Tensor xmoduli, Tensor ymoduli, Tensor zmoduli) -> Tensor");
    m.def("pme_direct_box(Tensor positions, Tensor charges, Tensor neighbors, Tensor deltas, Tensor distances, Tensor exclusions, "
          "Tensor box_vectors, Scalar alpha, Scalar coulomb) -> Tensor");
    // the twice-differentiable variants (force matching): the schemas of pme_direct and pme_reciprocal
    m.def("pme_direct_twice(Tensor positions, Tensor charges, Tensor neighbors, Tensor deltas, Tensor distances, Tensor exclusions, "
          "Scalar alpha, Scalar coulomb) -> Tensor");
    m.def("pme_reciprocal_twice(Tensor positions, Tensor charges, Tensor box_vectors, Scalar gridx, Scalar gridy, Scalar gridz, "
          "Scalar order, Scalar alpha, Scalar coulomb, Tensor xmoduli, Tensor ymoduli, Tensor zmoduli) -> Tensor");
}

Tensor pme_direct_box_entry(const Tensor& positions, const Tensor& charges, const Tensor& neighbors, const Tensor& deltas,
                            const Tensor& distances, const Tensor& exclusions, const Tensor& box_vectors, const torch::Scalar& alpha,
                            const torch::Scalar& coulomb) {
    const bool box_grad = torch::GradMode::is_enabled() && box_vectors.requires_grad();
    return PmeDirectBoxFunction::apply(positions, charges, neighbors, deltas, distances, exclusions, box_vectors, alpha, coulomb, box_grad);
}

Tensor pme_reciprocal_entry(const Tensor& positions, const Tensor& charges, const Tensor& box_vectors, const torch::Scalar& gridx,
                            const torch::Scalar& gridy, const torch::Scalar& gridz, const torch::Scalar& order, const torch::Scalar& alpha,
                            const torch::Scalar& coulomb, const Tensor& xmoduli, const Tensor& ymoduli, const Tensor& zmoduli) {
    // (decided here: inside forward() grad mode is off, and nothing is recorded under inference mode or no_grad)
    const bool box_grad = torch::GradMode::is_enabled() && box_vectors.requires_grad();
    return PmeReciprocalFunction::apply(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli,
                                        zmoduli, box_grad);
}

Tensor pme_direct_twice_entry(const Tensor& positions, const Tensor& charges, const Tensor& neighbors, const Tensor& deltas,
                              const Tensor& distances, const Tensor& exclusions, const torch::Scalar& alpha, const torch::Scalar& coulomb) {
    return PmeDirectTwiceFunction::apply(positions, charges, neighbors, deltas, distances, exclusions, alpha, coulomb);
}

Tensor pme_reciprocal_twice_entry(const Tensor& positions, const Tensor& charges, const Tensor& box_vectors, const torch::Scalar& gridx,
                                  const torch::Scalar& gridy, const torch::Scalar& gridz, const torch::Scalar& order,
                                  const torch::Scalar& alpha, const torch::Scalar& coulomb, const Tensor& xmoduli, const Tensor& ymoduli,
                                  const Tensor& zmoduli) {
    TORCH_CHECK(!(torch::GradMode::is_enabled() && box_vectors.requires_grad()),
                "pme_reciprocal_twice: box gradients need the default ops (pme_reciprocal; PME without twice_differentiable=True): the "
                "twice-differentiable ops return no box gradient");
    return PmeReciprocalTwiceFunction::apply(positions, charges, box_vectors, gridx, gridy, gridz, order, alpha, coulomb, xmoduli, ymoduli,
                                             zmoduli);
}

Tensor pme_direct_entry(const Tensor& positions, const Tensor& charges, const Tensor& neighbors, const Tensor& deltas,
                        const Tensor& distances, const Tensor& exclusions, const torch::Scalar& alpha, const torch::Scalar& coulomb) {
    return PmeDirectFunction::apply(positions, charges, neighbors, deltas, distances, exclusions, alpha, coulomb);
}

TORCH_LIBRARY_IMPL(pme, AutogradCUDA, m) {
    m.impl("pme_direct", pme_direct_entry);
    m.impl("pme_reciprocal", pme_reciprocal_entry);
    m.impl("pme_direct_box", pme_direct_box_entry);
    m.impl("pme_direct_twice", pme_direct_twice_entry);
    m.impl("pme_reciprocal_twice", pme_reciprocal_twice_entry);
}
TORCH_LIBRARY_IMPL(pme, AutogradCPU, m) {
    m.impl("pme_direct", pme_direct_entry);
    m.impl("pme_reciprocal", pme_reciprocal_entry);
    m.impl("pme_direct_box", pme_direct_box_entry);
    m.impl("pme_direct_twice", pme_direct_twice_entry);
    m.impl("pme_reciprocal_twice", pme_reciprocal_twice_entry);
}
// ... and the backend keys themselves (the reference registers its autograd Function under CPU, pmeCPU.cpp:381): below
// autograd -- torch.inference_mode(), AutoDispatchBelowAutograd -- the same entry runs without recording a graph
TORCH_LIBRARY_IMPL(pme, CUDA, m) {
    m.impl("pme_direct", pme_direct_entry);
    m.impl("pme_reciprocal", pme_reciprocal_entry);
    m.impl("pme_direct_box", pme_direct_box_entry);
    m.impl("pme_direct_twice", pme_direct_twice_entry);
    m.impl("pme_reciprocal_twice", pme_reciprocal_twice_entry);
}
TORCH_LIBRARY_IMPL(pme, CPU, m) {
    m.impl("pme_direct", pme_direct_entry);
    m.impl("pme_reciprocal", pme_reciprocal_entry);
    m.impl("pme_direct_box", pme_direct_box_entry);
    m.impl("pme_direct_twice", pme_direct_twice_entry);
    m.impl("pme_reciprocal_twice", pme_reciprocal_twice_entry);
}

// =============================================================================================
// BatchedLinear (reference src/pytorch/BatchedNN.cpp:30-50): y = W v + b broadcast over
// [molecules, atoms, models]; the backward skips the parameter gradients.
// =============================================================================================
class BatchedLinearFunction : public torch::autograd::Function<BatchedLinearFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& vectors, const Tensor& weights, const Tensor& biases) {
        ctx->save_for_backward({weights});
        return torch::matmul(weights, vectors) + biases;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const Tensor weights = ctx->get_saved_variables()[0];
        // dL/dv = W^T dL/dy, written as a row-vector product so no transpose is materialised
        const Tensor row = grads[0].squeeze(-1).unsqueeze(-2);
        return {torch::matmul(row, weights).squeeze(-2).unsqueeze(-1), Tensor(), Tensor()};
    }
};

Tensor BatchedLinear(const Tensor& vectors, const Tensor& weights, const Tensor& biases) {
    return BatchedLinearFunction::apply(vectors, weights, biases);
}

// =============================================================================================
// GroupedMLP: the atomic networks of one frame, atoms grouped by species, on the split-fp16 GEMM of the C ABI
// (nnpops_gemm_split, batched_nn.hip).  Same function as BatchedNN.py:100-122 of the reference -- Linear, CELU(0.1),
// Linear, CELU, Linear, CELU, Linear per atom and ensemble member -- with bias + CELU fused into the GEMM epilogues
// and CELU' into the epilogues / prologue of the input-gradient pass: six GEMM launches per species and step, no
// elementwise kernels in between.  Returns the per-atom energies (atoms' own order) summed over the ensemble members.
//   x          [atoms, F] fp32, atoms in their own order; order [atoms] int32: atoms grouped by kind (the layer-0 GEMM
//              reads its rows through it, the last backward GEMM writes through it)      group_sizes  atoms per kind
//   fwd_*      planes of the weights, per kind: [M*H1][Fp] | [M*H2][H1p] | [M*H3][H2p]   (p: rounded up to 32)
//   bwd_*      planes of their transposes, per kind: [F][(M*H1)p] | M x [H1][H2p] | M x [H2][H3p]
//   biases     per kind: [M*H1] | [M*H2] | [M*H3]           last_w per kind [M*H3], last_b per kind (summed over members)
// =============================================================================================
constexpr float kCeluAlpha = 0.1f;          // BatchedNN.py:103
constexpr float kOperandScale = 1.0f / 16;   // operands are split after this scale: |activation| up to 1e6 stays in fp16 range

inline int64_t up32(int64_t v) { return (v + 31) / 32 * 32; }

struct MlpLayout {
    int64_t F, M, H1, H2, H3;
    int64_t fwd_kind() const { return M * H1 * up32(F) + M * H2 * up32(H1) + M * H3 * up32(H2); }
    int64_t bwd_kind() const { return F * up32(M * H1) + M * H1 * up32(H2) + M * H2 * up32(H3); }
    int64_t bias_kind() const { return M * (H1 + H2 + H3); }
};

void gemm_checked(int rc) { TORCH_CHECK(rc == NNPOPS_OK, nnpops_last_error()); }

class GroupedMLPFunction : public torch::autograd::Function<GroupedMLPFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& order, std::vector<int64_t> group_sizes, int64_t num_models, int64_t h1,
                          int64_t h2, int64_t h3, const Tensor& fwd_hi, const Tensor& fwd_lo, const Tensor& bwd_hi,
                          const Tensor& bwd_lo, const Tensor& biases, const Tensor& last_w, std::vector<double> last_b_host) {
        require_device_tensor(x, "x");
        TORCH_CHECK(x.dim() == 2 && x.scalar_type() == torch::kFloat32 && x.is_contiguous(), "x must be a contiguous [atoms, features] float32 tensor");
        TORCH_CHECK(order.dim() == 1 && order.size(0) == x.size(0) && order.scalar_type() == torch::kInt32 && order.is_contiguous() && order.device() == x.device(),
                    "order must be an int32 permutation of the atoms on the same device");
        const MlpLayout L{x.size(1), num_models, h1, h2, h3};
        const int64_t kinds = (int64_t)group_sizes.size(), atoms = x.size(0);
        TORCH_CHECK(fwd_hi.numel() == kinds * L.fwd_kind() && bwd_hi.numel() == kinds * L.bwd_kind() &&
                    biases.numel() == kinds * L.bias_kind() && last_w.numel() == kinds * L.M * L.H3,
                    "GroupedMLP: packed parameter buffers do not match the layer widths");
        c10::hip::HIPGuard guard(x.device().index());
        void* stream = current_stream(x.device());
        const auto opts = x.options();
        Tensor y1 = torch::empty({atoms, L.M * L.H1}, opts), y2 = torch::empty({atoms, L.M * L.H2}, opts), y3 = torch::empty({atoms, L.M * L.H3}, opts);
        Tensor energies = torch::empty({atoms}, opts);
        const at::Half* fh = fwd_hi.data_ptr<at::Half>(); const at::Half* fl = fwd_lo.data_ptr<at::Half>();
        const float* bs = biases.data_ptr<float>();
        TORCH_CHECK((int64_t)last_b_host.size() == kinds, "GroupedMLP: one last-layer bias per kind");
        int64_t first = 0;
        for (int64_t k = 0; k < kinds; k++) {
            const int64_t n = group_sizes[k];
            if (n > 0) {
                const at::Half *h0 = fh + k * L.fwd_kind(), *l0 = fl + k * L.fwd_kind();
                const at::Half *h1p = h0 + L.M * L.H1 * up32(L.F), *l1p = l0 + L.M * L.H1 * up32(L.F);
                const at::Half *h2p = h1p + L.M * L.H2 * up32(L.H1), *l2p = l1p + L.M * L.H2 * up32(L.H1);
                const float* b0 = bs + k * L.bias_kind(); const float* b1 = b0 + L.M * L.H1; const float* b2 = b1 + L.M * L.H2;
                const int* rows = order.data_ptr<int>() + first;
                float* p1 = y1.data_ptr<float>() + first * L.M * L.H1;
                float* p2 = y2.data_ptr<float>() + first * L.M * L.H2;
                float* p3 = y3.data_ptr<float>() + first * L.M * L.H3;
                // layer 0: every member reads the same AEVs -> one GEMM, N = members * H1
                gemm_checked(nnpops_gemm_split(stream, n, L.M * L.H1, L.F, 1, x.data_ptr<float>(), L.F, 0, h0, l0, up32(L.F), 0, p1, L.M * L.H1, 0, 1, b0, 0,
                                               nullptr, 0, 0, 0, nullptr, 0, 0, nullptr, 0, kCeluAlpha, kOperandScale, rows, nullptr));
                // layers 2 and 4: one problem per member
                gemm_checked(nnpops_gemm_split(stream, n, L.H2, L.H1, L.M, p1, L.M * L.H1, L.H1, h1p, l1p, up32(L.H1), L.H2 * up32(L.H1), p2,
                                               L.M * L.H2, L.H2, 1, b1, L.H2, nullptr, 0, 0, 0, nullptr, 0, 0, nullptr, 0, kCeluAlpha, kOperandScale, nullptr, nullptr));
                gemm_checked(nnpops_gemm_split(stream, n, L.H3, L.H2, L.M, p2, L.M * L.H2, L.H2, h2p, l2p, up32(L.H2), L.H3 * up32(L.H2), p3,
                                               L.M * L.H3, L.H3, 1, b2, L.H3, nullptr, 0, 0, 0, nullptr, 0, 0, nullptr, 0, kCeluAlpha, kOperandScale, nullptr, nullptr));
                // layer 6: one output per member, summed over the members
                gemm_checked(nnpops_rows_dot(stream, n, L.M * L.H3, p3, L.M * L.H3, last_w.data_ptr<float>() + k * L.M * L.H3, last_b_host[k],
                                             energies.data_ptr<float>(), rows));
            }
            first += n;
        }
        TORCH_CHECK(first == atoms, "GroupedMLP: group sizes do not add up to the number of atoms");
        ctx->save_for_backward({y1, y2, y3, bwd_hi, bwd_lo, last_w, order});
        ctx->saved_data["group_sizes"] = group_sizes;
        ctx->saved_data["dims"] = std::vector<int64_t>{L.F, L.M, L.H1, L.H2, L.H3};
        return energies;
    }

    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const auto saved = ctx->get_saved_variables();
        const Tensor &y1 = saved[0], &y2 = saved[1], &y3 = saved[2], &bwd_hi = saved[3], &bwd_lo = saved[4], &last_w = saved[5], &order = saved[6];
        const std::vector<int64_t> group_sizes = ctx->saved_data["group_sizes"].toIntVector();
        const std::vector<int64_t> d = ctx->saved_data["dims"].toIntVector();
        const MlpLayout L{d[0], d[1], d[2], d[3], d[4]};
        const int64_t atoms = y1.size(0);
        c10::hip::HIPGuard guard(y1.device().index());
        void* stream = current_stream(y1.device());
        const auto opts = y1.options();
        Tensor d2 = torch::empty({atoms, L.M * L.H2}, opts), d1 = torch::empty({atoms, L.M * L.H1}, opts), dx = torch::empty({atoms, L.F}, opts);
        const at::Half* bh = bwd_hi.data_ptr<at::Half>(); const at::Half* bl = bwd_lo.data_ptr<at::Half>();
        int64_t first = 0;
        for (size_t k = 0; k < group_sizes.size(); k++) {
            const int64_t n = group_sizes[k];
            if (n > 0) {
                const at::Half *t0h = bh + k * L.bwd_kind(), *t0l = bl + k * L.bwd_kind();               // [F][(M*H1)p]
                const at::Half *t1h = t0h + L.F * up32(L.M * L.H1), *t1l = t0l + L.F * up32(L.M * L.H1);  // M x [H1][H2p]
                const at::Half *t2h = t1h + L.M * L.H1 * up32(L.H2), *t2l = t1l + L.M * L.H1 * up32(L.H2);  // M x [H2][H3p]
                const float* p1 = y1.data_ptr<float>() + first * L.M * L.H1;
                const float* p2 = y2.data_ptr<float>() + first * L.M * L.H2;
                const float* p3 = y3.data_ptr<float>() + first * L.M * L.H3;
                float* q2 = d2.data_ptr<float>() + first * L.M * L.H2;
                float* q1 = d1.data_ptr<float>() + first * L.M * L.H1;
                const float* w6 = last_w.data_ptr<float>() + k * L.M * L.H3;
                // dE/dy3 = w6 * CELU'(y3) is formed while it is staged (prologue); times W4, times CELU'(y2)
                gemm_checked(nnpops_gemm_split(stream, n, L.H2, L.H3, L.M, nullptr, 0, 0, t2h, t2l, up32(L.H3), L.H2 * up32(L.H3), q2, L.M * L.H2,
                                               L.H2, 2, nullptr, 0, p2, L.M * L.H2, L.H2, 1, p3, L.M * L.H3, L.H3, w6, L.H3, kCeluAlpha, kOperandScale, nullptr, nullptr));
                gemm_checked(nnpops_gemm_split(stream, n, L.H1, L.H2, L.M, q2, L.M * L.H2, L.H2, t1h, t1l, up32(L.H2), L.H1 * up32(L.H2), q1, L.M * L.H1,
                                               L.H1, 2, nullptr, 0, p1, L.M * L.H1, L.H1, 0, nullptr, 0, 0, nullptr, 0, kCeluAlpha, kOperandScale, nullptr, nullptr));
                // all members' first layers at once: K = members * H1
                gemm_checked(nnpops_gemm_split(stream, n, L.F, L.M * L.H1, 1, q1, L.M * L.H1, 0, t0h, t0l, up32(L.M * L.H1), 0,
                                               dx.data_ptr<float>(), L.F, 0, 0, nullptr, 0, nullptr, 0, 0, 0, nullptr, 0, 0, nullptr, 0,
                                               kCeluAlpha, kOperandScale, nullptr, order.data_ptr<int>() + first));
            }
            first += n;
        }
        Tensor gx = dx * grads[0].unsqueeze(1);             // upstream gradient of every atom's energy (atoms' own order)
        return {gx, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    }
};

Tensor GroupedMLP(const Tensor& x, const Tensor& order, std::vector<int64_t> group_sizes, int64_t num_models, int64_t h1, int64_t h2, int64_t h3,
                  const Tensor& fwd_hi, const Tensor& fwd_lo, const Tensor& bwd_hi, const Tensor& bwd_lo, const Tensor& biases,
                  const Tensor& last_w, std::vector<double> last_b) {
    return GroupedMLPFunction::apply(x, order, group_sizes, num_models, h1, h2, h3, fwd_hi, fwd_lo, bwd_hi, bwd_lo, biases, last_w, last_b);
}

// =============================================================================================
// FusedMLP: the atomic networks of one frame on mlp_fused.hip -- sum over atoms AND members of the networks' outputs
// (BatchedNN.py:100-111 up to the division by the number of members).  When x requires a gradient the input-gradient pass
// runs inside forward and backward is one multiplication (see EnergyFunction above).
// =============================================================================================
// how many gradient slots a node's backward returns: one for every argument of its forward behind the context
template <class R, class... Args>
constexpr size_t forward_arguments(R (*)(AutogradContext*, Args...)) { return sizeof...(Args); }

// The input gradient of a prepared frame, one launch of nnpops_mlp_input_grad into a fresh tensor: dx_scale times the plain sum
// over the members (the mean and total modes, FusedMLP's pass inside its forward), or -- with `upstream` [B, M], float32, contiguous --
// every (molecule, member) weighted by its upstream gradient (the member energies).
Tensor mlp_input_gradient(void* stream, MlpCall& call, const Tensor& x, float dx_scale, const Tensor* upstream, const c10::optional<Tensor>& offsets,
                          const char* op) {
    Tensor dx = torch::empty_like(x);
    mlp_point_gradient(call.frame, dx, dx_scale);
    if (upstream) mlp_point_upstream(call.frame, *upstream, offsets);
    if (nnpops_mlp_input_grad(stream, &call.frame) != NNPOPS_OK) raise_last(op);
    return dx;
}

class FusedMLPFunction : public torch::autograd::Function<FusedMLPFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths,
                          int64_t members, const Tensor& planes, const Tensor& floats, bool need_gradient, int64_t act_scale_log2) {
        const char* op = "NNPOpsBatchedNN::FusedMLP";
        c10::hip::HIPGuard guard(x.device().index());
        void* stream = current_stream(x.device());
        MlpCall call = mlp_prepare(x, rows, kind_atoms, widths, members, planes, floats, need_gradient, c10::nullopt, c10::nullopt, act_scale_log2);
        if (nnpops_mlp_forward(stream, &call.frame, need_gradient ? 1 : 0) != NNPOPS_OK) raise_last(op);
        Tensor total = torch::empty({1}, x.options());
        mlp_reduce(stream, call, members, nullptr, nullptr, MlpReduce::total, c10::nullopt, total, op);
        if (need_gradient) ctx->save_for_backward({mlp_input_gradient(stream, call, x, 1.0f, nullptr, c10::nullopt, op)});
        return total;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        TORCH_CHECK(!torch::GradMode::is_enabled(), "NNPOpsBatchedNN::FusedMLP: second derivatives are not implemented (create_graph=True); "
                                                    "use layout='grouped' for that");
        const auto saved = ctx->get_saved_variables();
        TORCH_CHECK(!saved.empty(), "FusedMLP was evaluated without a gradient request");
        tensor_list result(forward_arguments(&forward));
        result[0] = saved[0] * grads[0];                      // x
        return result;
    }
};

Tensor FusedMLP(const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                const Tensor& planes, const Tensor& floats, int64_t act_scale_log2) {
    const bool need = torch::GradMode::is_enabled() && x.requires_grad();
    return FusedMLPFunction::apply(x, rows, kind_atoms, widths, members, planes, floats, need, act_scale_log2);
}

// =============================================================================================
// FusedMLPMembers: the energy of every ensemble member as a differentiable output -- [B, M], B = 1 without the tables of a batch
// (offsets [B + 1], places [atoms]: nnpops_mlp_member_sums), float32, or float64 and shifted with `shift` (a float64 device scalar).
// forward: nnpops_mlp_forward (with its gradient half when x requires a gradient) + the member sums.  What the gradient half leaves
// (dE/dy1, or every member's share of dE/dx) belongs to the NODE -- not to a holder whose next step would overwrite it -- and waits
// for the upstream gradient: backward takes grad [B, M] and runs the WEIGHTED nnpops_mlp_input_grad (nnpops_hip.h: member_weights),
// one launch whatever the function of the member energies was.  No host synchronisation anywhere: the op can be captured.
// =============================================================================================
// What a members node keeps between its forward and its backward pass.  save() and load() are the only code that knows where a
// piece lies in the context.
struct MlpNodeState {
    Tensor x, rows, planes, floats, energies;
    std::vector<Tensor> workspace;    // what the forward's gradient half left: dx_partial alone, or dE/dy1 of every kind
    bool in_forward;                  // ... which of the two
    std::vector<int64_t> kind_atoms, widths;
    int64_t members, act_scale_log2;
    c10::optional<Tensor> x_blocks, dead_blocks, offsets;
    MlpReduce mode;                   // (the trainable node: what its output was, and the eight parameters' [out, in])
    std::vector<int64_t> parameter_shapes;
    c10::optional<Tensor> places;     // (the force-trainable node: the row places of a batch, and the parameters themselves -- the
    std::vector<Tensor> parameters;   //  inputs of its recorded backward)

    int64_t molecules() const { return offsets.has_value() ? offsets->numel() - 1 : 1; }

    void save(AutogradContext* ctx) const {
        tensor_list keep = {x, rows, planes, floats, energies};
        keep.insert(keep.end(), workspace.begin(), workspace.end());
        keep.insert(keep.end(), parameters.begin(), parameters.end());
        ctx->save_for_backward(keep);
        auto& d = ctx->saved_data;
        d["in_forward"] = in_forward; d["kind_atoms"] = kind_atoms; d["widths"] = widths; d["members"] = members;
        d["act_scale_log2"] = act_scale_log2; d["x_blocks"] = x_blocks; d["dead_blocks"] = dead_blocks; d["offsets"] = offsets;
        d["mean"] = (int64_t)mode; d["parameter_shapes"] = parameter_shapes;
        if (!parameters.empty()) { d["places"] = places; d["parameters"] = (int64_t)parameters.size(); }
    }
    static MlpNodeState load(AutogradContext* ctx, const char* name) {
        const auto saved = ctx->get_saved_variables();
        TORCH_CHECK(!saved.empty(), name, " was evaluated without a gradient request");
        auto& d = ctx->saved_data;
        const bool force = d.count("parameters") != 0;
        const auto behind = saved.end() - (force ? d["parameters"].toInt() : 0);
        return {saved[0], saved[1], saved[2], saved[3], saved[4], {saved.begin() + 5, behind}, d["in_forward"].toBool(),
                d["kind_atoms"].toIntVector(), d["widths"].toIntVector(), d["members"].toInt(), d["act_scale_log2"].toInt(),
                d["x_blocks"].toOptional<Tensor>(), d["dead_blocks"].toOptional<Tensor>(), d["offsets"].toOptional<Tensor>(),
                (MlpReduce)d["mean"].toInt(), d["parameter_shapes"].toIntVector(),
                force ? d["places"].toOptional<Tensor>() : c10::optional<Tensor>(), {behind, saved.end()}};
    }
};

// the frame of a node's backward pass: the forward's frame again, its workspaces handed back (nothing is allocated, nothing launched)
MlpCall prepare_backward(const MlpNodeState& s) {
    MlpScratch own;
    own.energies = s.energies;
    if (s.in_forward) own.partial = s.workspace[0];
    else own.d1 = s.workspace;
    return mlp_prepare(s.x, s.rows, s.kind_atoms, s.widths, s.members, s.planes, s.floats, true, s.x_blocks, s.dead_blocks, s.act_scale_log2, &own);
}

// the slots of a members node's gradients, in the order of the arguments of FusedMLPMembersFunction::forward; the trainable node's
// forward goes on with `mean` and the parameters (one slot each)
namespace mlp_slot { enum : size_t { x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets, places, shift,
                                     need_gradient, mean, parameters }; }

// The forward pass of the members nodes.  mode (mean and total: FusedMLPMeanTrainable only): the member energies [B, M]; the ensemble
// mean [B] of the one-node step (energy_step: the same launches on the same energies, hence its bits); the sum over atoms and members
// as FusedMLP returns it.  What is kept for the backward pass is the same.
Tensor mlp_members_forward(AutogradContext* ctx, const Tensor& x, const Tensor& rows, const std::vector<int64_t>& kind_atoms,
                           const std::vector<int64_t>& widths, int64_t members, const Tensor& planes, const Tensor& floats,
                           const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2,
                           const c10::optional<Tensor>& offsets, const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift,
                           bool need_gradient, MlpReduce mode, const std::vector<int64_t>& parameter_shapes, at::TensorList keep_parameters = {}) {
    const char* op = "NNPOpsBatchedNN::FusedMLPMembers";
    TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1, "FusedMLPMembers: an empty batch (x must be [atoms, features] with at least one atom)");
    TORCH_CHECK(offsets.has_value() == places.has_value(), "FusedMLPMembers: molecule offsets and row places come together");
    int64_t B = 1;
    if (offsets.has_value()) {
        for (const Tensor* t : {&*offsets, &*places})
            TORCH_CHECK(t->scalar_type() == torch::kInt32 && t->is_contiguous() && t->device() == x.device() && t->dim() == 1,
                        "FusedMLPMembers: molecule offsets and row places must be contiguous int32 vectors on the device of x");
        B = offsets->numel() - 1;
        TORCH_CHECK(B >= 1, "FusedMLPMembers: an empty batch (", offsets->numel(), " molecule offsets)");
        TORCH_CHECK(places->numel() == x.size(0), "FusedMLPMembers: ", x.size(0), " atoms need as many row places (got ", places->numel(), ")");
    }
    c10::hip::HIPGuard guard(x.device().index());
    void* stream = current_stream(x.device());
    MlpCall call = mlp_prepare(x, rows, kind_atoms, widths, members, planes, floats, need_gradient, x_blocks, dead_blocks, act_scale_log2);
    if (nnpops_mlp_forward(stream, &call.frame, need_gradient ? 1 : 0) != NNPOPS_OK) raise_last(op);
    check_shift(shift, x.device(), "FusedMLPMembers:", "x");
    const auto options = shift.has_value() ? x.options().dtype(torch::kFloat64) : x.options();
    Tensor out = mode == MlpReduce::members ? torch::empty({B, members}, options) : torch::empty({B}, options);
    mlp_reduce(stream, call, members, offsets.has_value() ? &*offsets : nullptr, places.has_value() ? &*places : nullptr, mode, shift, out, op);
    if (need_gradient)
        MlpNodeState{x, rows, planes, floats, call.energies, call.keep, call.frame.dx_partial != nullptr, kind_atoms, widths, members, act_scale_log2,
                     x_blocks, dead_blocks, offsets, mode, parameter_shapes, keep_parameters.empty() ? c10::optional<Tensor>() : places,
                     keep_parameters.vec()}.save(ctx);
    return out;
}

// the upstream gradient of the member energies as the weights of a gradient pass: [B, M], float32 or float64 -> float32, contiguous
Tensor mlp_member_upstream(const Tensor& grad, const MlpNodeState& s) {
    const int64_t B = s.molecules();
    TORCH_CHECK(grad.defined() && grad.dim() == 2 && grad.size(0) == B && grad.size(1) == s.members && grad.device() == s.x.device() &&
                (grad.scalar_type() == torch::kFloat32 || grad.scalar_type() == torch::kFloat64),
                "FusedMLPMembers: unexpected gradient of the member energies (shape [", B, ", ", s.members, "] in float32 or float64 expected)");
    return grad.to(torch::kFloat32).contiguous();
}

class FusedMLPMembersFunction : public torch::autograd::Function<FusedMLPMembersFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths,
                          int64_t members, const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks,
                          const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2, const c10::optional<Tensor>& offsets,
                          const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift, bool need_gradient) {
        return mlp_members_forward(ctx, x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets, places,
                                   shift, need_gradient, MlpReduce::members, {});
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        TORCH_CHECK(!torch::GradMode::is_enabled(), "NNPOpsBatchedNN::FusedMLPMembers: second derivatives are not implemented (create_graph=True); "
                                                    "use layout='grouped' for that");
        const MlpNodeState s = MlpNodeState::load(ctx, "FusedMLPMembers");
        const Tensor g = mlp_member_upstream(grads[0], s);
        c10::hip::HIPGuard guard(s.x.device().index());
        MlpCall call = prepare_backward(s);
        static_assert(forward_arguments(&forward) == mlp_slot::need_gradient + 1, "one gradient slot for every argument of forward");
        tensor_list result(forward_arguments(&forward));
        result[mlp_slot::x] = mlp_input_gradient(current_stream(s.x.device()), call, s.x, 1.0f, &g, s.offsets, "NNPOpsBatchedNN::FusedMLPMembers (backward)");
        return result;
    }
};

Tensor FusedMLPMembers(const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                       const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks, const c10::optional<Tensor>& dead_blocks,
                       int64_t act_scale_log2, const c10::optional<Tensor>& offsets, const c10::optional<Tensor>& places,
                       const c10::optional<Tensor>& shift) {
    const bool need = torch::GradMode::is_enabled() && x.requires_grad();
    return FusedMLPMembersFunction::apply(x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets, places,
                                          shift, need);
}

// =============================================================================================
// FusedMLPMembersTrainable: FusedMLPMembers with the networks' parameters as differentiable inputs -- `parameters`, the eight
// layer{0,2,4,6}_{weights,biases} tensors in the module's shapes [kinds, M, out, in] ([kinds, M, out, 1] for the biases), kind k of the
// module being kind k of the op.  The forward pass does not read them: it is FusedMLPMembers' forward on the packed planes, bit for
// bit, and the caller vouches that the planes were packed from these parameters (BatchedNN.py: _TrainableFusedNN).  The backward
// pass returns the gradient of x as FusedMLPMembers does and, from one call of nnpops_mlp_weight_grad with the upstream gradient of
// every (molecule, member) as its weights, the eight parameter gradients scattered into the module's shapes: entries outside a
// kind's packed widths and the columns of dead AEV blocks are exact zeros.  First derivatives only.
// =============================================================================================
// (how many times this process has asked for the first-order gradients, and for those of a directional derivative: WeightGradientCalls)
static std::atomic<int64_t> mlp_weight_gradient_calls[2];
// The gradients of the eight parameter arrays for `upstream` [B, M] (float32, contiguous), the weight of every (molecule, member):
// per-kind outputs at the packed widths, ONE call of nnpops_mlp_weight_grad, and the scatter into the module's shapes -- rows and
// columns up to the smaller of the packed width and the module's, the first layer's columns where the live blocks lie; the rest zeros.
// With `tangent` [atoms, width of x] (float32, contiguous) the gradients of the DIRECTIONAL DERIVATIVE of the networks along it instead
// (nnpops_mlp_weight_grad_tangent: what a loss on forces asks for), and into `tangent_energies`, when given, the unweighted
// <t_a, dE_m(a)/dx_a> [grouped atoms, M].
tensor_list mlp_weight_gradients(void* stream, MlpCall& call, const MlpNodeState& s, const Tensor& upstream, const char* op,
                                 const Tensor* tangent = nullptr, Tensor* tangent_energies = nullptr) {
    mlp_weight_gradient_calls[tangent ? 1 : 0]++;
    mlp_point_upstream(call.frame, upstream, s.offsets);
    const auto options = s.x.options();
    const std::vector<int64_t>& shapes = s.parameter_shapes;
    const int64_t F = call.frame.num_features, M = s.members, kinds = (int64_t)s.kind_atoms.size();
    nnpops_mlp_weight_grad_out wg{};
    const int64_t bytes = tangent ? nnpops_mlp_weight_grad_tangent_workspace_bytes(&call.frame) : nnpops_mlp_weight_grad_workspace_bytes(&call.frame);
    Tensor workspace = torch::empty({std::max<int64_t>(bytes / 4, 64)}, options);
    wg.workspace = workspace.data_ptr<float>(); wg.workspace_bytes = workspace.numel() * 4;
    std::vector<std::array<Tensor, 8>> packed((size_t)kinds);
    for (int64_t k = 0; k < kinds; k++) {
        const int64_t h1 = s.widths[3 * k], h2 = s.widths[3 * k + 1], h3 = s.widths[3 * k + 2];
        packed[k] = {torch::empty({M, h1, F}, options), torch::empty({M, h1, 1}, options), torch::empty({M, h2, h1}, options),
                     torch::empty({M, h2, 1}, options), torch::empty({M, h3, h2}, options), torch::empty({M, h3, 1}, options),
                     torch::empty({M, 1, h3}, options), torch::empty({M, 1, 1}, options)};
        nnpops_mlp_weight_grad_kind& o = wg.kinds[k];
        float** slots[8] = {&o.dw0, &o.db0, &o.dw2, &o.db2, &o.dw4, &o.db4, &o.dw6, &o.db6};
        for (int i = 0; i < 8; i++) *slots[i] = packed[k][i].data_ptr<float>();
    }
    if (tangent) {
        nnpops_mlp_weight_grad_tangent_out tg{};
        tg.t = tangent->data_ptr<float>(); tg.ldt = (int)tangent->size(1);
        tg.workspace = wg.workspace; tg.workspace_bytes = wg.workspace_bytes;
        tg.tangent_energies = tangent_energies ? tangent_energies->data_ptr<float>() : nullptr;
        for (int64_t k = 0; k < kinds; k++) tg.kinds[k] = wg.kinds[k];
        if (nnpops_mlp_weight_grad_tangent(stream, &call.frame, &tg) != NNPOPS_OK) raise_last(op);
    } else if (nnpops_mlp_weight_grad(stream, &call.frame, &wg) != NNPOPS_OK) raise_last(op);
    Tensor live_columns;
    if (call.frame.x_groups)
        live_columns = ((s.x_blocks->to(torch::kLong) * 16).unsqueeze(1) + torch::arange(16, s.x_blocks->options().dtype(torch::kLong)).unsqueeze(0)).reshape(-1);
    tensor_list gradients;
    for (int i = 0; i < 8; i++) {
        Tensor full = torch::zeros({kinds, M, shapes[2 * i], shapes[2 * i + 1]}, options);
        for (int64_t k = 0; k < kinds; k++) {
            const Tensor& src = packed[k][i];
            const int64_t r = std::min<int64_t>(src.size(1), shapes[2 * i]);
            if (i == 0 && live_columns.defined()) {
                full[k].narrow(1, 0, r).index_copy_(2, live_columns, src.narrow(1, 0, r));
                continue;
            }
            const int64_t c = std::min<int64_t>(src.size(2), shapes[2 * i + 1]);
            full[k].narrow(1, 0, r).narrow(2, 0, c).copy_(src.narrow(1, 0, r).narrow(2, 0, c));
        }
        gradients.push_back(full);
    }
    return gradients;
}

// The backward pass of the trainable nodes for the upstream gradient `grad` of their output: the slots of forward's arguments with the
// gradient of x in its place and -- with_weights -- the eight parameter gradients behind them.  weights_out: the weight of every
// (molecule, member) that `grad` amounts to, [B, M] (what a weight gradient of this node takes as member_weights).
tensor_list mlp_trainable_backward(const MlpNodeState& s, const Tensor& grad, bool with_weights, Tensor* weights_out, const char* op) {
    const int64_t B = s.molecules();
    c10::hip::HIPGuard guard(s.x.device().index());
    void* stream = current_stream(s.x.device());
    MlpCall call = prepare_backward(s);
    tensor_list result(mlp_slot::parameters);             // (... and one for every parameter of the list behind them)
    Tensor g;                                             // the weight of every (molecule, member) in the weight gradient
    if (s.mode == MlpReduce::members) {
        g = mlp_member_upstream(grad, s);
        result[mlp_slot::x] = mlp_input_gradient(stream, call, s.x, 1.0f, &g, s.offsets, op);
    } else {
        // the gradient of x as the one-node step forms it -- the unweighted pass with 1 / M as its scale -- then times the upstream
        // gradient of the row's molecule: with an upstream gradient of one, the bits energy_step hands to the AEV backward
        const float mean_scale = s.mode == MlpReduce::total ? 1.0f : 1.0f / (float)s.members;
        const Tensor up = grad.to(torch::kFloat32).contiguous();
        TORCH_CHECK(up.numel() == B && up.device() == s.x.device(), "FusedMLPMeanTrainable: unexpected gradient of the energies (", B, " expected)");
        g = (up.reshape({B, 1}) * mean_scale).expand({B, s.members}).contiguous();     // every member carries the upstream gradient over M
        Tensor dx = mlp_input_gradient(stream, call, s.x, mean_scale, nullptr, c10::nullopt, op);
        if (s.offsets.has_value()) {
            const Tensor counts = (s.offsets->slice(0, 1, B + 1) - s.offsets->slice(0, 0, B)).to(torch::kLong);
            dx.mul_(torch::repeat_interleave(up.reshape({B}), counts, 0, s.x.size(0)).unsqueeze(1));
        } else {
            dx.mul_(up.reshape({B}));
        }
        result[mlp_slot::x] = dx;
    }
    if (weights_out) *weights_out = g;
    if (with_weights)
        for (Tensor& gradient : mlp_weight_gradients(stream, call, s, g, op)) result.push_back(std::move(gradient));
    return result;
}

class FusedMLPMembersTrainableFunction : public torch::autograd::Function<FusedMLPMembersTrainableFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths,
                          int64_t members, const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks,
                          const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2, const c10::optional<Tensor>& offsets,
                          const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift, bool need_gradient, int64_t mean,
                          at::TensorList parameters) {
        const int64_t kinds = (int64_t)kind_atoms.size();
        TORCH_CHECK(parameters.size() == 8, "FusedMLPMembersTrainable: eight parameter tensors (layer{0,2,4,6}_{weights,biases}), got ", parameters.size());
        std::vector<int64_t> shapes;
        for (const Tensor& p : parameters) {
            TORCH_CHECK(p.dim() == 4 && p.size(0) == kinds && p.size(1) == members && p.device() == x.device() && p.scalar_type() == torch::kFloat32,
                        "FusedMLPMembersTrainable: parameters are float32 [kinds, members, out, in] tensors on the device of x");
            shapes.push_back(p.size(2)); shapes.push_back(p.size(3));
        }
        return mlp_members_forward(ctx, x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets, places,
                                   shift, need_gradient, (MlpReduce)mean, shapes);
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const char* op = "NNPOpsBatchedNN::FusedMLPMembersTrainable (backward)";
        TORCH_CHECK(!torch::GradMode::is_enabled(), "NNPOpsBatchedNN::FusedMLPMembersTrainable: second derivatives are not implemented (create_graph=True): "
                                                    "training on forces needs layout='grouped'");
        const MlpNodeState s = MlpNodeState::load(ctx, "FusedMLPMembersTrainable");
        static_assert(forward_arguments(&forward) == mlp_slot::parameters + 1, "one gradient slot for every argument of forward");
        return mlp_trainable_backward(s, grads[0], true, nullptr, op);
    }
};

// whether a trainable node has anything to keep: gradients are recorded and x or one of the parameters asks for one
bool needs_gradient(const Tensor& x, at::TensorList parameters) {
    bool need = x.requires_grad();
    for (const Tensor& p : parameters) need = need || p.requires_grad();
    return need && torch::GradMode::is_enabled();
}

Tensor FusedMLPMembersTrainable(const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                                const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks,
                                const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2, const c10::optional<Tensor>& offsets,
                                const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift, at::TensorList parameters) {
    return FusedMLPMembersTrainableFunction::apply(x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets,
                                                   places, shift, needs_gradient(x, parameters), (int64_t)MlpReduce::members, parameters);
}

// FusedMLPMeanTrainable: the same node with the ensemble mean [B] as its output -- the energy of the one-node step
// (NNPOpsANISymmetryFunctions::energy / energy_batch), bit for bit, and with an upstream gradient of one its gradient of x as well --
// differentiable in the parameters: the weight gradient runs with upstream / M for every member of the molecule.  total: the sum over
// atoms and members instead (scale 1, as FusedMLP returns it and differentiates it).
Tensor FusedMLPMeanTrainable(const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                             const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks,
                             const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2, const c10::optional<Tensor>& offsets,
                             const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift, at::TensorList parameters, bool total) {
    return FusedMLPMembersTrainableFunction::apply(x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets,
                                                   places, shift, needs_gradient(x, parameters), (int64_t)(total ? MlpReduce::total : MlpReduce::mean), parameters);
}

// =============================================================================================
// FusedMLPMembersForceTrainable / FusedMLPMeanForceTrainable: the trainable nodes for a loss on FORCES.  Forward and -- with grad mode
// off -- backward are the trainable nodes', bit for bit.  With grad mode on (create_graph=True) the backward pass is RECORDED, on the
// model of AevBackwardFunction: MlpBackwardFunction's forward makes the calls the plain backward makes (the same bits of dx; the eight
// first-order weight gradients only when the engine asks for them, so a force evaluation pays for none), and its own backward, given
// the cotangent t of dx (through the AEV node: the tangent J.v), returns
//   * the eight parameter gradients from ONE nnpops_mlp_weight_grad_tangent, the upstream gradient of every (molecule, member) as its
//     weights, scattered as mlp_weight_gradients scatters them;
//   * the gradient of the upstream tensor when that is asked for (a force of a function of the member energies whose weights depend
//     on the parameters, as the QBC factors do): <t_a, dE_m(a)/dx_a> summed per (molecule, member), times the mode's scale.
// Refused with a message, never dropped: the gradient of this node in x (the networks' Hessian in the AEV), a cotangent on one of the
// first-order weight gradients (weight-weight second derivatives) and a third derivative.
// =============================================================================================
namespace mlp_back { enum : size_t { upstream = 0, parameters = 1, x = 9, state = 10, with_weights = 11, count = 12 }; }

class MlpBackwardFunction : public torch::autograd::Function<MlpBackwardFunction> {
public:
    static tensor_list forward(AutogradContext* ctx, const Tensor& grad, at::TensorList parameters, const Tensor& x, const MlpNodeState& s,
                               bool with_weights) {
        const char* op = "NNPOpsBatchedNN::FusedMLPMembersForceTrainable (backward)";
        Tensor weights;
        tensor_list all = mlp_trainable_backward(s, grad, with_weights, &weights, op);      // (exactly the calls of the plain backward)
        tensor_list out = {all[mlp_slot::x]};
        out.insert(out.end(), all.begin() + mlp_slot::parameters, all.end());
        s.save(ctx);
        ctx->saved_data["upstream_weights"] = weights;
        ctx->saved_data["upstream_sizes"] = grad.sizes().vec();
        ctx->saved_data["upstream_double"] = grad.scalar_type() == torch::kFloat64;
        ctx->set_materialize_grads(false);                 // (an output nobody differentiates hands back an undefined cotangent, not zeros)
        return out;
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const char* op = "NNPOpsBatchedNN::FusedMLPMembersForceTrainable";
        TORCH_CHECK(!ctx->needs_input_grad(mlp_back::x), op, ": second derivatives with respect to the AEV are not implemented (the gradient "
                    "of a force with respect to the positions was asked for: a Hessian, or loss.backward() on a loss of forces, which also "
                    "differentiates in the positions).  The parameter gradient of a force loss is obtained with "
                    "torch.autograd.grad(loss, parameters) or loss.backward(inputs=parameters)");
        for (size_t i = 1; i < grads.size(); i++)
            TORCH_CHECK(!grads[i].defined(), op, ": second derivatives with respect to the parameters are not implemented (a gradient of the "
                        "networks' first-order weight gradients was asked for)");
        const Tensor& v = grads[0];
        TORCH_CHECK(!(torch::GradMode::is_enabled() && v.defined() && v.requires_grad()), op,
                    ": third derivatives are not implemented (the derivative of a force was taken with create_graph=True)");
        tensor_list out(mlp_back::count);                  // (one slot per argument, the parameter list taking eight)
        if (!v.defined()) return out;
        const MlpNodeState s = MlpNodeState::load(ctx, op);
        TORCH_CHECK(v.dim() == 2 && v.size(0) == s.x.size(0) && v.size(1) == s.x.size(1) && v.device() == s.x.device(), op,
                    ": unexpected cotangent of the AEV gradient");
        const Tensor t = v.to(torch::kFloat32).contiguous();
        const Tensor weights = ctx->saved_data["upstream_weights"].toTensor();
        c10::hip::HIPGuard guard(s.x.device().index());
        void* stream = current_stream(s.x.device());
        MlpCall call = prepare_backward(s);
        const bool want_upstream = ctx->needs_input_grad(mlp_back::upstream);
        Tensor edot;
        if (want_upstream) edot = torch::zeros({call.energies.size(0), s.members}, s.x.options());
        tensor_list gradients = mlp_weight_gradients(stream, call, s, weights, op, &t, want_upstream ? &edot : nullptr);
        for (size_t i = 0; i < 8; i++)
            if (ctx->needs_input_grad(mlp_back::parameters + i)) out[mlp_back::parameters + i] = gradients[i];
        if (want_upstream) {
            const int64_t B = s.molecules();
            Tensor sums = torch::empty({B, s.members}, s.x.options());
            if (nnpops_mlp_member_sums(stream, edot.data_ptr<float>(), (int)edot.size(0), (int)s.members,
                                       s.offsets.has_value() ? s.offsets->data_ptr<int32_t>() : nullptr, (int)B,
                                       s.places.has_value() ? s.places->data_ptr<int32_t>() : nullptr, sums.data_ptr<float>()) != NNPOPS_OK) raise_last(op);
            if (s.mode != MlpReduce::members) sums = sums.sum(1) * (s.mode == MlpReduce::total ? 1.0f : 1.0f / (float)s.members);
            if (ctx->saved_data["upstream_double"].toBool()) sums = sums.to(torch::kFloat64);
            out[mlp_back::upstream] = sums.reshape(ctx->saved_data["upstream_sizes"].toIntVector());
        }
        return out;
    }
};

class FusedMLPForceTrainableFunction : public torch::autograd::Function<FusedMLPForceTrainableFunction> {
public:
    static Tensor forward(AutogradContext* ctx, const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths,
                          int64_t members, const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks,
                          const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2, const c10::optional<Tensor>& offsets,
                          const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift, bool need_gradient, int64_t mean,
                          at::TensorList parameters) {
        const int64_t kinds = (int64_t)kind_atoms.size();
        TORCH_CHECK(parameters.size() == 8, "FusedMLPMembersForceTrainable: eight parameter tensors (layer{0,2,4,6}_{weights,biases}), got ", parameters.size());
        std::vector<int64_t> shapes;
        for (const Tensor& p : parameters) {
            TORCH_CHECK(p.dim() == 4 && p.size(0) == kinds && p.size(1) == members && p.device() == x.device() && p.scalar_type() == torch::kFloat32,
                        "FusedMLPMembersForceTrainable: parameters are float32 [kinds, members, out, in] tensors on the device of x");
            shapes.push_back(p.size(2)); shapes.push_back(p.size(3));
        }
        // (the node's edges count its tensor inputs only: x, rows, planes, floats, the optional tensors that are there, then the parameters)
        int64_t edge = 4;
        for (const c10::optional<Tensor>* t : {&x_blocks, &dead_blocks, &offsets, &places, &shift})
            if (t->has_value() && (*t)->defined()) edge++;
        ctx->saved_data["parameter_edge"] = edge;
        return mlp_members_forward(ctx, x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets, places,
                                   shift, need_gradient, (MlpReduce)mean, shapes, parameters);
    }
    static tensor_list backward(AutogradContext* ctx, const tensor_list& grads) {
        const char* op = "NNPOpsBatchedNN::FusedMLPMembersForceTrainable (backward)";
        const MlpNodeState s = MlpNodeState::load(ctx, "FusedMLPMembersForceTrainable");
        static_assert(forward_arguments(&forward) == mlp_slot::parameters + 1, "one gradient slot for every argument of forward");
        if (!torch::GradMode::is_enabled()) return mlp_trainable_backward(s, grads[0], true, nullptr, op);
        const size_t edge = (size_t)ctx->saved_data["parameter_edge"].toInt();
        bool with_weights = false;
        for (size_t i = 0; i < 8; i++) with_weights = with_weights || ctx->needs_input_grad(edge + i);
        // (the list goes in as a TensorList: a std::vector would be taken for a non-tensor argument and the node would have no edge to a parameter)
        const tensor_list recorded = MlpBackwardFunction::apply(grads[0], at::TensorList(s.parameters), s.x, s, with_weights);
        tensor_list result(mlp_slot::parameters);
        result[mlp_slot::x] = recorded[0];
        for (size_t i = 0; i < 8; i++) result.push_back(with_weights ? recorded[1 + i] : Tensor());
        return result;
    }
};

Tensor FusedMLPMembersForceTrainable(const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                                     const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks,
                                     const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2, const c10::optional<Tensor>& offsets,
                                     const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift, at::TensorList parameters) {
    return FusedMLPForceTrainableFunction::apply(x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets,
                                                 places, shift, needs_gradient(x, parameters), (int64_t)MlpReduce::members, parameters);
}

Tensor FusedMLPMeanForceTrainable(const Tensor& x, const Tensor& rows, std::vector<int64_t> kind_atoms, std::vector<int64_t> widths, int64_t members,
                                  const Tensor& planes, const Tensor& floats, const c10::optional<Tensor>& x_blocks,
                                  const c10::optional<Tensor>& dead_blocks, int64_t act_scale_log2, const c10::optional<Tensor>& offsets,
                                  const c10::optional<Tensor>& places, const c10::optional<Tensor>& shift, at::TensorList parameters, bool total) {
    return FusedMLPForceTrainableFunction::apply(x, rows, kind_atoms, widths, members, planes, floats, x_blocks, dead_blocks, act_scale_log2, offsets,
                                                 places, shift, needs_gradient(x, parameters), (int64_t)(total ? MlpReduce::total : MlpReduce::mean), parameters);
}

// [first-order weight gradients, weight gradients of a directional derivative] this process has launched through the nodes above
std::vector<int64_t> WeightGradientCalls() { return {mlp_weight_gradient_calls[0].load(), mlp_weight_gradient_calls[1].load()}; }

// =============================================================================================
// PackNetworks: the packed planes of FusedMLP* from the eight parameter arrays of a module ([kinds, M, out, in] / [kinds, M, out, 1],
// float32, contiguous, on one device) at the given packed widths, by nnpops_mlp_pack_networks: two launches on the current stream and
// no synchronisation.  -> (planes, floats, live_planes -- over the column blocks of x_blocks; an empty float32 tensor without them, as
// the module keeps it --, status: int32 [NNPOPS_MLP_PACK_STATUS_BYTES / 4], nnpops_hip.h).  FRESH tensors every call: a graph recorded
// on earlier planes keeps them.  Device tensors only, no autograd (the planes are not differentiable: FusedMLP*Trainable are).
// =============================================================================================
std::tuple<Tensor, Tensor, Tensor, Tensor> PackNetworks(at::TensorList parameters, std::vector<int64_t> widths, const c10::optional<Tensor>& x_blocks) {
    const char* op = "NNPOpsBatchedNN::PackNetworks";
    TORCH_CHECK(parameters.size() == 8, "PackNetworks: eight parameter tensors (layer{0,2,4,6}_{weights,biases}), got ", parameters.size());
    const Tensor& w0 = parameters[0];
    for (size_t i = 0; i < 8; i++) {
        const Tensor& p = parameters[i];
        TORCH_CHECK(p.is_cuda() && p.dim() == 4 && p.scalar_type() == torch::kFloat32 && p.is_contiguous() && p.device() == w0.device() &&
                    p.size(0) == w0.size(0) && p.size(1) == w0.size(1),
                    "PackNetworks: parameters are contiguous float32 [kinds, members, out, in] tensors on one device");
        if (i % 2)
            TORCH_CHECK(p.size(2) == parameters[i - 1].size(2) && p.size(3) == 1, "PackNetworks: biases are [kinds, members, out, 1]");
    }
    nnpops_mlp_networks nets{};
    TORCH_CHECK(w0.size(0) <= NNPOPS_MLP_MAX_KINDS && (int64_t)widths.size() == 3 * w0.size(0), "PackNetworks: at most ", NNPOPS_MLP_MAX_KINDS,
                " kinds, three widths each");
    auto dim = [&](int i, int d) { return (int)std::min<int64_t>(parameters[i].size(d), 1 << 30); };
    nets.num_kinds = dim(0, 0); nets.num_members = dim(0, 1); nets.num_features = dim(0, 3);
    nets.out0 = dim(0, 2); nets.out2 = dim(2, 2); nets.in2 = dim(2, 3); nets.out4 = dim(4, 2); nets.in4 = dim(4, 3); nets.out6 = dim(6, 2); nets.in6 = dim(6, 3);
    const float** slots[8] = {&nets.layer0_weights, &nets.layer0_biases, &nets.layer2_weights, &nets.layer2_biases,
                              &nets.layer4_weights, &nets.layer4_biases, &nets.layer6_weights, &nets.layer6_biases};
    for (int i = 0; i < 8; i++) *slots[i] = parameters[i].data_ptr<float>();
    for (size_t i = 0; i < widths.size(); i++) nets.widths[i] = (int)std::min<int64_t>(std::max<int64_t>(widths[i], -1), 1 << 30);
    const bool narrow = x_blocks.has_value() && x_blocks->numel() > 0;
    if (narrow) {
        TORCH_CHECK(x_blocks->scalar_type() == torch::kInt32 && x_blocks->is_contiguous() && x_blocks->device() == w0.device() && x_blocks->dim() == 1,
                    "PackNetworks: x_blocks must be a contiguous int32 vector on the device of the parameters");
        nets.live_blocks = x_blocks->data_ptr<int32_t>();
        nets.num_live_blocks = (int)std::min<int64_t>(x_blocks->numel(), 1 << 30);
    }
    const int64_t halves = nnpops_mlp_networks_plane_halves(&nets, 0);
    if (halves < 0) raise_last(op);
    const int64_t floats_n = nnpops_mlp_networks_floats(&nets), live_n = nnpops_mlp_networks_plane_halves(&nets, 1);
    if (floats_n < 0 || live_n < 0) raise_last(op);
    c10::hip::HIPGuard guard(w0.device().index());
    const auto f32 = w0.options().requires_grad(false);
    Tensor planes = torch::empty({halves}, f32.dtype(torch::kFloat16)), floats = torch::empty({floats_n}, f32);
    Tensor live = narrow ? torch::empty({live_n}, f32.dtype(torch::kFloat16)) : torch::empty({0}, f32);
    Tensor status = torch::empty({NNPOPS_MLP_PACK_STATUS_BYTES / 4}, f32.dtype(torch::kInt32));
    if (nnpops_mlp_pack_networks(current_stream(w0.device()), &nets, planes.data_ptr(), floats.data_ptr<float>(), narrow ? live.data_ptr() : nullptr,
                                 status.data_ptr()) != NNPOPS_OK) raise_last(op);
    return {planes, floats, live, status};
}

TORCH_LIBRARY(NNPOpsBatchedNN, m) {
    m.def("PackNetworks(Tensor[] parameters, int[] widths, Tensor? x_blocks) -> (Tensor planes, Tensor floats, Tensor live_planes, Tensor status)");
    m.def("BatchedLinear", BatchedLinear);
    m.def("FusedMLPMembersTrainable(Tensor x, Tensor rows, int[] kind_atoms, int[] widths, int members, Tensor planes, Tensor floats, Tensor? x_blocks, "
          "Tensor? dead_blocks, int act_scale_log2, Tensor? offsets, Tensor? places, Tensor? shift, Tensor[] parameters) -> Tensor",
          FusedMLPMembersTrainable);
    m.def("FusedMLPMeanTrainable(Tensor x, Tensor rows, int[] kind_atoms, int[] widths, int members, Tensor planes, Tensor floats, Tensor? x_blocks, "
          "Tensor? dead_blocks, int act_scale_log2, Tensor? offsets, Tensor? places, Tensor? shift, Tensor[] parameters, bool total=False) -> Tensor",
          FusedMLPMeanTrainable);
    m.def("FusedMLPMembersForceTrainable(Tensor x, Tensor rows, int[] kind_atoms, int[] widths, int members, Tensor planes, Tensor floats, Tensor? x_blocks, "
          "Tensor? dead_blocks, int act_scale_log2, Tensor? offsets, Tensor? places, Tensor? shift, Tensor[] parameters) -> Tensor",
          FusedMLPMembersForceTrainable);
    m.def("FusedMLPMeanForceTrainable(Tensor x, Tensor rows, int[] kind_atoms, int[] widths, int members, Tensor planes, Tensor floats, Tensor? x_blocks, "
          "Tensor? dead_blocks, int act_scale_log2, Tensor? offsets, Tensor? places, Tensor? shift, Tensor[] parameters, bool total=False) -> Tensor",
          FusedMLPMeanForceTrainable);
    m.def("WeightGradientCalls() -> int[]", WeightGradientCalls);
    m.def("FusedMLPMembers(Tensor x, Tensor rows, int[] kind_atoms, int[] widths, int members, Tensor planes, Tensor floats, Tensor? x_blocks=None, "
          "Tensor? dead_blocks=None, int act_scale_log2=4, Tensor? offsets=None, Tensor? places=None, Tensor? shift=None) -> Tensor", FusedMLPMembers);
    m.def("FusedMLP(Tensor x, Tensor rows, int[] kind_atoms, int[] widths, int members, Tensor planes, Tensor floats, int act_scale_log2=4) -> Tensor", FusedMLP);
    m.def("GroupedMLP(Tensor x, Tensor order, int[] group_sizes, int num_models, int h1, int h2, int h3, Tensor fwd_hi, Tensor fwd_lo, "
          "Tensor bwd_hi, Tensor bwd_lo, Tensor biases, Tensor last_w, float[] last_b) -> Tensor", GroupedMLP);
}

TORCH_LIBRARY_IMPL(NNPOpsBatchedNN, CUDA, m) { m.impl("PackNetworks", PackNetworks); }

}  // namespace
