// cfconv.hip -- SchNet continuous-filter convolution on gfx950 (C ABI: nnpops_cfconv_*).
//
// What is computed (reference src/schnet/CpuCFConv.cpp, maths in SURVEY.md App. A): for every pair
// (i, j) with r_ij < c
//     gamma_g = exp(-((r - mu_g)/sigma)^2 / 2),  mu_g = g*c/(G-1)                           ref :121-122, :151-154
//     y1 = act(W1 gamma + b1)      act = log((e^x + 1)/2)  or  tanh                          ref :158-166
//     y2 = fc(r) * (W2 y1 + b2)    fc = (cos(pi r/c) + 1)/2                                  ref :170-176
//     out[i] += y2 . x[j] ,  out[j] += y2 . x[i]           (elementwise over the W filters)  ref :180-183
// and the analytic derivatives with respect to x and to the positions                        ref :190-299
//
// How it is laid out for CDNA4 (new design; the reference CUDA code runs one warp per half pair and
// scatters 2W float atomics per pair):
//   * the neighbour build keeps a FULL list (rows of {dx, dy, dz, j} per atom, from the shared cell grid of
//     celllist.h or an all-pairs scan for small systems) and, behind it, a slot per PAIR that both ends know
//     (scan_half / half_slots).
//   * widths that are a multiple of 16 (16, 32, ... 128: every SchNet in use) evaluate the filter network ONCE
//     per pair on the MATRIX CORES -- 16 pair slots x W filters per tile, weights resident in LDS -- and spill the
//     filter row; an OWNER-COMPUTES gather (cfconv_gather: one wave per atom, lanes = channels) then accumulates
//     out[i] (backward: dE/dx[i], dE/dpos[i]) over the atom's full row.  No atomics, no scatter, deterministic.
//     The filters kernel is chosen once, when the convolution is created (ConvPath):
//       cfconv_filters_h2x2 / _h2b   W 32, 64, 96 with G + 1 <= 64, W 128 with G <= 55 (the W1 planes beside eight waves' tiles in
//                                    160 KiB): both layers as split-fp16 products (three v_mfma_f32_16x16x32_f16 in place of eight
//                                    fp32 ones), operands in registers
//       cfconv_filters_h2            the same widths with more Gaussians: layer 2 split, layer 1 on the fp32 instruction
//       cfconv_filters_mfma          W 16, 48, 80, 112, or weights outside the fp16 range: v_mfma_f32_16x16x4_f32 (exact fp32)
//   * other widths use the vector kernel: one wave per atom, lane = filter channel(s), pairs processed 8 at a
//     time so every weight read from LDS feeds 8 (x2 channels) FMAs; weights streamed through the caches
//     when they do not fit in LDS (W > 128).
// The kernels live in cfconv_build.h (neighbour rows, half list), cfconv_filters.h (the default filters kernels, the gather)
// and cfconv_fallback_kernels.h (the vector kernel, the fp32 matrix and LDS-plane filters kernels); this file holds the
// handles, the weight preparation, the choice of kernels and the C ABI.
// nnpops_cfconv_backprop_box adds dL/dbox of a periodic list behind the backward pass: one reduction over the wrapped pairs of what
// that pass leaves on the device (cfconv_box_grad.h).
// nnpops_cfconv_double_backward is the backward of the backward pass with respect to output_deriv, input and positions: one
// owner-computes pass over the full rows that keeps nothing between calls (cfconv_second_order.h).
// nnpops_cfconv_backprop_weights returns the gradients of the filter network's four weight arrays: one pass over the pair slots that
// writes a partial row per workgroup, and the float64 sum of the rows (cfconv_weight_grad.h); nnpops_cfconv_set_weights
// gives a live handle new weights through plan_and_upload, the planning and upload block it shares with nnpops_cfconv_create.
// nnpops_cfconv_double_backward_weights returns the gradients, in the same four arrays, of the scalar the double backward differentiates
// (the weight gradients of a force loss): a short pass over the rows for the pair scalar a, then the same partial rows and float64 sum
// (cfconv_weight_grad_second.h).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cfconv_box_grad.h"
#include "celllist_host.h"
#include "cfconv_build.h"
#include "cfconv_fallback_kernels.h"
#include "cfconv_filters.h"
#include "cfconv_second_order.h"
#include "cfconv_weight_grad.h"
#include "cfconv_weight_grad_second.h"

using namespace nnpops;

namespace {

constexpr int kMaxWidth = 512;      // <= 128: weights resident in LDS (matrix-core or vector kernels); above: streamed
constexpr int kMaxGauss = 256;

}  // namespace

// ---------------------------------------------------------------------------------------------
// handles
// ---------------------------------------------------------------------------------------------
struct nnpops_cfconv_neighbors {
    int N = 0;
    float cutoff = 0;
    bool periodic = false;
    int device = 0;
    hipStream_t stream = nullptr;
    int cap = 64;
    bool cells_disabled = false;
    bool built = false;
    float4* d_rows = nullptr;
    int* d_cnt = nullptr;
    int* d_status = nullptr;
    CellList cells;                 // cell grid (rows_cells reads sorted_cell with the slot's position)
    // half list behind the rows (scan_half / half_slots): built with the rows once a matrix-core convolution has
    // asked for it, on demand before that
    int *d_lo_cnt = nullptr, *d_half_off = nullptr, *d_pid = nullptr, *d_ids = nullptr;
    float* d_half_r = nullptr;
    int2* d_half_ij = nullptr;
    bool want_half = false, half_built = false;
    unsigned long long epoch = 0;      // number of the last build (process-wide counter): what a convolution keeps per list (its filter rows) is valid for one build
    bool cell_ordered = false;      // the last build went through the cell grid: cells.sorted_pos lists the atoms in cell order
    int2* d_segment = nullptr;      // [N] per-atom [lo, hi) of its molecule (batched lists only: nnpops_cfconv_neighbors_set_molecules)
    // periodic frames (nnpops_cfconv_neighbors_set_frames), all sized and uploaded there: the per-atom {lo, hi, frame, 0} of rows_frames
    // and the tables of the per-frame box pass (cfconv_box_grad.h): offsets [B + 1], one {frame, k} per workgroup, first_block [B + 1]
    int4* d_frame = nullptr;
    int* d_frame_offsets = nullptr;
    int2* d_frame_blocks = nullptr;
    int* d_frame_first = nullptr;
    int num_frames = 0, frame_blocks = 0;
    int pair_cap() const { return (int)std::min<size_t>((size_t)N * cap / 2, (size_t)INT32_MAX - 1); }
};

static int alloc_half(nnpops_cfconv_neighbors* h) {
    dev_free(h->d_pid); dev_free(h->d_half_r); dev_free(h->d_half_ij); dev_free(h->d_ids);
    h->d_ids = nullptr; h->d_pid = nullptr; h->d_half_r = nullptr; h->d_half_ij = nullptr;
    int rc;
    if ((rc = dev_alloc(&h->d_pid, (size_t)h->N * h->cap))) return rc;
    if ((rc = dev_alloc(&h->d_ids, (size_t)h->N * h->cap))) return rc;
    if ((rc = dev_alloc(&h->d_half_r, (size_t)h->pair_cap() + 1))) return rc;
    if ((rc = dev_alloc(&h->d_half_ij, (size_t)h->pair_cap() + 1))) return rc;
    if (hipMemset(h->d_half_r, 0, sizeof(float) * ((size_t)h->pair_cap() + 1)) != hipSuccess ||
        hipMemset(h->d_half_ij, 0, sizeof(int2) * ((size_t)h->pair_cap() + 1)) != hipSuccess ||
        hipMemset(h->d_pid, 0, sizeof(int) * (size_t)h->N * h->cap) != hipSuccess ||
        hipMemset(h->d_ids, 0, sizeof(int) * (size_t)h->N * h->cap) != hipSuccess)
        return fail(NNPOPS_ERR_HIP, "memset failed");
    return NNPOPS_OK;
}

// the two launches behind the rows that give every pair its slot
static int launch_half_build(nnpops_cfconv_neighbors* h, hipStream_t stream) {
    const float4* order = h->cell_ordered ? h->cells.sorted_pos : nullptr;
    hipLaunchKernelGGL(scan_half, dim3(1), dim3(1024), 0, stream, h->N, h->d_lo_cnt, h->d_half_off);
    hipLaunchKernelGGL(half_slots, dim3(h->N), dim3(64), 0, stream, h->d_rows, h->d_ids, h->d_cnt, h->d_half_off, h->cap, h->pair_cap(),
                       h->d_pid, h->d_half_r, h->d_half_ij, h->d_status, h->N, order);
    NNPOPS_HIP_TRY(hipGetLastError());
    h->half_built = true;
    return NNPOPS_OK;
}

namespace {
// Which kernels evaluate the filter network: decided once, by nnpops_cfconv_create, from the width, the number of Gaussians and
// the weights.  All but kVector run the half-list path (filters kernel + cfconv_gather).
enum class ConvPath {
    kVector,            // cfconv_kernel: W not a multiple of 16, W > 128, the matrix-core weights do not fit in LDS, or $NNPOPS_CFCONV_VALU=1
    kMatrix,            // cfconv_filters_mfma (fp32 matrix instruction): W in {16, 48, 80, 112}, or weights outside the fp16 range
    kSplitPlanes,       // cfconv_filters_h2 (layer 2 split-fp16, through LDS planes): W in {32, 64, 96, 128}, too many Gaussians for registers
    kSplitRegisters,    // cfconv_filters_h2x2 / _h2b (both layers split-fp16, register-fed): W in {32, 64, 96} with G <= 63, W = 128 with G <= 55
};

// ---------------------------------------------------------------------------------------------
// The plan of a convolution: which path, and the workgroup shape and dynamic LDS of its forward and backward launch.  Host arithmetic
// only -- nnpops_cfconv_create, the launches below, nnpops_cfconv_plan and nnpops_cfconv_describe all go through these helpers, so what
// the query reports is what is launched.
// ---------------------------------------------------------------------------------------------
// The environment switches, read by nnpops_cfconv_create and nnpops_cfconv_plan only.  Each forces a path that some shape or weights reach
// without it.
struct ConvSwitches {
    bool force_valu = false;        // $NNPOPS_CFCONV_VALU=1: keep the matrix cores out (A/B timing, debugging)
    int split_level = 2;            // $NNPOPS_CFCONV_SPLIT: 0 fp32 only, 1 second layer split, 2 both layers where possible
    bool reuse_filters = true;      // $NNPOPS_CFCONV_REUSE_FILTERS=0: a backward call always stores its filter rows
};

ConvSwitches read_switches() {
    ConvSwitches sw;
    if (const char* e = std::getenv("NNPOPS_CFCONV_VALU")) sw.force_valu = std::atoi(e) != 0;
    if (const char* e = std::getenv("NNPOPS_CFCONV_SPLIT")) sw.split_level = std::atoi(e);
    if (const char* e = std::getenv("NNPOPS_CFCONV_REUSE_FILTERS")) sw.reuse_filters = std::atoi(e) != 0;
    return sw;
}

// what create() and plan() refuse alike (create() has more to say about atoms, cutoff and device)
int check_layer(int width, int num_gaussians, float gaussian_width, int activation, const float* w1, const float* b1, const float* w2) {
    NNPOPS_REQUIRE(w1 && b1 && w2, "NULL weight pointer");
    NNPOPS_REQUIRE(activation == 0 || activation == 1, "Invalid value of \"activation\"");
    NNPOPS_REQUIRE(gaussian_width > 0, "gaussian_width must be positive");
    NNPOPS_REQUIRE(num_gaussians >= 2, "num_gaussians must be at least 2 (centres are spaced cutoff/(G-1))");
    if (width < 1 || width > kMaxWidth || num_gaussians > kMaxGauss)
        return fail(NNPOPS_ERR_UNSUPPORTED, "this build supports width in [1, %d] and up to %d Gaussians (got %d, %d)",
                    kMaxWidth, kMaxGauss, width, num_gaussians);
    return NNPOPS_OK;
}

// one launch: waves per workgroup (0: its tiles do not fit in LDS) and dynamic LDS bytes; the vector kernel's instantiation
struct LaunchShape {
    int waves = 0;
    size_t lds = 0;
    int cpl = 0;                    // vector kernel: channels per lane (1, 2, 4, 8)
    bool wlds = false;              // vector kernel: the weights sit in LDS (else they are streamed through the caches)
};

// The vector kernel of one direction: weights in LDS when they fit beside one wave's tiles (W <= 128 only), else streamed; as many waves
// per workgroup as fit next to the shared weights in 156 KiB.
LaunchShape vector_shape(int W, int G, bool bwd) {
    LaunchShape s;
    const size_t budget = 156 * 1024 / sizeof(float);
    const size_t per_wave = conv_wave_floats(W, G, bwd);
    s.wlds = conv_weight_floats(W, G) + per_wave <= budget && W <= 128;
    const int cpl = div_up(W, 64);
    s.cpl = s.wlds ? (W > 64 ? 2 : 1) : cpl <= 2 ? 2 : cpl <= 4 ? 4 : 8;
    const size_t wfl = s.wlds ? conv_weight_floats(W, G) : 0;
    if (wfl + per_wave > budget) return s;
    s.waves = (int)std::min<size_t>(kMaxWavesPerBlock, (budget - wfl) / per_wave);
    s.lds = (wfl + (size_t)s.waves * per_wave) * sizeof(float);
    return s;
}

// waves per workgroup of cfconv_filters_h2b: one per SIMD at widths 96 / 128, two below (launch_filters says why)
constexpr int h2b_waves(int ncb) { return ncb >= 6 ? 4 : 8; }

// The filters kernel of a matrix-core path, one direction (the gather behind it takes no dynamic LDS).
LaunchShape filters_shape(ConvPath path, int W, int G, bool bwd) {
    LaunchShape s;
    switch (path) {
        case ConvPath::kSplitRegisters:
            if (!bwd) {
                s.waves = kMaxWavesPerBlock;
                s.lds = h2_weight_bytes_l1h(W, G) + (size_t)s.waves * 128 * sizeof(float);
            } else {
                s.waves = h2b_waves(W / 16);
                s.lds = h2_weight_bytes_l1h(W, G) + ((size_t)W + s.waves * 96) * sizeof(float);
            }
            break;
        case ConvPath::kSplitPlanes: {
            const size_t budget = 160 * 1024;
            const size_t wb = h2_weight_bytes(W, G), per_wave = h2_wave_bytes(W);
            s.waves = (int)std::min<size_t>(kMaxWavesPerBlock, (budget - wb) / per_wave);
            s.lds = wb + (size_t)s.waves * per_wave;
            break;
        }
        case ConvPath::kMatrix: {
            const size_t budget = 160 * 1024 / sizeof(float);
            const size_t wfl = mfma_weight_floats(W, G), per_wave = mfma_wave_floats_bwd(W);
            s.waves = (int)std::min<size_t>(kMaxWavesPerBlock, (budget - wfl) / per_wave);
            s.lds = (wfl + (size_t)s.waves * per_wave) * sizeof(float);
            break;
        }
        case ConvPath::kVector:
            return vector_shape(W, G, bwd);
    }
    return s;
}

// Bounds on what the split-fp16 kernels put into fp16 planes, in the scaled domain they work in (see activate_fast): the largest |W2| entry,
// |Y1| and |dY1|
struct SplitBounds { double max_w2 = 0, max_y = 0, max_dy = 0; };

SplitBounds split_bounds(int W, int G, int activation, float gaussian_width, const float* w1, const float* b1, const float* w2) {
    const float s1 = activation == 0 ? kLog2e : 1.0f, s2 = activation == 0 ? 1.0f / kLog2e : 1.0f;
    SplitBounds b;
    for (int f = 0; f < W; f++) {
        double row = 0;
        for (int g = 0; g < G; g++) row += std::fabs((double)s1 * w1[(size_t)f * G + g]);
        b.max_y = std::max(b.max_y, row + std::fabs((double)s1 * b1[f]) + 1.0);     // |act(s)| <= |s| + 1 in either domain
        b.max_dy = std::max(b.max_dy, row * 0.61 / gaussian_width);                  // |d gamma / dr| <= 0.607 / sigma, act' <= 1
    }
    for (size_t q = 0; q < (size_t)W * W; q++) b.max_w2 = std::max(b.max_w2, (double)std::fabs(s2 * w2[q]));
    return b;
}

struct ConvPlan {
    ConvPath path = ConvPath::kVector;
    bool split_ok = false;          // the weights suit fp16 planes and $NNPOPS_CFCONV_SPLIT allows them (W in {32, 64, 96, 128})
    bool split_l1 = false;          // layer 1 as split products too (G + 1 <= 64 and the planes fit in LDS beside eight waves' tiles)
    int dy_log2 = 0;                // log2 of ConvParams::dy_scale
};

ConvPlan plan_conv(int W, int G, int activation, float gaussian_width, const float* w1, const float* b1, const float* w2,
                   const ConvSwitches& sw) {
    ConvPlan pl;
    if (W % 32 == 0 && W <= 128) {
        const SplitBounds b = split_bounds(W, G, activation, gaussian_width, w1, b1, w2);
        const double limit = 3.0e4;                         // fp16 holds 65504; the low planes stay below 32 in any case
        pl.split_ok = b.max_w2 < limit && b.max_y < limit && b.max_dy < limit && sw.split_level != 0;
        // dY1 goes into its fp16 planes scaled to the top of the range (ConvParams::dy_scale): the largest power of two, up to 2^12,
        // that keeps the bound on |dY1| below `limit`
        while (pl.dy_log2 < 12 && b.max_dy * std::ldexp(1.0, pl.dy_log2 + 1) < limit) pl.dy_log2++;
        pl.split_l1 = pl.split_ok && sw.split_level >= 2 && G + 1 <= 64 &&
                      h2_weight_bytes_l1h(W, G) + kMaxWavesPerBlock * h2_wave_bytes(W) <= (size_t)160 * 1024;
    }
    // the matrix-core kernels keep both weight matrices in LDS beside at least one wave's tile; layers with very many Gaussians
    // (W = 128: G > 172) do not fit and take the vector kernel, which streams its weights
    const bool mfma_fits = mfma_weight_floats(W, G) + mfma_wave_floats_bwd(W) <= (size_t)160 * 1024 / sizeof(float);
    if (sw.force_valu || W % 16 != 0 || W > 128 || !mfma_fits)
        pl.path = ConvPath::kVector;
    else if (pl.split_l1)
        pl.path = ConvPath::kSplitRegisters;
    else if (pl.split_ok && h2_weight_bytes(W, G) + h2_wave_bytes(W) <= (size_t)160 * 1024)
        pl.path = ConvPath::kSplitPlanes;
    else
        pl.path = ConvPath::kMatrix;
    return pl;
}

// the eight words of nnpops_cfconv_plan / nnpops_cfconv_describe (nnpops_hip.h)
int plan_words(ConvPath path, int W, int G, int dy_log2, int32_t out[8]) {
    const LaunchShape f = filters_shape(path, W, G, false), b = filters_shape(path, W, G, true);
    if (f.waves < 1 || b.waves < 1)
        return fail(NNPOPS_ERR_UNSUPPORTED, "CFConv tiles of width %d with %d Gaussians do not fit in LDS", W, G);
    const bool vec = path == ConvPath::kVector;
    out[0] = (int32_t)path;
    out[1] = f.waves; out[2] = (int32_t)f.lds;
    out[3] = b.waves; out[4] = (int32_t)b.lds;
    out[5] = vec ? f.cpl : 0;
    out[6] = vec ? (f.wlds ? 1 : 0) | (b.wlds ? 2 : 0) : 0;
    out[7] = dy_log2;
    return NNPOPS_OK;
}
}  // namespace

struct nnpops_cfconv {
    ConvParams p{};
    ConvPath path = ConvPath::kVector;
    bool periodic = false;
    int device = 0;
    hipStream_t stream = nullptr;
    float *d_w1t = nullptr, *d_b1 = nullptr, *d_w2t = nullptr, *d_b2 = nullptr;
    float* d_w2 = nullptr;          // W2 as given, [out][in]: the weight-gradient kernels (cfconv_weight_grad.h)
    float gaussian_width = 0;       // as given to create(): plan_conv's bounds are recomputed from it by set_weights()
    // shifted softplus on the matrix-core path: log2(e) folded into layer 1 and ln(2) into W2, so that the
    // activation is exp2 / fma / log2 with no scaling multiplies (see activate_fast)
    float *d_w1t_s = nullptr, *d_b1_s = nullptr, *d_w2t_s = nullptr;
    int blocks = 256;
    // split-fp16 kernels: W1^T with the bias row (kSplitPlanes), the two fp16 planes of W2 [out][in], the two of W1 with the bias
    // (kSplitRegisters)
    float* d_w1b = nullptr;
    _Float16 *d_w2h = nullptr, *d_w2l = nullptr, *d_w1h = nullptr, *d_w1l = nullptr;
    // filter rows F[pid][W] and pair forces s[pid] of the half-list path (+1: the all-zero row); sized on first use
    float *d_filt = nullptr, *d_pair_s = nullptr;
    size_t spill_rows = 0;
    // whose filter rows d_filt holds (the forward call writes them; a backward call on the same build of the same list reads them
    // back instead of storing them again: the same numbers to the last bit or two, 67 MB per call at config 3)
    const void* filt_list = nullptr;
    unsigned long long filt_epoch = 0;
    bool graph_seen = false;      // a filters launch of this convolution has been captured into a graph: replays write d_filt unseen
    bool reuse_filters = true;                     // $NNPOPS_CFCONV_REUSE_FILTERS=0: always store
    int dy_log2 = 0;                               // log2 of p.dy_scale (nnpops_cfconv_describe)
    // box-gradient calls only (nnpops_cfconv_backprop_box), sized on first use like d_filt: the partial sums of the pass
    // [cfconv_box_blocks(N)][9] ([N][9] once a list of frames has asked: ensure_box_buffers) and, on the vector path, the pair scalar of every row entry [N][cap]
    double* d_box_partials = nullptr;
    size_t box_partials_len = 0;       // in partial sums (9 doubles each)
    float* d_row_s = nullptr;
    size_t row_s_len = 0;
    // weight-gradient calls only (nnpops_cfconv_backprop_weights), sized once on first use: the workgroups' partial sums
    // [wgrad_blocks][W (W + G + 2)]
    float* d_wgrad_partials = nullptr;
    int wgrad_blocks = 0;
    // nnpops_cfconv_double_backward_weights: a = u.(Q_j - Q_i) per pair slot (it shares the partial rows above)
    float* d_pair_a = nullptr;
    size_t pair_a_len = 0;
};

extern "C" {

int nnpops_cfconv_neighbors_create(nnpops_cfconv_neighbors_t* out, int num_atoms, float cutoff, int periodic, int device) {
    NNPOPS_REQUIRE(out != nullptr, "out handle pointer is NULL");
    *out = nullptr;
    NNPOPS_REQUIRE(num_atoms > 0 && num_atoms <= kIdMask, "num_atoms must be in [1, %d]", kIdMask);
    NNPOPS_REQUIRE(cutoff > 0, "cutoff must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(NNPOPS_ERR_NO_DEVICE, "no HIP device available");
    NNPOPS_REQUIRE(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
    auto* h = new nnpops_cfconv_neighbors();
    h->N = num_atoms; h->cutoff = cutoff; h->periodic = periodic != 0; h->device = device;
    DeviceGuard guard(device);
    int rc;
    auto cleanup = [&](int code) { nnpops_cfconv_neighbors_destroy(h); return code; };
    if ((rc = dev_alloc(&h->d_rows, (size_t)num_atoms * h->cap))) return cleanup(rc);
    if ((rc = dev_alloc(&h->d_cnt, (size_t)num_atoms))) return cleanup(rc);
    if ((rc = dev_alloc(&h->d_status, (size_t)kStWordsN))) return cleanup(rc);
    if ((rc = h->cells.allocate(num_atoms, h->periodic, /*tiled_scan=*/false))) return cleanup(rc);     // (one-block scan at every size)
    if ((rc = dev_alloc(&h->d_lo_cnt, (size_t)num_atoms))) return cleanup(rc);
    if ((rc = dev_alloc(&h->d_half_off, (size_t)num_atoms + 1))) return cleanup(rc);
    if (hipMemset(h->d_lo_cnt, 0, sizeof(int) * num_atoms) != hipSuccess || hipMemset(h->d_half_off, 0, sizeof(int) * ((size_t)num_atoms + 1)) != hipSuccess)
        return cleanup(fail(NNPOPS_ERR_HIP, "memset failed"));
    if ((rc = alloc_half(h))) return cleanup(rc);
    if (hipMemset(h->d_cnt, 0, sizeof(int) * num_atoms) != hipSuccess || hipMemset(h->d_status, 0, sizeof(int) * kStWordsN) != hipSuccess)
        return cleanup(fail(NNPOPS_ERR_HIP, "memset failed"));
    *out = h;
    return NNPOPS_OK;
}

int nnpops_cfconv_neighbors_destroy(nnpops_cfconv_neighbors_t h) {
    if (!h) return NNPOPS_OK;
    DeviceGuard guard(h->device);
    dev_free(h->d_rows); dev_free(h->d_cnt); dev_free(h->d_status); dev_free(h->d_segment);
    dev_free(h->d_frame); dev_free(h->d_frame_offsets); dev_free(h->d_frame_blocks); dev_free(h->d_frame_first);
    dev_free(h->d_lo_cnt); dev_free(h->d_half_off); dev_free(h->d_pid); dev_free(h->d_half_r); dev_free(h->d_half_ij); dev_free(h->d_ids);
    h->cells.release();
    delete h;
    return NNPOPS_OK;
}

int nnpops_cfconv_neighbors_set_stream(nnpops_cfconv_neighbors_t h, void* stream) {
    NNPOPS_REQUIRE(h != nullptr, "NULL handle");
    h->stream = (hipStream_t)stream;
    return NNPOPS_OK;
}

// Batched molecules: the per-atom [lo, hi) table of rows_segments, uploaded once (the convention of nnpops_ani_set_molecules).
int nnpops_cfconv_neighbors_set_molecules(nnpops_cfconv_neighbors_t h, int num_molecules, const int32_t* molecule_offsets) {
    NNPOPS_REQUIRE(h != nullptr, "NULL handle");
    DeviceGuard guard(h->device);
    if (num_molecules <= 0 || molecule_offsets == nullptr) {     // back to one system
        NNPOPS_HIP_TRY(hipStreamSynchronize(h->stream));         // (a build in flight may still read the table)
        dev_free(h->d_segment);
        h->d_segment = nullptr;
        h->built = false;
        return NNPOPS_OK;
    }
    NNPOPS_REQUIRE(!h->periodic, "batched molecules are non-periodic systems (this list was created periodic)");
    NNPOPS_REQUIRE(molecule_offsets[0] == 0 && molecule_offsets[num_molecules] == h->N,
                   "molecule_offsets must start at 0 and end at num_atoms (%d)", h->N);
    for (int m = 0; m < num_molecules; m++)
        NNPOPS_REQUIRE(molecule_offsets[m] < molecule_offsets[m + 1] && molecule_offsets[m + 1] <= h->N,
                       "molecule %d is empty or offsets are not increasing", m);
    std::vector<int2> seg(h->N);
    for (int m = 0; m < num_molecules; m++)
        for (int i = molecule_offsets[m]; i < molecule_offsets[m + 1]; i++) seg[i] = int2{molecule_offsets[m], molecule_offsets[m + 1]};
    int rc;
    if (!h->d_segment && (rc = dev_alloc(&h->d_segment, (size_t)h->N))) return rc;
    NNPOPS_HIP_TRY(hipStreamSynchronize(h->stream));
    NNPOPS_HIP_TRY(hipMemcpy(h->d_segment, seg.data(), sizeof(int2) * seg.size(), hipMemcpyHostToDevice));
    h->built = false;
    return NNPOPS_OK;
}

// Periodic frames: a batch of periodic systems behind one list, every frame in its own box.  Every table is sized and uploaded here --
// that of rows_frames and those of the per-frame box pass -- so that build(), compute(), backprop() and backprop_box() allocate nothing.
static void drop_frames(nnpops_cfconv_neighbors* h) {
    dev_free(h->d_frame); dev_free(h->d_frame_offsets); dev_free(h->d_frame_blocks); dev_free(h->d_frame_first);
    h->d_frame = nullptr; h->d_frame_offsets = nullptr; h->d_frame_blocks = nullptr; h->d_frame_first = nullptr;
    h->num_frames = 0; h->frame_blocks = 0;
}

int nnpops_cfconv_neighbors_set_frames(nnpops_cfconv_neighbors_t h, int num_frames, const int32_t* frame_offsets) {
    NNPOPS_REQUIRE(h != nullptr, "NULL handle");
    DeviceGuard guard(h->device);
    if (num_frames <= 0 || frame_offsets == nullptr) {           // back to one system
        NNPOPS_HIP_TRY(hipStreamSynchronize(h->stream));         // (a build in flight may still read the tables)
        drop_frames(h);
        h->built = false;
        return NNPOPS_OK;
    }
    NNPOPS_REQUIRE(h->periodic, "frames are periodic systems, each in its own box (this list was created non-periodic: batches of "
                                "non-periodic molecules take nnpops_cfconv_neighbors_set_molecules)");
    NNPOPS_REQUIRE(frame_offsets[0] == 0 && frame_offsets[num_frames] == h->N, "frame_offsets must start at 0 and end at num_atoms (%d)", h->N);
    for (int m = 0; m < num_frames; m++)
        NNPOPS_REQUIRE(frame_offsets[m] < frame_offsets[m + 1] && frame_offsets[m + 1] <= h->N,
                       "frame %d is empty or offsets are not increasing", m);
    std::vector<int4> fr(h->N);
    std::vector<int2> blocks;
    std::vector<int> first(num_frames + 1);
    for (int m = 0; m < num_frames; m++) {
        for (int i = frame_offsets[m]; i < frame_offsets[m + 1]; i++) fr[i] = int4{frame_offsets[m], frame_offsets[m + 1], m, 0};
        first[m] = (int)blocks.size();
        const int nb = cfconv_box_frame_blocks(frame_offsets[m + 1] - frame_offsets[m]);
        for (int k = 0; k < nb; k++) blocks.push_back(int2{m, k});
    }
    first[num_frames] = (int)blocks.size();
    NNPOPS_HIP_TRY(hipStreamSynchronize(h->stream));
    drop_frames(h);
    h->built = false;
    int rc;
    auto cleanup = [&](int code) { drop_frames(h); return code; };
    if ((rc = dev_alloc(&h->d_frame, (size_t)h->N))) return cleanup(rc);
    if ((rc = dev_alloc(&h->d_frame_offsets, (size_t)num_frames + 1))) return cleanup(rc);
    if ((rc = dev_alloc(&h->d_frame_blocks, blocks.size()))) return cleanup(rc);
    if ((rc = dev_alloc(&h->d_frame_first, first.size()))) return cleanup(rc);
    if (hipMemcpy(h->d_frame, fr.data(), sizeof(int4) * fr.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_frame_offsets, frame_offsets, sizeof(int) * ((size_t)num_frames + 1), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_frame_blocks, blocks.data(), sizeof(int2) * blocks.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_frame_first, first.data(), sizeof(int) * first.size(), hipMemcpyHostToDevice) != hipSuccess)
        return cleanup(fail(NNPOPS_ERR_HIP, "frame table upload failed"));
    h->num_frames = num_frames;
    h->frame_blocks = (int)blocks.size();
    return NNPOPS_OK;
}

int nnpops_cfconv_neighbors_build(nnpops_cfconv_neighbors_t h, const float* positions, const float* box) {
    NNPOPS_REQUIRE(h != nullptr && positions != nullptr, "NULL argument");
    NNPOPS_REQUIRE(!h->d_frame || box, "a list of periodic frames needs the box vectors of every frame, [num_frames][3][3] "
                                       "(nnpops_cfconv_neighbors_set_frames)");
    NNPOPS_REQUIRE(!h->periodic || box, "periodic neighbour list needs box vectors");
    NNPOPS_REQUIRE(!h->d_segment || !box, "a list of batched molecules takes no box vectors (nnpops_cfconv_neighbors_set_molecules)");
    DeviceGuard guard(h->device);
    const int N = h->N;
    const bool per = h->periodic;
    const float c2 = h->cutoff * h->cutoff;
    // positions and box are read in place (the rows keep displacements, nothing refers back to them later); the
    // status words are cleared by create() and by check() after it has read them, not per build
    // batched molecules overlap in space: the shared cell grid tells them nothing, so their rows come from the segmented scan at every size
    // (so do periodic frames, each in its own box: rows_frames)
    const bool use_cells = N >= 1024 && !h->cells_disabled && !h->d_segment && !h->d_frame;
    if (h->d_frame) {
        hipLaunchKernelGGL(rows_frames, dim3(N), dim3(64), 0, h->stream, N, h->num_frames, positions, box, (const int4*)h->d_frame, c2,
                           h->d_rows, h->d_ids, h->cap, h->d_cnt, h->d_lo_cnt);
    } else if (h->d_segment) {
        hipLaunchKernelGGL(rows_segments, dim3(N), dim3(64), 0, h->stream, N, positions, (const int2*)h->d_segment, c2, h->d_rows, h->d_ids,
                           h->cap, h->d_cnt, h->d_lo_cnt);
    } else if (use_cells) {
        const CellList& g = h->cells;
        launch_cell_build(h->stream, N, positions, box, per, h->cutoff, nullptr, g);
        if (per)
            hipLaunchKernelGGL(rows_cells<true>, dim3(N), dim3(64), 0, h->stream, box, c2, g.grid, g.cell_start,
                               g.sorted_cell, g.sorted_pos, h->d_rows, h->d_ids, h->cap, h->d_cnt, h->d_lo_cnt, h->d_status, g.hist);
        else
            hipLaunchKernelGGL(rows_cells<false>, dim3(N), dim3(64), 0, h->stream, box, c2, g.grid, g.cell_start,
                               g.sorted_cell, g.sorted_pos, h->d_rows, h->d_ids, h->cap, h->d_cnt, h->d_lo_cnt, h->d_status, g.hist);
    } else if (per) {
        hipLaunchKernelGGL(rows_allpairs<true>, dim3(N), dim3(64), 0, h->stream, N, positions, box, c2, h->d_rows, h->d_ids, h->cap, h->d_cnt, h->d_lo_cnt);
    } else {
        hipLaunchKernelGGL(rows_allpairs<false>, dim3(N), dim3(64), 0, h->stream, N, positions, box, c2, h->d_rows, h->d_ids, h->cap, h->d_cnt, h->d_lo_cnt);
    }
    NNPOPS_HIP_TRY(hipGetLastError());
    h->built = true;
    h->half_built = false;
    static std::atomic<unsigned long long> build_counter{0};      // (unique across lists: a new list at a freed list's address is another build)
    h->epoch = ++build_counter;
    h->cell_ordered = use_cells;
    if (h->want_half) return launch_half_build(h, h->stream);
    return NNPOPS_OK;
}

int nnpops_cfconv_neighbors_build_count(nnpops_cfconv_neighbors_t h, unsigned long long* count) {
    NNPOPS_REQUIRE(h != nullptr && count != nullptr, "NULL argument");
    *count = h->built ? h->epoch : 0;       // 0: never built, or the last build was rejected by check()
    return NNPOPS_OK;
}

int nnpops_cfconv_neighbors_check(nnpops_cfconv_neighbors_t h, int* num_pairs) {
    NNPOPS_REQUIRE(h != nullptr, "NULL handle");
    DeviceGuard guard(h->device);
    int st[kStWordsN] = {0, 0, 0, 0};
    // the statistics are recomputed on every call; the overflow word keeps the builder's "grid unusable" bit
    NNPOPS_HIP_TRY(hipMemsetAsync(h->d_status + kStMaxRow, 0, 2 * sizeof(int), h->stream));
    hipLaunchKernelGGL(row_stats, dim3(std::min(64, div_up(h->N, 256))), dim3(256), 0, h->stream, h->N, h->d_cnt, h->d_rows,
                       h->cap, h->d_status);
    NNPOPS_HIP_TRY(hipGetLastError());
    NNPOPS_HIP_TRY(hipMemcpyAsync(st, h->d_status, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    NNPOPS_HIP_TRY(hipMemsetAsync(h->d_status, 0, sizeof(int) * kStWordsN, h->stream));   // consumed: builds do not clear it
    NNPOPS_HIP_TRY(hipStreamSynchronize(h->stream));
    if (num_pairs) *num_pairs = st[kStPairs];
    if (st[kStOverflow] & kGridBinOverflow) {      // a cell holds more atoms than a bin of the two-kernel grid build: grow the bins
        int old_bin;
        int rc = h->cells.grow_bins(&old_bin);
        if (rc != NNPOPS_OK) return rc;
        h->built = false;
        return fail(NNPOPS_ERR_CAPACITY, "cell bins overflowed (%d ids per cell); grown to %d, call build() again", old_bin, h->cells.bin_cap);
    }
    if (st[kStOverflow] & kGridBoxTooSmall) {
        h->cells_disabled = true;
        h->built = false;
        return fail(NNPOPS_ERR_CAPACITY, "periodic box is fewer than 3 cells wide on some axis: switched to the all-pairs "
                                         "neighbour search, call build() again");
    }
    if (st[kStOverflow]) {
        const int old = h->cap;
        while (h->cap < st[kStMaxRow]) h->cap *= 2;
        dev_free(h->d_rows);
        h->d_rows = nullptr;
        int rc = dev_alloc(&h->d_rows, (size_t)h->N * h->cap);
        if (rc != NNPOPS_OK) return rc;
        if ((rc = alloc_half(h)) != NNPOPS_OK) return rc;
        h->built = false;
        return fail(NNPOPS_ERR_CAPACITY, "neighbour rows overflowed (max %d > %d); capacity grown to %d, call build() again",
                    st[kStMaxRow], old, h->cap);
    }
    return NNPOPS_OK;
}

int nnpops_cfconv_neighbors_read_grid(nnpops_cfconv_neighbors_t h, int32_t* out) {
    NNPOPS_REQUIRE(h != nullptr && out != nullptr, "NULL argument");
    DeviceGuard guard(h->device);
    return h->cells.read_words(h->stream, out);
}

int nnpops_cfconv_neighbors_export(nnpops_cfconv_neighbors_t h, int capacity, int32_t* pair_atoms, float* distances) {
    NNPOPS_REQUIRE(h != nullptr && pair_atoms && distances, "NULL argument");
    NNPOPS_REQUIRE(h->built, "export() must follow build()");
    DeviceGuard guard(h->device);
    std::vector<float4> rows((size_t)h->N * h->cap);
    std::vector<int> cnt(h->N);
    NNPOPS_HIP_TRY(hipStreamSynchronize(h->stream));
    NNPOPS_HIP_TRY(hipMemcpy(rows.data(), h->d_rows, rows.size() * sizeof(float4), hipMemcpyDeviceToHost));
    NNPOPS_HIP_TRY(hipMemcpy(cnt.data(), h->d_cnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    int p = 0;
    for (int i = 0; i < h->N; i++) {
        std::vector<std::pair<int, float>> half;
        for (int e = 0; e < std::min(cnt[i], h->cap); e++) {
            const float4 r = rows[(size_t)i * h->cap + e];
            int j;
            std::memcpy(&j, &r.w, sizeof(int));
            j &= kIdMask;
            if (j > i) half.push_back({j, std::sqrt(r.x * r.x + r.y * r.y + r.z * r.z)});
        }
        std::sort(half.begin(), half.end());
        for (auto& e : half) {
            if (p >= capacity) return fail(NNPOPS_ERR_CAPACITY, "export capacity %d too small", capacity);
            pair_atoms[p] = i;
            pair_atoms[capacity + p] = e.first;
            distances[p] = e.second;
            p++;
        }
    }
    return NNPOPS_OK;
}

}  // extern "C"

// What a convolution derives from its four weight arrays: the plan (path, dy_log2) and every packed form on the device.  Shared by
// nnpops_cfconv_create and nnpops_cfconv_set_weights, so that a handle given new weights holds what a fresh one would.  Buffers are
// allocated on first need and kept (their sizes depend on W and G alone); the caller holds the device and has drained the stream.
static int plan_and_upload(nnpops_cfconv* h, const float* w1, const float* b1, const float* w2, const float* b2) {
    const int W = h->p.W, G = h->p.G, activation = h->p.activation;
    const ConvSwitches sw = read_switches();
    h->reuse_filters = sw.reuse_filters;
    const ConvPlan plan = plan_conv(W, G, activation, h->gaussian_width, w1, b1, w2, sw);
    h->path = plan.path;
    h->dy_log2 = plan.dy_log2;
    h->p.dy_scale = (float)std::ldexp(1.0, plan.dy_log2);
    h->p.dy_unscale = (float)std::ldexp(1.0, -plan.dy_log2);
    std::vector<float> w1t((size_t)G * W), w2t((size_t)W * W);
    for (int a = 0; a < W; a++)
        for (int g = 0; g < G; g++) w1t[(size_t)g * W + a] = w1[(size_t)a * G + g];        // core layout [W][G], CpuCFConv.cpp:163
    for (int a = 0; a < W; a++)
        for (int b = 0; b < W; b++) w2t[(size_t)b * W + a] = w2[(size_t)a * W + b];        // [out][in], CpuCFConv.cpp:174
    int rc;
    if (!h->d_w1t && (rc = dev_alloc(&h->d_w1t, w1t.size()))) return rc;
    if (!h->d_w2t && (rc = dev_alloc(&h->d_w2t, w2t.size()))) return rc;
    if (!h->d_b1 && (rc = dev_alloc(&h->d_b1, (size_t)W))) return rc;
    if (!h->d_b2 && (rc = dev_alloc(&h->d_b2, (size_t)W))) return rc;
    if (!h->d_w2 && (rc = dev_alloc(&h->d_w2, (size_t)W * W))) return rc;
    if (hipMemcpy(h->d_w1t, w1t.data(), w1t.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_w2t, w2t.data(), w2t.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_b1, b1, (size_t)W * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_b2, b2, (size_t)W * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_w2, w2, (size_t)W * W * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(NNPOPS_ERR_HIP, "weight upload failed");
    if (activation == 0) {
        std::vector<float> w1s(w1t), w2s(w2t), b1s(b1, b1 + W);
        for (float& v : w1s) v *= kLog2e;
        for (float& v : b1s) v *= kLog2e;
        for (float& v : w2s) v *= 1.0f / kLog2e;
        if (!h->d_w1t_s && (rc = dev_alloc(&h->d_w1t_s, w1s.size()))) return rc;
        if (!h->d_w2t_s && (rc = dev_alloc(&h->d_w2t_s, w2s.size()))) return rc;
        if (!h->d_b1_s && (rc = dev_alloc(&h->d_b1_s, (size_t)W))) return rc;
        if (hipMemcpy(h->d_w1t_s, w1s.data(), w1s.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_w2t_s, w2s.data(), w2s.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_b1_s, b1s.data(), (size_t)W * 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail(NNPOPS_ERR_HIP, "weight upload failed");
    }
    if (plan.split_ok) {
        // operands of the split-fp16 kernels, in the scaled domain they work in (see activate_fast)
        const float s1 = activation == 0 ? kLog2e : 1.0f, s2 = activation == 0 ? 1.0f / kLog2e : 1.0f;
        const int Gq = h2_l1_rows(G);
        std::vector<float> w1b((size_t)Gq * W, 0.f);
        std::vector<_Float16> w2h((size_t)W * W), w2l((size_t)W * W);
        for (int f = 0; f < W; f++) {
            for (int g = 0; g < G; g++) w1b[(size_t)g * W + f] = s1 * w1[(size_t)f * G + g];
            w1b[(size_t)G * W + f] = s1 * b1[f];
        }
        for (int f2 = 0; f2 < W; f2++)
            for (int k = 0; k < W; k++) {
                const float v = s2 * w2[(size_t)f2 * W + k];
                const _Float16 hi = (_Float16)v;
                w2h[(size_t)f2 * W + k] = hi;
                w2l[(size_t)f2 * W + k] = (_Float16)((v - (float)hi) * kLoScale);
            }
        if (plan.split_l1) {
            const int rowh = h2_l1_row_bytes(G) / 2;        // halves per plane row
            std::vector<_Float16> w1h((size_t)W * rowh, (_Float16)0.f), w1l((size_t)W * rowh, (_Float16)0.f);
            for (int f = 0; f < W; f++)
                for (int k = 0; k <= G; k++) {
                    const float v = w1b[(size_t)k * W + f];  // (row G = the bias)
                    const _Float16 hi = (_Float16)v;
                    w1h[(size_t)f * rowh + k] = hi;
                    w1l[(size_t)f * rowh + k] = (_Float16)((v - (float)hi) * kLoScale);
                }
            if (!h->d_w1h && (rc = dev_alloc(&h->d_w1h, w1h.size()))) return rc;
            if (!h->d_w1l && (rc = dev_alloc(&h->d_w1l, w1l.size()))) return rc;
            if (hipMemcpy(h->d_w1h, w1h.data(), w1h.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(h->d_w1l, w1l.data(), w1l.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
                return fail(NNPOPS_ERR_HIP, "weight upload failed");
        }
        if (!h->d_w1b && (rc = dev_alloc(&h->d_w1b, w1b.size()))) return rc;
        if (!h->d_w2h && (rc = dev_alloc(&h->d_w2h, w2h.size()))) return rc;
        if (!h->d_w2l && (rc = dev_alloc(&h->d_w2l, w2l.size()))) return rc;
        if (hipMemcpy(h->d_w1b, w1b.data(), w1b.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_w2h, w2h.data(), w2h.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(h->d_w2l, w2l.data(), w2l.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
            return fail(NNPOPS_ERR_HIP, "weight upload failed");
    }
    h->filt_list = nullptr;                                 // the kept filter rows belong to the old weights
    return NNPOPS_OK;
}

extern "C" {

int nnpops_cfconv_create(nnpops_cfconv_t* out, int num_atoms, int width, int num_gaussians, float cutoff, int periodic,
                         float gaussian_width, int activation, const float* w1, const float* b1, const float* w2,
                         const float* b2, int device) {
    NNPOPS_REQUIRE(out != nullptr, "out handle pointer is NULL");
    *out = nullptr;
    NNPOPS_REQUIRE(num_atoms > 0, "num_atoms must be positive");
    NNPOPS_REQUIRE(b2 != nullptr, "NULL weight pointer");
    NNPOPS_REQUIRE(cutoff > 0, "cutoff must be positive");
    if (int rc = check_layer(width, num_gaussians, gaussian_width, activation, w1, b1, w2)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(NNPOPS_ERR_NO_DEVICE, "no HIP device available");
    NNPOPS_REQUIRE(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
    auto* h = new nnpops_cfconv();
    h->p.N = num_atoms; h->p.W = width; h->p.G = num_gaussians; h->p.cutoff = cutoff;
    h->p.sigma_inv = 1.0f / gaussian_width; h->p.activation = activation;
    h->p.skip_filter_store = 0; h->p.dy_scale = 1.0f; h->p.dy_unscale = 1.0f;
    h->periodic = periodic != 0; h->device = device;
    h->gaussian_width = gaussian_width;
    DeviceGuard guard(device);
    if (int rc = plan_and_upload(h, w1, b1, w2, b2)) { nnpops_cfconv_destroy(h); return rc; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->blocks = prop.multiProcessorCount;
    *out = h;
    return NNPOPS_OK;
}

int nnpops_cfconv_plan(int width, int num_gaussians, float gaussian_width, int activation, const float* w1, const float* b1,
                       const float* w2, int32_t out[8]) {
    NNPOPS_REQUIRE(out != nullptr, "out pointer is NULL");
    if (int rc = check_layer(width, num_gaussians, gaussian_width, activation, w1, b1, w2)) return rc;
    const ConvPlan plan = plan_conv(width, num_gaussians, activation, gaussian_width, w1, b1, w2, read_switches());
    return plan_words(plan.path, width, num_gaussians, plan.dy_log2, out);
}

int nnpops_cfconv_describe(nnpops_cfconv_t h, int32_t out[8]) {
    NNPOPS_REQUIRE(h != nullptr && out != nullptr, "NULL argument");
    return plan_words(h->path, h->p.W, h->p.G, h->dy_log2, out);
}

int nnpops_cfconv_destroy(nnpops_cfconv_t h) {
    if (!h) return NNPOPS_OK;
    DeviceGuard guard(h->device);
    dev_free(h->d_w1t); dev_free(h->d_w2t); dev_free(h->d_b1); dev_free(h->d_b2); dev_free(h->d_w2); dev_free(h->d_wgrad_partials); dev_free(h->d_pair_a);
    dev_free(h->d_w1t_s); dev_free(h->d_w2t_s); dev_free(h->d_b1_s);
    dev_free(h->d_filt); dev_free(h->d_pair_s); dev_free(h->d_box_partials); dev_free(h->d_row_s);
    dev_free(h->d_w1b); dev_free(h->d_w2h); dev_free(h->d_w2l); dev_free(h->d_w1h); dev_free(h->d_w1l);
    delete h;
    return NNPOPS_OK;
}

int nnpops_cfconv_set_stream(nnpops_cfconv_t h, void* stream) {
    NNPOPS_REQUIRE(h != nullptr, "NULL handle");
    h->stream = (hipStream_t)stream;
    return NNPOPS_OK;
}

}  // extern "C"

namespace {

// (ROW_S: the pair scalar of every row entry to h->d_row_s and nothing else, for a box-gradient call)
template <int ACT, int CPL, bool BWD, bool WLDS = true, bool ROW_S = false>
int launch_conv(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* gout, float* out, float* pos_grad) {
    // as many waves per workgroup as fit next to the shared weights (vector_shape, which also chose this instantiation)
    const LaunchShape shape = vector_shape(h->p.W, h->p.G, BWD);
    if (shape.waves < 1 || shape.wlds != WLDS || shape.cpl != CPL)
        return fail(NNPOPS_ERR_UNSUPPORTED, "CFConv tiles of width %d with %d Gaussians do not fit in LDS", h->p.W, h->p.G);
    const int wpb = shape.waves;
    const size_t lds = shape.lds;
    auto k = cfconv_kernel<ACT, CPL, BWD, WLDS, ROW_S>;
    if (lds > 64 * 1024)
        NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int blocks = std::max(1, std::min(h->blocks, div_up(h->p.N, wpb)));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * wpb), lds, h->stream, h->p, h->d_w1t, h->d_b1, h->d_w2t, h->d_b2,
                       nb->d_rows, nb->d_cnt, nb->cap, x, gout, out, pos_grad, ROW_S ? h->d_row_s : (float*)nullptr);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

// the vector kernels: weights in LDS when they fit beside one wave's tiles, else streamed through the caches
template <bool BWD, bool ROW_S = false>
int launch_vector(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* gout, float* out, float* pos_grad) {
    const LaunchShape shape = vector_shape(h->p.W, h->p.G, BWD);
    if (shape.wlds) {
        const bool two = shape.cpl == 2;
        if (h->p.activation == 0)
            return two ? launch_conv<0, 2, BWD, true, ROW_S>(h, nb, x, gout, out, pos_grad) : launch_conv<0, 1, BWD, true, ROW_S>(h, nb, x, gout, out, pos_grad);
        return two ? launch_conv<1, 2, BWD, true, ROW_S>(h, nb, x, gout, out, pos_grad) : launch_conv<1, 1, BWD, true, ROW_S>(h, nb, x, gout, out, pos_grad);
    }
    const int cpl = shape.cpl;
    if (h->p.activation == 0) {
        if (cpl <= 2) return launch_conv<0, 2, BWD, false, ROW_S>(h, nb, x, gout, out, pos_grad);
        if (cpl <= 4) return launch_conv<0, 4, BWD, false, ROW_S>(h, nb, x, gout, out, pos_grad);
        return launch_conv<0, 8, BWD, false, ROW_S>(h, nb, x, gout, out, pos_grad);
    }
    if (cpl <= 2) return launch_conv<1, 2, BWD, false, ROW_S>(h, nb, x, gout, out, pos_grad);
    if (cpl <= 4) return launch_conv<1, 4, BWD, false, ROW_S>(h, nb, x, gout, out, pos_grad);
    return launch_conv<1, 8, BWD, false, ROW_S>(h, nb, x, gout, out, pos_grad);
}

// the pair slots behind the neighbour rows and the convolution's filter-row buffers
int ensure_half_path(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb) {
    nb->want_half = true;                                   // later builds carry the pair slots along
    if (!nb->half_built) {
        const int rc = launch_half_build(nb, h->stream);
        if (rc != NNPOPS_OK) return rc;
    }
    const size_t need = (size_t)nb->pair_cap() + 1;
    if (h->spill_rows < need) {                             // (first use, or the neighbour rows have grown: not capturable)
        dev_free(h->d_filt); dev_free(h->d_pair_s);
        h->d_filt = nullptr; h->d_pair_s = nullptr; h->spill_rows = 0; h->filt_list = nullptr;
        int rc;
        if ((rc = dev_alloc(&h->d_filt, need * h->p.W))) return rc;
        if ((rc = dev_alloc(&h->d_pair_s, need))) return rc;
        h->spill_rows = need;
    }

    return NNPOPS_OK;
}

// The filters kernel of the convolution's path: it leaves the filter rows of this list in d_filt (backward: and the pair forces in
// d_pair_s) for the gather.  Odd numbers of column blocks never take a split path (nnpops_cfconv_create).
template <int ACT, int NCB, bool BWD>
int launch_filters(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const ConvParams& cp, const float* x, const float* gout) {
    const int pair_cap = nb->pair_cap();
    const LaunchShape shape = filters_shape(h->path, h->p.W, h->p.G, BWD);     // waves per workgroup and LDS: what describe() reports
    switch (h->path) {
        case ConvPath::kSplitRegisters:
            if constexpr (NCB % 2 == 0 && !BWD) {
                // forward: 32 pairs per wave, layer 2 fed from registers
                // (measured, 10 000 atoms: two tiles per pass on 8 waves 45.8 us; one tile per pass on 12 waves -- three per SIMD,
                //  154 registers -- 50.5 us; on 16 waves, spilling, 68.6 us: the weight reads a second tile shares are worth more than a third wave)
                // (... and on FOUR waves -- one per SIMD, 512 registers -- two tiles per pass 57.0 us, four tiles per pass 84.8 us)
                auto k2 = cfconv_filters_h2x2<ACT, NCB, 2, kMaxWavesPerBlock>;
                const int wv = shape.waves;                  // (kMaxWavesPerBlock, the kernel's launch bound)
                const size_t lds2 = shape.lds;
                if (lds2 > 64 * 1024)
                    NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
                hipLaunchKernelGGL(k2, dim3(h->blocks), dim3(64 * wv), lds2, h->stream, cp, h->d_w1h, h->d_w1l, h->d_w2h, h->d_w2l,
                                   h->d_b2, nb->d_half_off, nb->d_half_r, pair_cap, h->d_filt);
                return NNPOPS_OK;
            } else if constexpr (NCB % 2 == 0) {
                // backward: one pass per layer, operands from registers.  FOUR waves per workgroup at widths 96 / 128: one per SIMD,
                // which gives the wave all 512 registers of its lanes.  The kernel holds four accumulator sets, four sets of operand
                // fragments and the x / gout rows of its pair: ~410 registers.  With two waves per SIMD (256 each) it spills 444 bytes
                // per lane and takes 206 us; with one, nothing is spilled: 99 us (the round-5 four-pass kernel, two waves per SIMD:
                // 125.5 us).  Widths below 96 fit two waves per SIMD.
                constexpr int wv = h2b_waves(NCB);
                auto k2 = cfconv_filters_h2b<ACT, NCB, wv>;
                const size_t lds2 = shape.lds;
                if (lds2 > 64 * 1024)
                    NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
                hipLaunchKernelGGL(k2, dim3(h->blocks), dim3(64 * wv), lds2, h->stream, cp, h->d_w1h, h->d_w1l, h->d_w2h, h->d_w2l,
                                   h->d_b2, nb->d_half_off, nb->d_half_r, nb->d_half_ij, pair_cap, x, gout, h->d_filt, h->d_pair_s);
                return NNPOPS_OK;
            }
            break;
        case ConvPath::kSplitPlanes:
            if constexpr (NCB % 2 == 0) {
                const int wpb = shape.waves;
                const size_t lds = shape.lds;
                auto k = cfconv_filters_h2<ACT, NCB, BWD>;
                if (lds > 64 * 1024)
                    NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(k, dim3(h->blocks), dim3(64 * wpb), lds, h->stream, cp, h->d_w1b, h->d_w1h, h->d_w1l, h->d_w2h,
                                   h->d_w2l, h->d_b2, nb->d_half_off, nb->d_half_r, nb->d_half_ij, pair_cap, x, gout, h->d_filt,
                                   h->d_pair_s);
                return NNPOPS_OK;
            }
            break;
        case ConvPath::kMatrix: {
            const int wpb = shape.waves;
            const size_t lds = shape.lds;
            auto k = cfconv_filters_mfma<ACT, NCB, BWD>;
            if (lds > 64 * 1024)
                NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k, dim3(h->blocks), dim3(64 * wpb), lds, h->stream, cp, ACT == 0 ? h->d_w1t_s : h->d_w1t,
                               ACT == 0 ? h->d_b1_s : h->d_b1, ACT == 0 ? h->d_w2t_s : h->d_w2t, h->d_b2, nb->d_half_off, nb->d_half_r,
                               nb->d_half_ij, pair_cap, x, gout, h->d_filt, h->d_pair_s);
            return NNPOPS_OK;
        }
        case ConvPath::kVector:
            break;
    }
    return fail(NNPOPS_ERR_UNSUPPORTED, "CFConv: no filters kernel for width %d on this path", h->p.W);
}

// Half-list path: filters once per pair, then the owner-computes gather.
template <int ACT, int NCB, bool BWD>
int launch_half(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* gout, float* out, float* pos_grad) {
    int rc = ensure_half_path(h, nb);
    if (rc != NNPOPS_OK) return rc;
    const int pair_cap = nb->pair_cap();
    bool capturing = true;                                  // (unknown = treated as capturing)
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(h->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) capturing = false;
    }
    ConvParams cp = h->p;
    if (BWD && !capturing && !h->graph_seen && h->reuse_filters && h->filt_list == nb && h->filt_epoch == nb->epoch)
        cp.skip_filter_store = 1;                           // (read by the split kernels only)
    if ((rc = launch_filters<ACT, NCB, BWD>(h, nb, cp, x, gout)) != NNPOPS_OK) return rc;
    // Every filters kernel, either direction, leaves this list's rows in d_filt -- once it has RUN.  A launch that is only being captured has
    // written nothing yet, and a replay of the captured graph writes d_filt behind the host's back, for whatever build of whatever list
    // it was captured on: nothing is recorded while capturing, and a convolution that has ever been captured never
    // reads rows back again (graph_seen) -- the host cannot know what the last replay left there.
    // (Call-history dependence, documented: a backward call that reads the forward call's rows back differs from one that stores its
    //  own in the last bit or two -- the forward kernel adds the second layer's bias behind the products, the backward kernel carries
    //  it in the accumulator, docs/LAB_NOTEBOOK_r05.md #13; both are inside the parity bars, NNPOPS_CFCONV_REUSE_FILTERS=0 switches it off.)
    if (capturing) { h->graph_seen = true; h->filt_list = nullptr; }
    else { h->filt_list = nb; h->filt_epoch = nb->epoch; }
    const int N = h->p.N;
    const float* v = BWD ? gout : x;
    const float4* order = nb->cell_ordered ? nb->cells.sorted_pos : nullptr;
    if (h->p.W == 128)
        hipLaunchKernelGGL((cfconv_gather<BWD, true>), dim3(div_up(N, 4)), dim3(256), 0, h->stream, N, h->p.W, nb->d_rows, nb->d_cnt,
                           nb->cap, nb->d_pid, pair_cap, h->d_filt, h->d_pair_s, v, out, pos_grad, order);
    else
        hipLaunchKernelGGL((cfconv_gather<BWD, false>), dim3(div_up(N, 4)), dim3(256), 0, h->stream, N, h->p.W, nb->d_rows, nb->d_cnt,
                           nb->cap, nb->d_pid, pair_cap, h->d_filt, h->d_pair_s, v, out, pos_grad, order);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

template <int ACT, bool BWD>
int dispatch_half(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* gout, float* out, float* pos_grad) {
    switch (h->p.W) {
        case 16:  return launch_half<ACT, 1, BWD>(h, nb, x, gout, out, pos_grad);
        case 32:  return launch_half<ACT, 2, BWD>(h, nb, x, gout, out, pos_grad);
        case 48:  return launch_half<ACT, 3, BWD>(h, nb, x, gout, out, pos_grad);
        case 64:  return launch_half<ACT, 4, BWD>(h, nb, x, gout, out, pos_grad);
        case 80:  return launch_half<ACT, 5, BWD>(h, nb, x, gout, out, pos_grad);
        case 96:  return launch_half<ACT, 6, BWD>(h, nb, x, gout, out, pos_grad);
        case 112: return launch_half<ACT, 7, BWD>(h, nb, x, gout, out, pos_grad);
        case 128: return launch_half<ACT, 8, BWD>(h, nb, x, gout, out, pos_grad);
        default:  return fail(NNPOPS_ERR_UNSUPPORTED, "CFConv: no matrix-core kernel for width %d", h->p.W);
    }
}

template <bool BWD>
int dispatch_conv(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* gout, float* out, float* pos_grad) {
    if (h->path == ConvPath::kVector) return launch_vector<BWD>(h, nb, x, gout, out, pos_grad);
    return h->p.activation == 0 ? dispatch_half<0, BWD>(h, nb, x, gout, out, pos_grad)
                                : dispatch_half<1, BWD>(h, nb, x, gout, out, pos_grad);
}

// what a box-gradient call keeps beside the backward pass's own buffers (first use, or the neighbour rows have grown: not capturable)
int ensure_box_buffers(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, bool row_s) {
    int rc;
    // (a list of frames leaves one partial sum per workgroup of its pass, at most one per atom whatever the partition)
    const size_t partials = nb->d_frame ? (size_t)h->p.N : (size_t)cfconv_box_blocks(h->p.N);
    if (h->box_partials_len < partials) {
        dev_free(h->d_box_partials);
        h->d_box_partials = nullptr; h->box_partials_len = 0;
        if ((rc = dev_alloc(&h->d_box_partials, 9 * partials))) return rc;
        h->box_partials_len = partials;
    }
    const size_t need = (size_t)nb->N * nb->cap;
    if (row_s && h->row_s_len < need) {
        dev_free(h->d_row_s);
        h->d_row_s = nullptr; h->row_s_len = 0;
        if ((rc = dev_alloc(&h->d_row_s, need))) return rc;
        h->row_s_len = need;
    }
    return NNPOPS_OK;
}

// The double backward (cfconv_second_order.h).  The family is a matter of the width and of LDS alone: the fp32 matrix instruction where
// W is a multiple of 16 up to 128 and both weight matrices fit in LDS beside one wave's tile, else the vector kernel.
template <int ACT, int NCB>
int launch_second_mfma(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* g, const float* V, const float* Q,
                       float* out_g, float* out_x, float* out_pos) {
    const size_t budget = 160 * 1024 / sizeof(float);
    const size_t wfl = mfma_weight_floats(h->p.W, h->p.G), per_wave = second_mfma_wave_floats(h->p.W);
    constexpr int waves = NCB > 4 ? 4 : kMaxWavesPerBlock;
    const int wpb = (int)std::min<size_t>(waves, (budget - wfl) / per_wave);
    const size_t lds = (wfl + (size_t)wpb * per_wave) * sizeof(float);
    auto k = cfconv_second_mfma<ACT, NCB, waves>;
    if (lds > 64 * 1024)
        NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int blocks = std::max(1, std::min(h->blocks, div_up(h->p.N, wpb)));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * wpb), lds, h->stream, h->p, h->d_w1t, h->d_b1, h->d_w2t, h->d_b2, nb->d_rows, nb->d_cnt,
                       nb->cap, nb->cell_ordered ? nb->cells.sorted_pos : (const float4*)nullptr, x, g, V, Q, out_g, out_x, out_pos);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

template <int ACT, int CPL, bool WLDS>
int launch_second_vector(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* g, const float* V, const float* Q,
                         float* out_g, float* out_x, float* out_pos) {
    const size_t budget = 156 * 1024 / sizeof(float);
    const size_t wfl = WLDS ? conv_weight_floats(h->p.W, h->p.G) : 0, per_wave = second_wave_floats(h->p.W, h->p.G);
    if (wfl + per_wave > budget)
        return fail(NNPOPS_ERR_UNSUPPORTED, "CFConv tiles (%zu floats) do not fit in LDS", wfl + per_wave);
    const int wpb = (int)std::min<size_t>(kMaxWavesPerBlock, (budget - wfl) / per_wave);
    const size_t lds = (wfl + (size_t)wpb * per_wave) * sizeof(float);
    auto k = cfconv_second_vector<ACT, CPL, WLDS>;
    if (lds > 64 * 1024)
        NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int blocks = std::max(1, std::min(h->blocks, div_up(h->p.N, wpb)));
    hipLaunchKernelGGL(k, dim3(blocks), dim3(64 * wpb), lds, h->stream, h->p, h->d_w1t, h->d_b1, h->d_w2t, h->d_b2, nb->d_rows, nb->d_cnt,
                       nb->cap, nb->cell_ordered ? nb->cells.sorted_pos : (const float4*)nullptr, x, g, V, Q, out_g, out_x, out_pos);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

template <int ACT>
int dispatch_second(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* g, const float* V, const float* Q,
                    float* out_g, float* out_x, float* out_pos) {
    const int W = h->p.W, G = h->p.G;
    if (W % 16 == 0 && W <= 128 && mfma_weight_floats(W, G) + second_mfma_wave_floats(W) <= (size_t)160 * 1024 / sizeof(float)) {
        switch (W) {
            case 16:  return launch_second_mfma<ACT, 1>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
            case 32:  return launch_second_mfma<ACT, 2>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
            case 48:  return launch_second_mfma<ACT, 3>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
            case 64:  return launch_second_mfma<ACT, 4>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
            case 80:  return launch_second_mfma<ACT, 5>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
            case 96:  return launch_second_mfma<ACT, 6>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
            case 112: return launch_second_mfma<ACT, 7>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
            default:  return launch_second_mfma<ACT, 8>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
        }
    }
    const size_t budget = 156 * 1024 / sizeof(float);
    if (W <= 128 && conv_weight_floats(W, G) + second_wave_floats(W, G) <= budget)
        return W > 64 ? launch_second_vector<ACT, 2, true>(h, nb, x, g, V, Q, out_g, out_x, out_pos)
                      : launch_second_vector<ACT, 1, true>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
    const int cpl = div_up(W, 64);
    if (cpl <= 2) return launch_second_vector<ACT, 2, false>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
    if (cpl <= 4) return launch_second_vector<ACT, 4, false>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
    return launch_second_vector<ACT, 8, false>(h, nb, x, g, V, Q, out_g, out_x, out_pos);
}

int check_pair(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb) {
    NNPOPS_REQUIRE(h != nullptr && nb != nullptr, "NULL handle");
    NNPOPS_REQUIRE(nb->built, "the neighbour list has not been built");
    NNPOPS_REQUIRE(nb->N == h->p.N, "neighbour list is for %d atoms, convolution for %d", nb->N, h->p.N);
    NNPOPS_REQUIRE(nb->cutoff == h->p.cutoff, "The cutoff of \"neighbors\" has changed");
    NNPOPS_REQUIRE(nb->device == h->device, "neighbour list and convolution live on different devices");
    return NNPOPS_OK;
}

// The weight gradients (cfconv_weight_grad.h).  As for the double backward, the family is a matter of the width and of LDS alone, whatever
// path the forward runs: the fp32 matrix instruction where W is a multiple of 16 up to 128 and the kernel's LDS image fits, else the
// vector kernel.  One workgroup per compute unit, fewer where the partial rows would pass kWgradPartialBytes: every matrix-core layer of
// SchNet's sizes keeps the full launch (W = 128, G = 50: 256 rows of 92 KB, 23 MB), and the widest layer the library accepts
// (W = 512, G = 256: 1.5 MB a row) runs on 21 workgroups instead of holding 400 MB.
constexpr size_t kWgradPartialBytes = (size_t)32 << 20;

bool wgrad_takes_mfma(int W, int G) {
    return W % 16 == 0 && W <= 128 && wgrad_mfma_floats(W, G) * sizeof(float) <= (size_t)160 * 1024;
}

// the partial rows, shared by both weight-gradient entry points (first call of either: not capturable)
int ensure_wgrad_partials(nnpops_cfconv* h) {
    if (h->d_wgrad_partials) return NNPOPS_OK;
    const size_t row_bytes = wgrad_row_floats(h->p.W, h->p.G) * sizeof(float);
    const int blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)h->blocks, kWgradPartialBytes / row_bytes));
    int rc;
    if ((rc = dev_alloc(&h->d_wgrad_partials, (size_t)blocks * wgrad_row_floats(h->p.W, h->p.G)))) return rc;
    h->wgrad_blocks = blocks;
    return NNPOPS_OK;
}

template <int NCB>
int launch_wgrad_mfma(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* g) {
    const size_t lds = wgrad_mfma_floats(h->p.W, h->p.G) * sizeof(float);
    auto launch = [&](auto k) {
        if (lds > 64 * 1024)
            NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(h->wgrad_blocks), dim3(64 * NCB), lds, h->stream, h->p, h->d_w1t, h->d_b1, h->d_w2, nb->d_half_off,
                           nb->d_half_r, nb->d_half_ij, nb->pair_cap(), x, g, h->d_wgrad_partials);
        return (int)NNPOPS_OK;
    };
    return wgrad_gamma_blocks(h->p.G) == 4 ? launch(cfconv_wgrad_mfma<NCB, 4>) : launch(cfconv_wgrad_mfma<NCB, 16>);
}

int launch_wgrad(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* g, float* dw1, float* db1, float* dw2,
                 float* db2) {
    const int W = h->p.W, G = h->p.G;
    nb->want_half = true;                                   // later builds carry the pair slots along (as launch_filters asks)
    int rc;
    if (!nb->half_built && (rc = launch_half_build(nb, h->stream)) != NNPOPS_OK) return rc;
    if ((rc = ensure_wgrad_partials(h)) != NNPOPS_OK) return rc;
    if (wgrad_takes_mfma(W, G)) {
        switch (W) {
            case 16:  rc = launch_wgrad_mfma<1>(h, nb, x, g); break;
            case 32:  rc = launch_wgrad_mfma<2>(h, nb, x, g); break;
            case 48:  rc = launch_wgrad_mfma<3>(h, nb, x, g); break;
            case 64:  rc = launch_wgrad_mfma<4>(h, nb, x, g); break;
            case 80:  rc = launch_wgrad_mfma<5>(h, nb, x, g); break;
            case 96:  rc = launch_wgrad_mfma<6>(h, nb, x, g); break;
            case 112: rc = launch_wgrad_mfma<7>(h, nb, x, g); break;
            default:  rc = launch_wgrad_mfma<8>(h, nb, x, g); break;
        }
        if (rc != NNPOPS_OK) return rc;
    } else {
        const size_t lds = wgrad_vector_floats(W, G) * sizeof(float);
        if (lds > 64 * 1024)
            NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)cfconv_wgrad_vector, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(cfconv_wgrad_vector, dim3(h->wgrad_blocks), dim3(kWgradVectorThreads), lds, h->stream, h->p, h->d_w1t, h->d_b1,
                           h->d_w2, nb->d_half_off, nb->d_half_r, nb->d_half_ij, nb->pair_cap(), x, g, h->d_wgrad_partials);
    }
    hipLaunchKernelGGL(cfconv_wgrad_finish, dim3(div_up((long long)wgrad_row_floats(W, G), 256)), dim3(256), 0, h->stream, W, G,
                       h->wgrad_blocks, (const float*)h->d_wgrad_partials, dw1, db1, dw2, db2);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

// The weight gradients of the double backward's scalar (cfconv_weight_grad_second.h): launch_wgrad's choice of family with the taller
// LDS image, its partial rows and its finish.  Q given: cfconv_pair_a first fills a per pair slot from the full rows.
bool wgrad2_takes_mfma(int W, int G) {
    return W % 16 == 0 && W <= 128 && wgrad2_mfma_floats(W, G) * sizeof(float) <= (size_t)160 * 1024;
}

template <int NCB>
int launch_wgrad2_mfma(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* pair_a, const float* x, const float* g, const float* V) {
    const size_t lds = wgrad2_mfma_floats(h->p.W, h->p.G) * sizeof(float);
    auto launch = [&](auto k) {
        if (lds > 64 * 1024)
            NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(h->wgrad_blocks), dim3(64 * NCB), lds, h->stream, h->p, h->d_w1t, h->d_b1, h->d_w2, nb->d_half_off,
                           nb->d_half_r, nb->d_half_ij, nb->pair_cap(), pair_a, x, g, V, h->d_wgrad_partials);
        return (int)NNPOPS_OK;
    };
    return wgrad_gamma_blocks(h->p.G) == 4 ? launch(cfconv_wgrad2_mfma<NCB, 4>) : launch(cfconv_wgrad2_mfma<NCB, 16>);
}

int launch_wgrad2(nnpops_cfconv* h, nnpops_cfconv_neighbors* nb, const float* x, const float* g, const float* V, const float* Q, float* dw1,
                  float* db1, float* dw2, float* db2) {
    const int W = h->p.W, G = h->p.G;
    nb->want_half = true;                                   // later builds carry the pair slots along (as launch_filters asks)
    int rc;
    if (!nb->half_built && (rc = launch_half_build(nb, h->stream)) != NNPOPS_OK) return rc;
    if ((rc = ensure_wgrad_partials(h)) != NNPOPS_OK) return rc;
    const float* pair_a = nullptr;
    if (Q) {
        const size_t need = (size_t)nb->pair_cap() + 1;
        if (h->pair_a_len < need) {                         // first call with Q, or the neighbour rows have grown: not capturable
            dev_free(h->d_pair_a);
            h->d_pair_a = nullptr; h->pair_a_len = 0;
            if ((rc = dev_alloc(&h->d_pair_a, need))) return rc;
            h->pair_a_len = need;
        }
        hipLaunchKernelGGL(cfconv_pair_a, dim3(div_up(nb->N, 4)), dim3(256), 0, h->stream, nb->N, (const float4*)nb->d_rows,
                           (const int*)nb->d_cnt, nb->cap, (const int*)nb->d_pid, nb->pair_cap(), Q, h->d_pair_a);
        pair_a = h->d_pair_a;
    }
    if (wgrad2_takes_mfma(W, G)) {
        switch (W) {
            case 16:  rc = launch_wgrad2_mfma<1>(h, nb, pair_a, x, g, V); break;
            case 32:  rc = launch_wgrad2_mfma<2>(h, nb, pair_a, x, g, V); break;
            case 48:  rc = launch_wgrad2_mfma<3>(h, nb, pair_a, x, g, V); break;
            case 64:  rc = launch_wgrad2_mfma<4>(h, nb, pair_a, x, g, V); break;
            case 80:  rc = launch_wgrad2_mfma<5>(h, nb, pair_a, x, g, V); break;
            case 96:  rc = launch_wgrad2_mfma<6>(h, nb, pair_a, x, g, V); break;
            case 112: rc = launch_wgrad2_mfma<7>(h, nb, pair_a, x, g, V); break;
            default:  rc = launch_wgrad2_mfma<8>(h, nb, pair_a, x, g, V); break;
        }
        if (rc != NNPOPS_OK) return rc;
    } else {
        const size_t lds = wgrad2_vector_floats(W, G) * sizeof(float);
        if (lds > 64 * 1024)
            NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)cfconv_wgrad2_vector, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(cfconv_wgrad2_vector, dim3(h->wgrad_blocks), dim3(kWgradVectorThreads), lds, h->stream, h->p, h->d_w1t, h->d_b1,
                           h->d_w2, nb->d_half_off, nb->d_half_r, nb->d_half_ij, nb->pair_cap(), pair_a, x, g, V, h->d_wgrad_partials);
    }
    hipLaunchKernelGGL(cfconv_wgrad_finish, dim3(div_up((long long)wgrad_row_floats(W, G), 256)), dim3(256), 0, h->stream, W, G,
                       h->wgrad_blocks, (const float*)h->d_wgrad_partials, dw1, db1, dw2, db2);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // namespace

extern "C" {

int nnpops_cfconv_compute(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions, const float* box,
                          const float* input, float* output) {
    (void)positions; (void)box;     // forward works from the distances stored by build() (CpuCFConv.cpp:146-147)
    int rc = check_pair(h, neighbors);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(input && output, "NULL device pointer");
    DeviceGuard guard(h->device);
    return dispatch_conv<false>(h, neighbors, input, nullptr, output, nullptr);
}

int nnpops_cfconv_backprop(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions, const float* box,
                           const float* input, const float* output_deriv, float* input_deriv, float* position_deriv) {
    (void)positions; (void)box;     // displacements were stored by build() from the same positions
    int rc = check_pair(h, neighbors);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(input && output_deriv && input_deriv && position_deriv, "NULL device pointer");
    DeviceGuard guard(h->device);
    return dispatch_conv<true>(h, neighbors, input, output_deriv, input_deriv, position_deriv);
}

int nnpops_cfconv_backprop_box(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions, const float* box,
                               const float* input, const float* output_deriv, float* input_deriv, float* position_deriv,
                               float* box_deriv) {
    int rc = check_pair(h, neighbors);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(neighbors->periodic, "the box gradient needs a periodic neighbour list (this one was created without box vectors)");
    NNPOPS_REQUIRE(positions && box && box_deriv, "NULL device pointer (the box gradient needs positions, box and box_deriv)");
    NNPOPS_REQUIRE(input && output_deriv && input_deriv && position_deriv, "NULL device pointer");
    DeviceGuard guard(h->device);
    const bool row_s = h->path == ConvPath::kVector;
    if ((rc = ensure_box_buffers(h, neighbors, row_s)) != NNPOPS_OK) return rc;
    // the backward pass exactly as nnpops_cfconv_backprop launches it (the same kernels: the same bits); the vector path, which has no
    // pair slots, then walks the rows once more for the pair scalar of every entry (cfconv_kernel<..., ROW_S>: a second evaluation of
    // the filter network, on the path that is functional rather than tuned) ...
    if ((rc = dispatch_conv<true>(h, neighbors, input, output_deriv, input_deriv, position_deriv)) != NNPOPS_OK) return rc;
    if (row_s && (rc = launch_vector<true, true>(h, neighbors, input, output_deriv, nullptr, nullptr)) != NNPOPS_OK) return rc;
    // ... then one pass over the rows and the pair scalars it left behind, and the sum of its workgroups (cfconv_box_grad.h)
    const int N = h->p.N, nblocks = cfconv_box_blocks(N);
    if (neighbors->d_frame) {
        // periodic frames: box and box_deriv are [num_frames][3][3]; every frame's workgroups, then one workgroup per frame
        const int total = neighbors->frame_blocks, B = neighbors->num_frames;
        if (row_s)
            hipLaunchKernelGGL(cfconv_box_partials_frames<true>, dim3(total), dim3(kBoxThreads), 0, h->stream, N, positions, box,
                               (const int*)neighbors->d_frame_offsets, (const int2*)neighbors->d_frame_blocks, neighbors->d_rows,
                               neighbors->d_cnt, neighbors->cap, (const int*)nullptr, 0, (const float*)h->d_row_s, h->d_box_partials);
        else
            hipLaunchKernelGGL(cfconv_box_partials_frames<false>, dim3(total), dim3(kBoxThreads), 0, h->stream, N, positions, box,
                               (const int*)neighbors->d_frame_offsets, (const int2*)neighbors->d_frame_blocks, neighbors->d_rows,
                               neighbors->d_cnt, neighbors->cap, (const int*)neighbors->d_pid, neighbors->pair_cap(),
                               (const float*)h->d_pair_s, h->d_box_partials);
        hipLaunchKernelGGL(cfconv_box_finish_frames, dim3(B), dim3(kBoxThreads), 0, h->stream, (const int*)neighbors->d_frame_first,
                           (const double*)h->d_box_partials, box_deriv);
        NNPOPS_HIP_TRY(hipGetLastError());
        return NNPOPS_OK;
    }
    const float4* order = neighbors->cell_ordered ? neighbors->cells.sorted_pos : nullptr;
    if (row_s)
        hipLaunchKernelGGL(cfconv_box_partials<true>, dim3(nblocks), dim3(kBoxThreads), 0, h->stream, N, positions, box, neighbors->d_rows,
                           neighbors->d_cnt, neighbors->cap, (const int*)nullptr, 0, (const float*)h->d_row_s, order, h->d_box_partials);
    else
        hipLaunchKernelGGL(cfconv_box_partials<false>, dim3(nblocks), dim3(kBoxThreads), 0, h->stream, N, positions, box, neighbors->d_rows,
                           neighbors->d_cnt, neighbors->cap, (const int*)neighbors->d_pid, neighbors->pair_cap(), (const float*)h->d_pair_s,
                           order, h->d_box_partials);
    hipLaunchKernelGGL(pairs_box_finish<float>, dim3(1), dim3(kBoxThreads), 0, h->stream, nblocks, (const double*)h->d_box_partials, box_deriv);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_cfconv_double_backward(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* positions, const float* input,
                                  const float* output_deriv, const float* gg_input_deriv, const float* gg_position_deriv,
                                  float* out_output_deriv, float* out_input, float* out_positions) {
    (void)positions;                // displacements were stored by build() from the same positions
    int rc = check_pair(h, neighbors);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(input && output_deriv && out_output_deriv && out_input && out_positions, "NULL device pointer");
    NNPOPS_REQUIRE(gg_input_deriv || gg_position_deriv, "gg_input_deriv and gg_position_deriv are both NULL: nothing to differentiate");
    DeviceGuard guard(h->device);
    return h->p.activation == 0
               ? dispatch_second<0>(h, neighbors, input, output_deriv, gg_input_deriv, gg_position_deriv, out_output_deriv, out_input, out_positions)
               : dispatch_second<1>(h, neighbors, input, output_deriv, gg_input_deriv, gg_position_deriv, out_output_deriv, out_input, out_positions);
}

int nnpops_cfconv_backprop_weights(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* input, const float* output_deriv,
                                   float* w1_deriv, float* b1_deriv, float* w2_deriv, float* b2_deriv) {
    int rc = check_pair(h, neighbors);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(input && output_deriv && w1_deriv && b1_deriv && w2_deriv && b2_deriv, "NULL device pointer");
    DeviceGuard guard(h->device);
    return launch_wgrad(h, neighbors, input, output_deriv, w1_deriv, b1_deriv, w2_deriv, b2_deriv);
}

int nnpops_cfconv_double_backward_weights(nnpops_cfconv_t h, nnpops_cfconv_neighbors_t neighbors, const float* input,
                                          const float* output_deriv, const float* gg_input_deriv, const float* gg_position_deriv,
                                          float* w1_deriv, float* b1_deriv, float* w2_deriv, float* b2_deriv) {
    int rc = check_pair(h, neighbors);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(input && output_deriv && w1_deriv && b1_deriv && w2_deriv && b2_deriv, "NULL device pointer");
    NNPOPS_REQUIRE(gg_input_deriv || gg_position_deriv, "gg_input_deriv and gg_position_deriv are both NULL: nothing to differentiate");
    DeviceGuard guard(h->device);
    return launch_wgrad2(h, neighbors, input, output_deriv, gg_input_deriv, gg_position_deriv, w1_deriv, b1_deriv, w2_deriv, b2_deriv);
}

int nnpops_cfconv_set_weights(nnpops_cfconv_t h, const float* w1, const float* b1, const float* w2, const float* b2) {
    NNPOPS_REQUIRE(h != nullptr, "NULL handle");
    NNPOPS_REQUIRE(w1 && b1 && w2 && b2, "NULL weight pointer");
    DeviceGuard guard(h->device);
    NNPOPS_HIP_TRY(hipStreamSynchronize(h->stream));        // launches in flight still read the old forms
    return plan_and_upload(h, w1, b1, w2, b2);
}

}  // extern "C"
