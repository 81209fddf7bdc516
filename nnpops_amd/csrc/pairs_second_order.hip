// pairs_second_order.hip -- getNeighborPairs: the box gradient of the backward pass and its second derivatives.
//
// One used slot k of a pair list, i = neighbors[0][k], j = neighbors[1][k]: the forward op emits
//     delta_k = x_i - x_j - sum_a n_ka B[a,:],   r_k = |delta_k|,   u_k = delta_k / r_k
// with n_k in Z^3 the minimum-image shift of the z -> y -> x rounds (neighbor_pairs.hip: wrapped_delta).  The backward pass forms
// G_k = g_delta,k + g_r,k u_k and adds +G_k to atom i and -G_k to atom j (neighbor_pairs.hip / pairs_index.hip); the rounds have
// zero derivative, as in the reference's CPU op (src/pytorch/neighbors/getNeighborPairsCPU.cpp:56-98), so
//     grad_B[a,:] = - sum_k n_ka G_k                                      (pairs_box_partials + pairs_box_finish)
// The backward pass Bwd(g_delta, g_r, delta, r) -> (grad_x, grad_B) is linear in (g_delta, g_r); its vector-Jacobian product with
// (h_x, h_B) is per slot, with w_k = h_x[i] - h_x[j] - sum_a n_ka h_B[a,:]:
//     d/dg_delta = w,   d/dg_r = u.w,   d/ddelta = (g_r / r) w,   d/dr = -g_r (delta.w) / r^2    (pairs_double_backward)
// The last two are the (g_r / r)(I - u u^T) w of the Hessian once they have gone back through the forward op's own backward.
//
// n_k is RECOVERED from what the list stores, not replayed (box_grad.h: image_shift, shared with PME's direct term).  Only the box
// terms need it.
//
// A slot is used when both of its atoms lie in [0, num_atoms) (-1: unused); an unused slot contributes nothing to any output.  A used
// slot with r = 0 divides by zero, as the first-order kernels do: its NaN stays in its own outputs (and in grad_B, which sums them all).
// No atomics: the double backward writes every output of its slot; the box gradient is a fixed-order float64 sum over fixed blocks,
// then one workgroup over the blocks in a fixed order -- bitwise reproducible, no host synchronisation, capturable.
#include "box_grad.h"
#include "device_common.h"
#include "host_common.h"

using namespace nnpops;

namespace {

__device__ __forceinline__ bool used_slot(int i, int j, int num_atoms) { return (unsigned)i < (unsigned)num_atoms && (unsigned)j < (unsigned)num_atoms; }

// one lane per slot; BOX: h_B is given (then positions and box are read for n_k)
template <typename T, bool BOX>
__global__ __launch_bounds__(256) void pairs_double_backward(long long num_slots, int num_atoms, const int32_t* __restrict__ neighbors,
                                                             const T* __restrict__ pos, const T* __restrict__ box,
                                                             const T* __restrict__ deltas, const T* __restrict__ distances,
                                                             const T* __restrict__ grad_distances, const T* __restrict__ gg_positions,
                                                             const T* __restrict__ gg_box, T* __restrict__ d_grad_deltas,
                                                             T* __restrict__ d_grad_distances, T* __restrict__ d_deltas,
                                                             T* __restrict__ d_distances) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= num_slots) return;
    const int i = neighbors[k], j = neighbors[num_slots + k];
    T w[3] = {T(0), T(0), T(0)}, a = T(0), b[3] = {T(0), T(0), T(0)}, c = T(0);
    if (used_slot(i, j, num_atoms)) {
        const T dx = deltas[3 * k], dy = deltas[3 * k + 1], dz = deltas[3 * k + 2], r = distances[k], g = grad_distances[k];
        if (gg_positions) {
#pragma unroll
            for (int q = 0; q < 3; q++) w[q] = gg_positions[3 * i + q] - gg_positions[3 * j + q];
        }
        if (BOX) {
            T n[3];
            image_shift(pos, i, j, dx, dy, dz, box, n);
#pragma unroll
            for (int q = 0; q < 3; q++) w[q] -= n[0] * gg_box[q] + n[1] * gg_box[3 + q] + n[2] * gg_box[6 + q];
        }
        const T dw = dx * w[0] + dy * w[1] + dz * w[2];
        const T inv = T(1) / r;
        a = dw * inv;                               // u.w
        const T s = g * inv;
#pragma unroll
        for (int q = 0; q < 3; q++) b[q] = s * w[q];     // (g_r / r) w
        c = -s * dw * inv;                          // -g_r (delta.w) / r^2
    }
#pragma unroll
    for (int q = 0; q < 3; q++) { d_grad_deltas[3 * k + q] = w[q]; d_deltas[3 * k + q] = b[q]; }
    d_grad_distances[k] = a;
    d_distances[k] = c;
}

// grad_B = - sum_k n_k (x) G_k: block b adds up slots b*256 + t, then strides of gridDim*256 (float64) and writes its 9 partial sums
// (box_grad.h: box_block_sum9)
template <typename T>
__global__ __launch_bounds__(kBoxThreads) void pairs_box_partials(long long num_slots, int num_atoms, const int32_t* __restrict__ neighbors,
                                                                  const T* __restrict__ pos, const T* __restrict__ box,
                                                                  const T* __restrict__ deltas, const T* __restrict__ distances,
                                                                  const T* __restrict__ grad_deltas, const T* __restrict__ grad_distances,
                                                                  double* __restrict__ partials) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    for (long long k = (long long)blockIdx.x * kBoxThreads + threadIdx.x; k < num_slots; k += (long long)gridDim.x * kBoxThreads) {
        const int i = neighbors[k], j = neighbors[num_slots + k];
        if (!used_slot(i, j, num_atoms)) continue;
        const T dx = deltas[3 * k], dy = deltas[3 * k + 1], dz = deltas[3 * k + 2];
        const T gd = grad_distances[k] / distances[k];               // (the first-order kernels' G, bit for bit)
        const T G[3] = {grad_deltas[3 * k] + dx * gd, grad_deltas[3 * k + 1] + dy * gd, grad_deltas[3 * k + 2] + dz * gd};
        T n[3];
        image_shift(pos, i, j, dx, dy, dz, box, n);
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int q = 0; q < 3; q++) acc[3 * a + q] -= (double)n[a] * (double)G[q];
    }
    box_block_sum9(acc, partials + (size_t)blockIdx.x * 9);
}

// (the blocks are added up by box_grad.h: pairs_box_finish)

template <typename T>
void launch_double_backward(long long num_slots, int num_atoms, const int32_t* neighbors, const void* positions, const void* box,
                            const void* deltas, const void* distances, const void* grad_distances, const void* gg_positions,
                            const void* gg_box, void* d_grad_deltas, void* d_grad_distances, void* d_deltas, void* d_distances,
                            hipStream_t s) {
    const dim3 grid((unsigned)((num_slots + 255) / 256)), block(256);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, num_slots, num_atoms, neighbors, (const T*)positions, (const T*)box, (const T*)deltas,
                           (const T*)distances, (const T*)grad_distances, (const T*)gg_positions, (const T*)gg_box, (T*)d_grad_deltas,
                           (T*)d_grad_distances, (T*)d_deltas, (T*)d_distances);
    };
    if (gg_box) launch(pairs_double_backward<T, true>);
    else launch(pairs_double_backward<T, false>);
}

template <typename T>
void launch_box_backward(long long num_slots, int num_atoms, const int32_t* neighbors, const void* positions, const void* box,
                         const void* deltas, const void* distances, const void* grad_deltas, const void* grad_distances, void* grad_box,
                         double* partials, hipStream_t s) {
    const int nblocks = box_blocks(num_slots);
    hipLaunchKernelGGL(pairs_box_partials<T>, dim3(nblocks), dim3(kBoxThreads), 0, s, num_slots, num_atoms, neighbors, (const T*)positions,
                       (const T*)box, (const T*)deltas, (const T*)distances, (const T*)grad_deltas, (const T*)grad_distances, partials);
    hipLaunchKernelGGL(pairs_box_finish<T>, dim3(1), dim3(kBoxThreads), 0, s, nblocks, (const double*)partials, (T*)grad_box);
}

}  // namespace

extern "C" {

int nnpops_neighbor_pairs_double_backward(int dtype, int num_atoms, int64_t num_slots, const int32_t* neighbors, const void* positions,
                                          const void* box, const void* deltas, const void* distances, const void* grad_distances,
                                          const void* gg_positions, const void* gg_box, void* d_grad_deltas, void* d_grad_distances,
                                          void* d_deltas, void* d_distances, void* stream) {
    NNPOPS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (float32) or 1 (float64)");
    NNPOPS_REQUIRE(num_atoms > 0 && num_slots >= 0, "bad sizes");
    NNPOPS_REQUIRE(gg_box == nullptr || (positions && box), "gg_box needs positions and box");
    NNPOPS_REQUIRE(num_slots == 0 || (neighbors && deltas && distances && grad_distances && d_grad_deltas && d_grad_distances && d_deltas &&
                                      d_distances), "NULL device pointer");
    if (num_slots == 0) return NNPOPS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        launch_double_backward<float>(num_slots, num_atoms, neighbors, positions, box, deltas, distances, grad_distances, gg_positions, gg_box,
                                      d_grad_deltas, d_grad_distances, d_deltas, d_distances, s);
    else
        launch_double_backward<double>(num_slots, num_atoms, neighbors, positions, box, deltas, distances, grad_distances, gg_positions, gg_box,
                                       d_grad_deltas, d_grad_distances, d_deltas, d_distances, s);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int64_t nnpops_neighbor_pairs_box_backward_workspace_bytes(int64_t num_slots) {
    if (num_slots < 0) return 0;
    return (int64_t)sizeof(double) * 9 * box_blocks(num_slots);
}

int nnpops_neighbor_pairs_box_backward(int dtype, int num_atoms, int64_t num_slots, const int32_t* neighbors, const void* positions,
                                       const void* box, const void* deltas, const void* distances, const void* grad_deltas,
                                       const void* grad_distances, void* grad_box, void* workspace, void* stream) {
    NNPOPS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (float32) or 1 (float64)");
    NNPOPS_REQUIRE(num_atoms > 0 && num_slots >= 0, "bad sizes");
    NNPOPS_REQUIRE(grad_box != nullptr && workspace != nullptr, "NULL device pointer");
    NNPOPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "the workspace must be 8-byte aligned");
    NNPOPS_REQUIRE(num_slots == 0 || (neighbors && positions && box && deltas && distances && grad_deltas && grad_distances), "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        launch_box_backward<float>(num_slots, num_atoms, neighbors, positions, box, deltas, distances, grad_deltas, grad_distances, grad_box,
                                   (double*)workspace, s);
    else
        launch_box_backward<double>(num_slots, num_atoms, neighbors, positions, box, deltas, distances, grad_deltas, grad_distances, grad_box,
                                    (double*)workspace, s);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // extern "C"
