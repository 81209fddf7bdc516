// box_grad.h -- what the box-gradient passes over a pair list share: the pair list's own (pairs_second_order.hip) and that of
// PME's direct term (pme.hip).  Both form grad_B = - sum_k n_k (x) G_k over the used slots k, with n_k in Z^3 the slot's
// minimum-image shift, as 9 float64 partial sums per block (box_block_sum9); pairs_box_finish adds the blocks up in the same order.
//
// n_k is RECOVERED from what the list stores, not replayed: D = x_i - x_j - delta_k is an integer combination of the rows of the
// lower-triangular box, so n_z = round(D_z / B_zz), n_y = round((D_y - n_z B_zy) / B_yy), n_x = round((D_x - n_z B_zx - n_y B_yx) / B_xx)
// -- exact whatever rounding choices (ties, reciprocal multiplies) the forward made.
#pragma once

#include <algorithm>

#include "device_common.h"
#include "host_common.h"

namespace nnpops {
namespace {

constexpr int kBoxThreads = 256;
constexpr int kBoxMaxBlocks = 1024;      // partial sums per call: a function of num_slots alone (the order of the sums is fixed)

int box_blocks(long long num_slots) { return (int)std::max<long long>(1, std::min<long long>(div_up(num_slots, kBoxThreads), kBoxMaxBlocks)); }

// n_k of the slot: box rows a = (B00, 0, 0), b = (B10, B11, 0), c = (B20, B21, B22) as the forward op uses them
template <typename T>
__device__ __forceinline__ void image_shift(const T* __restrict__ pos, int i, int j, T dx, T dy, T dz, const T* __restrict__ box, T (&n)[3]) {
    const T Dx = (pos[3 * i] - pos[3 * j]) - dx, Dy = (pos[3 * i + 1] - pos[3 * j + 1]) - dy, Dz = (pos[3 * i + 2] - pos[3 * j + 2]) - dz;
    n[2] = round(Dz / box[8]);
    n[1] = round((Dy - n[2] * box[7]) / box[4]);
    n[0] = round((Dx - n[2] * box[6] - n[1] * box[3]) / box[0]);
}

// The 9 sums of a workgroup of kBoxThreads lanes, in ONE fixed order shared by every box pass: a xor tree over each wave, then the
// four waves in order; lane q < 9 stores sum q to out[q] (converted to T).  Every lane of the workgroup must call it.
template <typename T>
__device__ __forceinline__ void box_block_sum9(double (&acc)[9], T* __restrict__ out) {
    __shared__ double red[kBoxThreads / 64][9];
#pragma unroll
    for (int q = 0; q < 9; q++)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 9; q++) red[wave][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < kBoxThreads / 64; w++) s += red[w][threadIdx.x];
        out[threadIdx.x] = (T)s;
    }
}

// one workgroup: lane t adds up partials t, t + 256, ... of each of the 9 sums, then box_block_sum9
template <typename T>
__global__ __launch_bounds__(kBoxThreads) void pairs_box_finish(int nblocks, const double* __restrict__ partials, T* __restrict__ grad_box) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kBoxThreads) {
#pragma unroll
        for (int q = 0; q < 9; q++) acc[q] += partials[(size_t)b * 9 + q];
    }
    box_block_sum9(acc, grad_box);
}

}  // namespace
}  // namespace nnpops
