// cfconv_box_grad.h -- box-vector gradient (virial) of the periodic CFConv: one pass over what backprop() leaves behind.
//
// Every displacement the convolution uses is d_ij = x_j - x_i + n_ij B (B: rows = box vectors, n_ij in Z^3 the minimum-image shift
// the builder chose, held fixed), and the backward pass forms one scalar per pair with dL/dd_ij = s_ij d_ij (dL/dpos[i] =
// -sum_e s_e delta_e, cfconv_gather), so
//     dL/dB[k][c] = sum over half pairs i < j of  n_ij,k s_ij (d_ij)_c
// One wave per atom walks the atom's row, a lane per neighbour, and takes the entries whose partner id is above its own: the pairs
// whose slots the row owns, each once, as the half list counts them.  Where the pair scalar comes from is the only difference between
// the two layouts:
//   ROW_S = false   the half-list paths (every matrix-core filters kernel): s = pair_s[pid[i][e]]; an entry whose mirror image is
//                   missing points at the all-zero slot behind the last pair and adds nothing
//   ROW_S = true    the vector kernel has no half list: a second walk of it, launched by box-gradient calls only, stores the scalar
//                   of every row entry, s = row_s[i][e] (cfconv_kernel<..., ROW_S>, cfconv_fallback_kernels.h)
// n is RECOVERED (box_grad.h: image_shift) from the positions, the stored displacement and the box -- exact whatever rounding the
// builder's minimum image took, whether or not the cell grid wrapped the atoms -- and a pair with n = 0, which is most of them, ends
// there.  Products and sums in float64; the 9 sums of a workgroup by box_block_sum9, the workgroups by pairs_box_finish: the number of
// partial sums is a function of the number of atoms alone, no atomics, two calls agree bit for bit.  Included by cfconv.hip only.
#pragma once

#include "box_grad.h"
#include "celllist.h"

namespace nnpops {

constexpr int kConvBoxWaves = kBoxThreads / 64;      // atoms in flight per workgroup

inline int cfconv_box_blocks(int num_atoms) { return std::max(1, std::min(div_up(num_atoms, kConvBoxWaves), kBoxMaxBlocks)); }

template <bool ROW_S>
__global__ __launch_bounds__(kBoxThreads) void cfconv_box_partials(
    int N, const float* __restrict__ pos, const float* __restrict__ box, const float4* __restrict__ rows, const int* __restrict__ cnt,
    int cap, const int* __restrict__ pid, int pair_cap,
    const float* __restrict__ s,               // ROW_S: [N][cap] by row entry, else [pair_cap + 1] by pair slot
    const float4* __restrict__ sorted_pos,     // atoms in cell order (id in .w), or NULL
    double* __restrict__ partials) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    const int lane = lane_id();
    for (int w = blockIdx.x * kConvBoxWaves + wave_in_group(); w < N; w += gridDim.x * kConvBoxWaves) {
        const int i = sorted_pos ? __float_as_int(sorted_pos[w].w) & kIdMask : w;
        if (i >= N) continue;                               // (a grid that could not be built: check() reports it)
        const int n_row = min(cnt[i], cap);                 // (an overflowed build stays in bounds and is incomplete, as its forces are)
        const size_t base = (size_t)i * cap;
        for (int e = lane; e < n_row; e += 64) {
            const float4 rec = rows[base + e];
            const int j = __float_as_int(rec.w) & kIdMask;
            if (j <= i || j >= N) continue;                 // the other end's row owns this pair
            float n[3];
            image_shift(pos, i, j, -rec.x, -rec.y, -rec.z, box, n);
            if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) continue;
            float sc;
            if (ROW_S) {
                sc = s[base + e];
            } else {
                const int p = pid[base + e];
                if ((unsigned)p > (unsigned)pair_cap) continue;
                sc = s[p];
            }
            const double G[3] = {(double)sc * (double)rec.x, (double)sc * (double)rec.y, (double)sc * (double)rec.z};
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int q = 0; q < 3; q++) acc[3 * a + q] += (double)n[a] * G[q];
        }
    }
    box_block_sum9(acc, partials + (size_t)blockIdx.x * 9);
}

}  // namespace nnpops
