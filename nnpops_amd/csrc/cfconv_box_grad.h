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

// What one wave adds for atom i: the entries of its row whose partner id is above its own, shifts recovered against `box`.
template <bool ROW_S>
__device__ __forceinline__ void cfconv_box_atom(int N, const float* __restrict__ pos, const float* __restrict__ box,
                                                const float4* __restrict__ rows, const int* __restrict__ cnt, int cap,
                                                const int* __restrict__ pid, int pair_cap, const float* __restrict__ s, int i,
                                                double (&acc)[9]) {
    const int lane = lane_id();
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
    for (int w = blockIdx.x * kConvBoxWaves + wave_in_group(); w < N; w += gridDim.x * kConvBoxWaves) {
        const int i = sorted_pos ? __float_as_int(sorted_pos[w].w) & kIdMask : w;
        if (i >= N) continue;                               // (a grid that could not be built: check() reports it)
        cfconv_box_atom<ROW_S>(N, pos, box, rows, cnt, cap, pid, pair_cap, s, i, acc);
    }
    box_block_sum9(acc, partials + (size_t)blockIdx.x * 9);
}

// Periodic frames (nnpops_cfconv_neighbors_set_frames): the same pass with one box and one sum per frame, laid out as the ANI pass
// lays out its molecules (ani_box_grad.h).  A frame of n atoms is dealt to cfconv_box_frame_blocks(n) workgroups -- a function of n
// alone -- whose waves stride over its atoms [offsets[m], offsets[m + 1]) in index order (frames never use the cell order), every
// shift recovered against boxes + 9 m; workgroup k of the frame leaves its nine float64 sums at partials[first_block[m] + k], and
// cfconv_box_finish_frames, one workgroup per frame, adds them in the order of pairs_box_finish and writes box_deriv[m].  No atomics;
// the order of every sum depends on the frame's atom count alone, so two calls agree bit for bit and a frame's nine entries do not
// depend on its companions or on its place in the batch.  `blocks` (one {frame, k} per workgroup), `first_block` and `offsets` belong
// to the neighbour list (sized and uploaded by nnpops_cfconv_neighbors_set_frames).  (One workgroup per frame was measured for the
// ANI pass and cost ~185 us at 192 atoms whatever the batch: not repeated here.)
constexpr int kConvBoxFrameBlocks = 64;      // a frame's stride is at most 64 * kConvBoxWaves = 256 atoms

__host__ __device__ inline int cfconv_box_frame_blocks(int num_atoms) {
    const int want = (num_atoms + kConvBoxWaves - 1) / kConvBoxWaves;
    return want < 1 ? 1 : want > kConvBoxFrameBlocks ? kConvBoxFrameBlocks : want;
}

template <bool ROW_S>
__global__ __launch_bounds__(kBoxThreads) void cfconv_box_partials_frames(
    int N, const float* __restrict__ pos, const float* __restrict__ boxes, const int* __restrict__ offsets,
    const int2* __restrict__ blocks, const float4* __restrict__ rows, const int* __restrict__ cnt, int cap, const int* __restrict__ pid,
    int pair_cap, const float* __restrict__ s, double* __restrict__ partials) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    const int2 mine = blocks[blockIdx.x];                   // wave-uniform: the frame, its range and its box through scalar loads
    const int m = mine.x;
    const int lo = max(offsets[m], 0), hi = min(offsets[m + 1], N);
    const int stride = cfconv_box_frame_blocks(hi - lo) * kConvBoxWaves;
    const float* box = boxes + 9 * (size_t)m;
    for (int i = lo + mine.y * kConvBoxWaves + wave_in_group(); i < hi; i += stride)
        cfconv_box_atom<ROW_S>(hi, pos, box, rows, cnt, cap, pid, pair_cap, s, i, acc);      // (N = hi: no partner beyond the frame)
    box_block_sum9(acc, partials + (size_t)blockIdx.x * 9);
}

// one workgroup per frame: lane t adds up the frame's partial sums t, t + 256, ..., then box_block_sum9 (cf. pairs_box_finish)
__global__ __launch_bounds__(kBoxThreads) void cfconv_box_finish_frames(const int* __restrict__ first_block, const double* __restrict__ partials,
                                                                       float* __restrict__ box_deriv) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    const int m = blockIdx.x;
    for (int b = first_block[m] + threadIdx.x; b < first_block[m + 1]; b += kBoxThreads) {
#pragma unroll
        for (int q = 0; q < 9; q++) acc[q] += partials[(size_t)b * 9 + q];
    }
    box_block_sum9(acc, box_deriv + 9 * (size_t)m);
}

}  // namespace nnpops
