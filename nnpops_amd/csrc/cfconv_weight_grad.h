// cfconv_weight_grad.h -- dL/d(weights1, biases1, weights2, biases2) of the CFConv filter network (nnpops_cfconv_backprop_weights).
//
// For a half pair p = (i < j) at stored distance r, with upstream gradient g = dL/dout:
//     gamma_g = exp(-((r - mu_g)/sigma)^2 / 2)      z_a = b1_a + sum_g w1[a][g] gamma_g      y_a = act(z_a)
//     s_c = fc(r) (g[i][c] x[j][c] + g[j][c] x[i][c])
//     db2[c] = sum_p s_c                             dw2[c][a] = sum_p s_c y_a
//     t_a = act'(z_a) sum_c s_c w2[c][a]             db1[a] = sum_p t_a          dw1[a][g] = sum_p t_a gamma_g
// Only the list's stored distances, x and g are read: periodic and batched lists need nothing of their own.
//
// Every workgroup walks a fixed, contiguous slice of the pair slots in tiles of kWgradTile, recomputes Gamma, Y, S and T of the tile
// in fp32 into LDS, and adds the two outer products S^T Y and T^T Gamma and the two column sums to its own partial row
//     [dw1 W x G | db1 W | dw2 W x W | db2 W]
// of `partials`.  No atomics: cfconv_wgrad_finish then adds the rows in block order in float64.  Slots past the list's count carry
// fc = 0, hence S = T = 0: they contribute exact zeros, and a list without pairs gives exact zeros.
//   cfconv_wgrad_mfma     W a multiple of 16 up to 128 with both weight matrices in LDS: everything on v_mfma_f32_16x16x4_f32 (exact fp32
//                         products, fp32 accumulation).  One wave per 16-wide block of filters: wave w evaluates columns 16w .. 16w+15 of
//                         Z, Y, S, T for the tile, then owns ROWS 16w .. 16w+15 of dw2 and dw1 as accumulators in registers.
//   cfconv_wgrad_vector   every other layer: weights streamed through the caches, the partial row accumulated in place by the thread
//                         that owns each entry.  Functional, not tuned.
// Included by cfconv.hip only.
#pragma once

#include "cfconv_fallback_kernels.h"

namespace {
using namespace nnpops;

constexpr int kWgradTile = 16;          // pair slots per tile, both kernels
constexpr int kWgradVectorThreads = 512;

__host__ __device__ inline size_t wgrad_row_floats(int W, int G) { return (size_t)W * ((size_t)W + G + 2); }

// ---- matrix-core kernel ----------------------------------------------------------------------------------------------------------
// LDS: W2 [out][in] | W1^T [Gp][W] | Y, S, T tiles [16][W + 16] | Gamma tile [16][16 NGB] | r, fc, i, j of the tile
__host__ __device__ inline int wgrad_gamma_blocks(int G) { return G <= 64 ? 4 : 16; }      // the kernel's NGB: 16-wide blocks of Gaussians
__host__ __device__ inline size_t wgrad_mfma_floats(int W, int G) {
    const size_t Gp = (size_t)(G + 3) & ~(size_t)3;
    return (size_t)W * W + Gp * W + (size_t)3 * kWgradTile * (W + 16) + (size_t)kWgradTile * 16 * wgrad_gamma_blocks(G) + 4 * kWgradTile;
}

template <int NCB, int NGB>
__global__ __launch_bounds__(64 * NCB) void cfconv_wgrad_mfma(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2,
    const int* __restrict__ half_off, const float* __restrict__ half_r, const int2* __restrict__ half_ij, int pair_cap,
    const float* __restrict__ x, const float* __restrict__ gout, float* __restrict__ partials) {
    constexpr int W = NCB * 16, TS = W + 16, GS = NGB * 16, TP = kWgradTile;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int G = P.G, Gp = (G + 3) & ~3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* s_w2 = lds;                                      // [c][a]: the core layout
    float* s_w1t = s_w2 + W * W;                            // [g][a]
    float* tY = s_w1t + Gp * W;
    float* tS = tY + TP * TS;
    float* tT = tS + TP * TS;
    float* tG = tT + TP * TS;                               // [pair][GS]; columns G .. GS-1 stay zero
    float* ps = tG + TP * GS;                               // r | fc | i | j, 16 each
    for (int q = tid; q < W * W; q += blockDim.x) s_w2[q] = w2[q];
    for (int q = tid; q < Gp * W; q += blockDim.x) s_w1t[q] = q < G * W ? w1t[q] : 0.f;
    for (int q = tid; q < TP * GS; q += blockDim.x) tG[q] = 0.f;

    const int col = lane & 15, grp = lane >> 4;
    const int mycol = wave * 16 + col;                      // my column of Z / Y / S / T; my row offset of the accumulators is 16 * wave
    const float b1v = b1[mycol];
    const float mu_step = P.cutoff / (float)(G - 1);
    const float gscale = -0.5f * kLog2e * P.sigma_inv * P.sigma_inv;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc2[NCB], acc1[NGB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) acc2[cb] = zero;
#pragma unroll
    for (int gb = 0; gb < NGB; gb++) acc1[gb] = zero;
    float sum_s = 0.f, sum_t = 0.f;                         // my share of db2[mycol], db1[mycol]: pairs 4 grp .. 4 grp + 3 of every tile

    const int pairs = min(half_off[P.N], pair_cap);
    const int tiles = (pairs + TP - 1) / TP;
    const int per_block = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t_end = min(tiles, ((int)blockIdx.x + 1) * per_block);
    __syncthreads();                                        // the weights are in
    for (int t = blockIdx.x * per_block; t < t_end; t++) {
        // (no barrier here: the last tile's products do not read `ps`, and nothing else is written before the next barrier)
        if (tid < TP) {
            const int p = TP * t + tid;
            float r = 1.0f, fc = 0.f;
            int2 ij = make_int2(0, 0);
            if (p < pairs) {
                r = half_r[p];
                ij = half_ij[p];
                fc = 0.5f * cospif(r / P.cutoff) + 0.5f;
            }
            ps[tid] = r; ps[16 + tid] = fc;
            ps[32 + tid] = __int_as_float(ij.x); ps[48 + tid] = __int_as_float(ij.y);
        }
        __syncthreads();
        // ---- Z = b1 + Gamma W1^T, my 16 columns; the Gaussians straight in operand layout (pair = col, g = 4 s + grp) ----
        f32x4 z = f32x4{b1v, b1v, b1v, b1v};
        const float rp = ps[col];
        for (int s = 0; s < Gp / 4; s++) {
            const int g = 4 * s + grp;
            const float d = rp - (float)g * mu_step;
            const float a = g < G ? fast_exp2(gscale * d * d) : 0.f;
            if (s % NCB == wave && g < G) tG[col * GS + g] = a;
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_w1t[g * W + mycol], z, 0, 0, 0);
        }
        // ---- Y, act', S in result layout: pair = 4 grp + q, column = mycol ----
        f32x4 dact;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int pr = 4 * grp + q;
            float yv, dv;
            if (P.activation == 0) activate_d<0>(z[q], yv, dv); else activate_d<1>(z[q], yv, dv);
            dact[q] = dv;
            tY[pr * TS + mycol] = yv;
            const float fc = ps[16 + pr];
            float sv = 0.f;
            if (fc != 0.f) {                                // (uniform over the 16 lanes of a pair; empty slots gather nothing)
                const size_t i = (size_t)__float_as_int(ps[32 + pr]), j = (size_t)__float_as_int(ps[48 + pr]);
                sv = fc * (gout[i * W + mycol] * x[j * W + mycol] + gout[j * W + mycol] * x[i * W + mycol]);
            }
            tS[pr * TS + mycol] = sv;
            sum_s += sv;
        }
        __syncthreads();
        // ---- U = S W2, my 16 columns; T = act' U ----
        f32x4 u = zero;
        {
            const float* a_lane = tS + col * TS + grp;
            const float* b_lane = s_w2 + grp * W + mycol;
#pragma unroll 4
            for (int s = 0; s < W / 4; s++) u = __builtin_amdgcn_mfma_f32_16x16x4f32(a_lane[4 * s], b_lane[4 * s * W], u, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float tv = dact[q] * u[q];
            tT[(4 * grp + q) * TS + mycol] = tv;
            sum_t += tv;
        }
        __syncthreads();
        // ---- dw2[16 wave + row][:] += S^T Y and dw1[16 wave + row][:] += T^T Gamma: K = the tile's pairs ----
#pragma unroll
        for (int s = 0; s < TP / 4; s++) {
            const int pr = 4 * s + grp;
            const float sa = tS[pr * TS + mycol], ta = tT[pr * TS + mycol];
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) acc2[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa, tY[pr * TS + cb * 16 + col], acc2[cb], 0, 0, 0);
#pragma unroll
            for (int gb = 0; gb < NGB; gb++) acc1[gb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta, tG[pr * GS + gb * 16 + col], acc1[gb], 0, 0, 0);
        }
    }
    // ---- my partial row (every entry written, also by a workgroup without tiles) ----
    float* row = partials + (size_t)blockIdx.x * wgrad_row_floats(W, G);
    float* p_w1 = row;
    float* p_b1 = p_w1 + (size_t)W * G;
    float* p_w2 = p_b1 + W;
    float* p_b2 = p_w2 + (size_t)W * W;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = wave * 16 + 4 * grp + q;              // result layout: D[row = 4 grp + q][col]
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) p_w2[(size_t)r * W + cb * 16 + col] = acc2[cb][q];
#pragma unroll
        for (int gb = 0; gb < NGB; gb++)
            if (gb * 16 + col < G) p_w1[(size_t)r * G + gb * 16 + col] = acc1[gb][q];
    }
    sum_s += __shfl_xor(sum_s, 16, 64); sum_s += __shfl_xor(sum_s, 32, 64);
    sum_t += __shfl_xor(sum_t, 16, 64); sum_t += __shfl_xor(sum_t, 32, 64);
    if (grp == 0) { p_b2[mycol] = sum_s; p_b1[mycol] = sum_t; }
}

// ---- vector kernel ---------------------------------------------------------------------------------------------------------------
// LDS: Y, S, T tiles [16][W] | Gamma tile [16][G] | r, fc, i, j of the tile
__host__ __device__ inline size_t wgrad_vector_floats(int W, int G) { return (size_t)kWgradTile * (3 * (size_t)W + G) + 4 * kWgradTile; }

__global__ __launch_bounds__(kWgradVectorThreads) void cfconv_wgrad_vector(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2,
    const int* __restrict__ half_off, const float* __restrict__ half_r, const int2* __restrict__ half_ij, int pair_cap,
    const float* __restrict__ x, const float* __restrict__ gout, float* __restrict__ partials) {
    constexpr int TP = kWgradTile;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int W = P.W, G = P.G, tid = threadIdx.x, nthreads = blockDim.x;
    float* tY = lds;
    float* tS = tY + TP * W;
    float* tT = tS + TP * W;                                // act' first, then T
    float* tG = tT + TP * W;
    float* ps = tG + TP * G;
    const float mu_step = P.cutoff / (float)(G - 1);
    const float gscale = -0.5f * kLog2e * P.sigma_inv * P.sigma_inv;
    const int n_w1 = W * G, n_w2 = W * W, row_len = W * (W + G + 2);
    float* row = partials + (size_t)blockIdx.x * row_len;   // dw1 | db1 | dw2 | db2, each entry owned by one thread
    for (int e = tid; e < row_len; e += nthreads) row[e] = 0.f;

    const int pairs = min(half_off[P.N], pair_cap);
    const int tiles = (pairs + TP - 1) / TP;
    const int per_block = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t_end = min(tiles, ((int)blockIdx.x + 1) * per_block);
    for (int t = blockIdx.x * per_block; t < t_end; t++) {
        // (no barrier here: the last tile's sums do not read `ps`, and nothing else is written before the next barrier)
        if (tid < TP) {
            const int p = TP * t + tid;
            float r = 1.0f, fc = 0.f;
            int2 ij = make_int2(0, 0);
            if (p < pairs) {
                r = half_r[p];
                ij = half_ij[p];
                fc = 0.5f * cospif(r / P.cutoff) + 0.5f;
            }
            ps[tid] = r; ps[16 + tid] = fc;
            ps[32 + tid] = __int_as_float(ij.x); ps[48 + tid] = __int_as_float(ij.y);
        }
        __syncthreads();
        for (int e = tid; e < TP * G; e += nthreads) {
            const int pr = e / G, g = e - pr * G;
            const float d = ps[pr] - (float)g * mu_step;
            tG[e] = fast_exp2(gscale * d * d);
        }
        __syncthreads();
        for (int e = tid; e < TP * W; e += nthreads) {      // Y, act', S
            const int pr = e / W, a = e - pr * W;
            float z = b1[a];
            for (int g = 0; g < G; g++) z = fmaf(w1t[(size_t)g * W + a], tG[pr * G + g], z);
            float yv, dv;
            if (P.activation == 0) activate_d<0>(z, yv, dv); else activate_d<1>(z, yv, dv);
            tY[e] = yv;
            tT[e] = dv;
            const float fc = ps[16 + pr];
            float sv = 0.f;
            if (fc != 0.f) {
                const size_t i = (size_t)__float_as_int(ps[32 + pr]), j = (size_t)__float_as_int(ps[48 + pr]);
                sv = fc * (gout[i * W + a] * x[j * W + a] + gout[j * W + a] * x[i * W + a]);
            }
            tS[e] = sv;
        }
        __syncthreads();
        for (int e = tid; e < TP * W; e += nthreads) {      // T = act' (S W2)
            const int pr = e / W, a = e - pr * W;
            float u = 0.f;
            for (int c = 0; c < W; c++) u = fmaf(tS[pr * W + c], w2[(size_t)c * W + a], u);
            tT[e] *= u;
        }
        __syncthreads();
        for (int e = tid; e < row_len; e += nthreads) {     // the tile's share of every entry, added in place by its owner
            float sum = 0.f;
            if (e < n_w1) {
                const int a = e / G, g = e - a * G;
                for (int pr = 0; pr < TP; pr++) sum = fmaf(tT[pr * W + a], tG[pr * G + g], sum);
            } else if (e < n_w1 + W) {
                const int a = e - n_w1;
                for (int pr = 0; pr < TP; pr++) sum += tT[pr * W + a];
            } else if (e < n_w1 + W + n_w2) {
                const int q = e - n_w1 - W, c = q / W, a = q - c * W;
                for (int pr = 0; pr < TP; pr++) sum = fmaf(tS[pr * W + c], tY[pr * W + a], sum);
            } else {
                const int c = e - n_w1 - W - n_w2;
                for (int pr = 0; pr < TP; pr++) sum += tS[pr * W + c];
            }
            row[e] += sum;
        }
    }
}

// The sum of the workgroups' rows, in block order, in float64; stored as float32 into the four arrays of the caller.
__global__ __launch_bounds__(256) void cfconv_wgrad_finish(int W, int G, int nblocks, const float* __restrict__ partials,
                                                            float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                            float* __restrict__ db2) {
    const int n_w1 = W * G, n_w2 = W * W, row_len = W * (W + G + 2);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= row_len) return;
    double sum = 0.0;
    for (int b = 0; b < nblocks; b++) sum += (double)partials[(size_t)b * row_len + e];
    const float v = (float)sum;
    if (e < n_w1) dw1[e] = v;
    else if (e < n_w1 + W) db1[e - n_w1] = v;
    else if (e < n_w1 + W + n_w2) dw2[e - n_w1 - W] = v;
    else db2[e - n_w1 - W - n_w2] = v;
}

}  // namespace
