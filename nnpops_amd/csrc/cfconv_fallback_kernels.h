// cfconv_fallback_kernels.h -- the CFConv kernels for the shapes and weights the default filters kernels (cfconv_filters.h) do not take.
//
//   cfconv_kernel         vector kernel, one wave per atom: widths that are not a multiple of 16, widths above 128 (weights streamed
//                         through the caches), weights of the matrix-core kernels that do not fit in LDS, or $NNPOPS_CFCONV_VALU=1
//                         (its ROW_S instantiations, launched by box-gradient calls only, store the pair scalar of every row entry)
//   cfconv_filters_mfma   filters on the fp32 matrix instruction: widths 16, 48, 80, 112, weights outside the fp16 range, or
//                         $NNPOPS_CFCONV_SPLIT=0
//   cfconv_filters_h2     filters with layer 2 as split-fp16 products through LDS planes: widths 32, 64, 96 with more than 63 Gaussians,
//                         width 128 with more than 55 (and up to 171), or $NNPOPS_CFCONV_SPLIT=1
// Both filters kernels feed cfconv_gather.  Included by cfconv.hip only.
#pragma once

#include <type_traits>

#include "cfconv_filters.h"

namespace {
using namespace nnpops;

template <int ACT>
__device__ __forceinline__ float activate(float s) {
    if (ACT == 0) return logf(0.5f * expf(s) + 0.5f);      // ref :163
    return tanhf(s);
}
// activation and its derivative in one go
template <int ACT>
__device__ __forceinline__ void activate_d(float s, float& y, float& dy) {
    if (ACT == 0) {
        const float e = expf(s);
        y = logf(0.5f * e + 0.5f);
        dy = e / (e + 1.0f);                               // ref :254-257
    } else {
        const float th = tanhf(s);
        y = th;
        dy = 1.0f - th * th;                               // ref :259-262
    }
}

// LDS: W2^T [W][W] | W1^T [G][W] | per wave: gam[G][8], y1[W][8], pair scalars [8][8] (+ dgam, dy1 backward)
__host__ __device__ inline size_t conv_weight_floats(int W, int G) {
    return ((size_t)W * W + (size_t)G * W + 3) & ~(size_t)3;          // keeps the per-wave slices 16-byte aligned
}
__host__ __device__ inline size_t conv_wave_floats(int W, int G, bool backward) {
    return (size_t)(backward ? 2 : 1) * ((size_t)G * kPairTile + (size_t)W * kPairTile) + 64;
}

// CPL = channels per lane (1: W <= 64, 2: W <= 128).  BACKWARD adds the d/dr path and the two gradients.
// WLDS = false: the weights do not fit in LDS next to one wave's tiles (W > 128): they are read through the
// caches instead.  Same arithmetic, a functional path for unusually wide layers, not a tuned one.
// ROW_S (box-gradient calls only, behind the backward pass proper): the same walk stores the pair scalar sc of every row entry to
// row_s[i][entry] for the box-gradient pass (cfconv_box_grad.h) and NOTHING else -- `out` and `pos_grad` are not written.  It is a
// second launch and not a flag on the backward pass itself because the gradients of a box-gradient call have to be those of a plain
// one to the bit: one more use of sc in the loop below makes the compiler pack and contract the force update differently (measured
// on the ISA: 8 of its 24 updates per tile change between v_pk_mul + v_sub and v_fma), so an instantiation that did both would give
// other last bits.  Every other instantiation ignores row_s (the host passes NULL) and is, instruction for instruction, what it was
// without the argument.
template <int ACT, int CPL, bool BACKWARD, bool WLDS = true, bool ROW_S = false>
__global__ __launch_bounds__(64 * kMaxWavesPerBlock) void cfconv_kernel(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2t,
    const float* __restrict__ b2, const float4* __restrict__ rows, const int* __restrict__ cnt, int cap,
    const float* __restrict__ x, const float* __restrict__ gout,   // gout: upstream gradient (backward only)
    float* __restrict__ out,                                       // forward: output ; backward: input gradient
    float* __restrict__ pos_grad, float* __restrict__ row_s) {
    static_assert(BACKWARD || !ROW_S, "the pair scalars belong to the backward pass");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int W = P.W, G = P.G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* s_w2t = WLDS ? lds : w2t;                // [W][W]   s_w2t[b*W + a] = w2[a][b]
    const float* s_w1t = WLDS ? lds + (size_t)W * W : w1t;   // [G][W]   s_w1t[g*W + a] = w1[a][g]
    const int waves_per_block = blockDim.x >> 6;
    float* wv = lds + (WLDS ? conv_weight_floats(W, G) : 0) + (size_t)wave * conv_wave_floats(W, G, BACKWARD);
    float* ps = wv;                                       // [8][8] per-pair scalars: r, fc, dfc, j, 1/r, dx, dy, dz
    float* gam = ps + 64;                                 // [G][8]
    float* y1b = gam + (size_t)G * kPairTile;             // [W][8]
    float* dgam = y1b + (size_t)W * kPairTile;            // [G][8]  (backward only)
    float* dy1b = dgam + (size_t)G * kPairTile;           // [W][8]  (backward only)

    if (WLDS) {
        for (int q = tid; q < W * W; q += blockDim.x) lds[q] = w2t[q];
        for (int q = tid; q < G * W; q += blockDim.x) lds[(size_t)W * W + q] = w1t[q];
        __syncthreads();
    }

    int ch[CPL];
    bool live[CPL];
    float bias1[CPL], bias2[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c++) {
        ch[c] = lane + 64 * c;
        live[c] = ch[c] < W;
        if (!live[c]) ch[c] = 0;
        bias1[c] = b1[ch[c]];
        bias2[c] = b2[ch[c]];
    }
    const float mu_step = P.cutoff / (float)(G - 1);       // ref :121-122

    for (int i = blockIdx.x * waves_per_block + wave; i < P.N; i += gridDim.x * waves_per_block) {
        const int n = min(cnt[i], cap);
        const float4* row = rows + (size_t)i * cap;
        float acc[CPL];
        float xi[CPL], gi[CPL];
#pragma unroll
        for (int c = 0; c < CPL; c++) {
            acc[c] = 0.f;
            xi[c] = BACKWARD ? x[(size_t)i * W + ch[c]] : 0.f;
            gi[c] = BACKWARD ? gout[(size_t)i * W + ch[c]] : 0.f;
        }
        float fx = 0.f, fy = 0.f, fz = 0.f;
        for (int t0 = 0; t0 < n; t0 += kPairTile) {
            const int np = min(kPairTile, n - t0);
            // ---- per-pair scalars (lanes 0..7) ----
            float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lane < np) rec = row[t0 + lane];
            if (lane < kPairTile) {
                const float r = lane < np ? sqrtf(rec.x * rec.x + rec.y * rec.y + rec.z * rec.z) : 1.0f;
                float sn, cs;
                sincospif(r / P.cutoff, &sn, &cs);
                ps[0 * 8 + lane] = r;
                ps[1 * 8 + lane] = lane < np ? 0.5f * cs + 0.5f : 0.f;                       // fc   (ref :301-303)
                ps[2 * 8 + lane] = lane < np ? -(0.5f * kPi / P.cutoff) * sn : 0.f;           // dfc  (ref :305-307)
                ps[3 * 8 + lane] = __int_as_float(lane < np ? (__float_as_int(rec.w) & kIdMask) : i);
                ps[4 * 8 + lane] = 1.0f / r;
                ps[5 * 8 + lane] = rec.x; ps[6 * 8 + lane] = rec.y; ps[7 * 8 + lane] = rec.z;
            }
            __builtin_amdgcn_wave_barrier();          // per-wave LDS slice: LDS ops of one wave execute in order
            // ---- Gaussians for the 8 pairs ----
            for (int q = lane; q < G * kPairTile; q += 64) {
                const int g = q >> 3, p = q & 7;
                const float xg = (ps[p] - (float)g * mu_step) * P.sigma_inv;
                const float gm = expf(-0.5f * xg * xg);                                       // ref :152-153
                gam[q] = gm;
                if (BACKWARD) dgam[q] = -xg * gm * P.sigma_inv;                                // ref :242
            }
            __builtin_amdgcn_wave_barrier();
            // ---- dense 1 + activation ----
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                float s[kPairTile], ds[kPairTile];
#pragma unroll
                for (int p = 0; p < kPairTile; p++) { s[p] = bias1[c]; ds[p] = 0.f; }
                for (int g = 0; g < G; g++) {
                    const float w = s_w1t[g * W + ch[c]];
                    const float4 ga = *reinterpret_cast<const float4*>(gam + g * 8), gb = *reinterpret_cast<const float4*>(gam + g * 8 + 4);
                    s[0] += ga.x * w; s[1] += ga.y * w; s[2] += ga.z * w; s[3] += ga.w * w;
                    s[4] += gb.x * w; s[5] += gb.y * w; s[6] += gb.z * w; s[7] += gb.w * w;
                    if (BACKWARD) {
                        const float4 da = *reinterpret_cast<const float4*>(dgam + g * 8), db = *reinterpret_cast<const float4*>(dgam + g * 8 + 4);
                        ds[0] += da.x * w; ds[1] += da.y * w; ds[2] += da.z * w; ds[3] += da.w * w;
                        ds[4] += db.x * w; ds[5] += db.y * w; ds[6] += db.z * w; ds[7] += db.w * w;
                    }
                }
                float yv[kPairTile], dyv[kPairTile];
#pragma unroll
                for (int p = 0; p < kPairTile; p++) {
                    if (BACKWARD) {
                        float dact;
                        activate_d<ACT>(s[p], yv[p], dact);
                        dyv[p] = ds[p] * dact;
                    } else {
                        yv[p] = activate<ACT>(s[p]);
                    }
                }
                if (live[c]) {
                    *reinterpret_cast<float4*>(y1b + ch[c] * 8) = make_float4(yv[0], yv[1], yv[2], yv[3]);
                    *reinterpret_cast<float4*>(y1b + ch[c] * 8 + 4) = make_float4(yv[4], yv[5], yv[6], yv[7]);
                    if (BACKWARD) {
                        *reinterpret_cast<float4*>(dy1b + ch[c] * 8) = make_float4(dyv[0], dyv[1], dyv[2], dyv[3]);
                        *reinterpret_cast<float4*>(dy1b + ch[c] * 8 + 4) = make_float4(dyv[4], dyv[5], dyv[6], dyv[7]);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            // ---- dense 2, cutoff, accumulate ----
            float scale_p[kPairTile];
#pragma unroll
            for (int p = 0; p < kPairTile; p++) scale_p[p] = 0.f;
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                float s[kPairTile], ds[kPairTile];
#pragma unroll
                for (int p = 0; p < kPairTile; p++) { s[p] = bias2[c]; ds[p] = 0.f; }
                for (int b = 0; b < W; b++) {
                    const float w = s_w2t[b * W + ch[c]];
                    const float4 ya = *reinterpret_cast<const float4*>(y1b + b * 8), yb = *reinterpret_cast<const float4*>(y1b + b * 8 + 4);
                    s[0] += ya.x * w; s[1] += ya.y * w; s[2] += ya.z * w; s[3] += ya.w * w;
                    s[4] += yb.x * w; s[5] += yb.y * w; s[6] += yb.z * w; s[7] += yb.w * w;
                    if (BACKWARD) {
                        const float4 da = *reinterpret_cast<const float4*>(dy1b + b * 8), db = *reinterpret_cast<const float4*>(dy1b + b * 8 + 4);
                        ds[0] += da.x * w; ds[1] += da.y * w; ds[2] += da.z * w; ds[3] += da.w * w;
                        ds[4] += db.x * w; ds[5] += db.y * w; ds[6] += db.z * w; ds[7] += db.w * w;
                    }
                }
#pragma unroll
                for (int p = 0; p < kPairTile; p++) {
                    const float fc = ps[1 * 8 + p];
                    const int j = __float_as_int(ps[3 * 8 + p]);
                    const float y2 = fc * s[p];                                               // ref :175 / :275
                    if (!BACKWARD) {
                        const float xj = live[c] ? x[(size_t)j * W + ch[c]] : 0.f;
                        acc[c] += y2 * xj;                                                    // ref :181
                    } else {
                        const float gj = live[c] ? gout[(size_t)j * W + ch[c]] : 0.f;
                        const float xj = live[c] ? x[(size_t)j * W + ch[c]] : 0.f;
                        acc[c] += y2 * gj;                                                    // ref :284
                        const float dy2 = ps[2 * 8 + p] * s[p] + fc * ds[p];                   // ref :276
                        scale_p[p] += live[c] ? dy2 * (xj * gi[c] + xi[c] * gj) : 0.f;         // ref :286
                    }
                }
            }
            if (BACKWARD) {
#pragma unroll
                for (int p = 0; p < kPairTile; p++) {
                    const float sc = wave_sum(scale_p[p]) * ps[4 * 8 + p];                    // * 1/r
                    // position_deriv[i] -= sc * delta  (owner side of ref :287-291; delta = pos_j - pos_i)
                    fx -= sc * ps[5 * 8 + p]; fy -= sc * ps[6 * 8 + p]; fz -= sc * ps[7 * 8 + p];
                    if (ROW_S && lane == p && p < np) row_s[(size_t)i * cap + t0 + p] = sc;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int c = 0; c < CPL; c++)
            if (live[c] && !ROW_S) out[(size_t)i * W + ch[c]] = acc[c];
        if (BACKWARD && !ROW_S && lane == 0) {
            pos_grad[3 * i] = fx; pos_grad[3 * i + 1] = fy; pos_grad[3 * i + 2] = fz;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The two dense layers of the filter network as 16x16x4 fp32 matrix-core tiles (cfconv_filters_mfma).
//
// `v_mfma_f32_16x16x4_f32` is exact fp32 (an fmaf chain) at the fp32 matrix rate.  A tile is 16 pair slots
// x all W = 16*NCB filters; lane l owns pair/row `l & 15` as the A operand and column `l & 15` of each
// 16-wide column block as the B operand and result, k = 4*step + (l >> 4):
//   layer 1  A = Gaussians (computed in registers, straight in operand layout: no redundancy),
//            B = W1^T from LDS, C initialised with b1;  activation on the accumulators -> Y1 tile in LDS
//   layer 2  A = Y1 tile read back transposed (row stride W+1: conflict-free), B = W2^T from LDS, C = b2
// Result layout of the instruction: D[row = 4*(l >> 4) + reg][col = l & 15].
// ---------------------------------------------------------------------------------------------
// One dense layer of a 16-row tile on the matrix core: acc[cb] += A(16 x 4*ksteps) * B(4*ksteps x 16) for the NCB
// column blocks.  a_lane / b_lane point at this lane's operands of K step 0; a K step advances A by 4 floats and B
// by 4 rows of W floats.  The operands of step s + 1 are requested BEFORE the MFMAs of step s are issued (explicit
// double buffer): left to itself the compiler reuses one register pair for B and waits for LDS every two MFMAs.
template <int NCB, int W>
__device__ __forceinline__ void mfma_layer(const float* a_lane, const float* b_lane, int ksteps, f32x4 (&acc)[NCB]) {
    float a_cur = a_lane[0], b_cur[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) b_cur[cb] = b_lane[cb * 16];
#pragma unroll 2
    for (int s = 0; s < ksteps; s++) {
        const int nx = min(s + 1, ksteps - 1);                 // (the last step re-reads itself: no branch in the loop)
        const float a_nxt = a_lane[4 * nx];
        float b_nxt[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) b_nxt[cb] = b_lane[(size_t)4 * nx * W + cb * 16];
        __builtin_amdgcn_sched_barrier(0);                     // the requests above stay above the MFMAs below
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur, b_cur[cb], acc[cb], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        a_cur = a_nxt;
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) b_cur[cb] = b_nxt[cb];
    }
}

__host__ __device__ inline size_t mfma_weight_floats(int W, int G) { return (size_t)W * W + (size_t)((G + 3) & ~3) * W; }
__host__ __device__ inline size_t mfma_wave_floats_bwd(int W) { return (size_t)16 * (W + 1) + 144; }

// ---------------------------------------------------------------------------------------------
// Half-list path (every matrix-core width): the filter network is evaluated once per PAIR.
//   cfconv_filters_mfma   tile = 16 consecutive pair slots (no owners, no raggedness); writes the filter row
//                         F[pid] = fc * (W2 y1 + b2) -- 512 B at W = 128 -- and, backward, the pair's radial
//                         force  s[pid] = sum_c (dfc S2 + fc dS2)_c (x_j g_i + x_i g_j)_c / r            ref :275-291
//   cfconv_gather         owner computes: out[i] = sum_e F[pid_e] * x[j_e]   (backward: the same sum over gout gives
//                         dE/dx[i], and dE/dpos[i] = -sum_e s[pid_e] delta_e) -- deterministic, no atomics.
// Compared with evaluating every pair from both ends this halves the matrix-core AND the activation work (which
// add up on a SIMD) for one round trip of F through HBM / the Infinity Cache.
// ---------------------------------------------------------------------------------------------
template <int ACT, int NCB, bool BWD>
__global__ __launch_bounds__(64 * kMaxWavesPerBlock) void cfconv_filters_mfma(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2t,
    const float* __restrict__ b2, const int* __restrict__ half_off, const float* __restrict__ half_r,
    const int2* __restrict__ half_ij, int pair_cap, const float* __restrict__ x, const float* __restrict__ gout,
    float* __restrict__ filt, float* __restrict__ pair_s) {
    constexpr int W = NCB * 16, YS = W + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int G = P.G, Gp = (G + 3) & ~3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves_per_block = blockDim.x >> 6;
    float* s_w2t = lds;
    float* s_w1t = s_w2t + (size_t)W * W;
    float* y1 = s_w1t + (size_t)Gp * W + (size_t)wave * mfma_wave_floats_bwd(W);   // [16][YS]
    float* ps = y1 + 16 * YS;                              // r | fc | dfc | 1/r | i | j, 16 each
    for (int q = tid; q < W * W; q += blockDim.x) s_w2t[q] = w2t[q];
    for (int q = tid; q < Gp * W; q += blockDim.x) s_w1t[q] = q < G * W ? w1t[q] : 0.f;
    __syncthreads();
    if (blockIdx.x == 0) {                                  // the all-zero row behind the last slot (entries without a mirror image)
        for (int q = tid; q < W; q += blockDim.x) filt[(size_t)pair_cap * W + q] = 0.f;
        if (BWD && tid == 0) pair_s[pair_cap] = 0.f;
    }

    const int col = lane & 15, grp = lane >> 4;
    float b1v[NCB], b2v[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) { b1v[cb] = b1[cb * 16 + col]; b2v[cb] = b2[cb * 16 + col]; }
    const float mu_step = P.cutoff / (float)(G - 1);
    const float sig2 = P.sigma_inv * P.sigma_inv;
    const float gscale = -0.5f * kLog2e * sig2;

    const int pairs = min(half_off[P.N], pair_cap);
    const int tiles = (pairs + 15) >> 4;
    const int total_waves = gridDim.x * waves_per_block;
    int t = blockIdx.x * waves_per_block + wave;
    auto request = [&](int tile, float& r, int2& ij) {      // lanes 0..15 (the others mirror them)
        const int p = 16 * tile + (lane & 15);
        r = -1.f;
        ij = make_int2(0, 0);
        if (tile < tiles && p < pairs) {
            r = half_r[p];
            if constexpr (BWD) ij = half_ij[p];
        }
    };
    float my_r;
    int2 my_ij;
    request(t, my_r, my_ij);
    for (; t < tiles; t += total_waves) {
        if (lane < 16) {
            float r = 1.0f, fc = 0.f, dfc = 0.f;
            if (my_r >= 0.f) {
                r = my_r;
                if constexpr (BWD) {
                    float sn, cs;
                    sincospif(r / P.cutoff, &sn, &cs);
                    fc = 0.5f * cs + 0.5f;                                              // ref :301-303
                    dfc = -(0.5f * kPi / P.cutoff) * sn;                                // ref :305-307
                } else {
                    fc = 0.5f * cospif(r / P.cutoff) + 0.5f;
                }
            }
            ps[lane] = r; ps[16 + lane] = fc;
            if constexpr (BWD) {
                ps[32 + lane] = dfc; ps[48 + lane] = 1.0f / r;
                ps[64 + lane] = __int_as_float(my_ij.x); ps[80 + lane] = __int_as_float(my_ij.y);
            }
        }
        float next_r;
        int2 next_ij;
        request(t + total_waves, next_r, next_ij);          // used after the GEMMs
        wave_fence();
        // ---- layer 1 (backward: value and d/dr together) ----
        f32x4 acc[NCB], dacc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
            acc[cb] = f32x4{b1v[cb], b1v[cb], b1v[cb], b1v[cb]};
            if constexpr (BWD) dacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float rp = ps[col];
        for (int s = 0; s < Gp / 4; s++) {
            const int g = 4 * s + grp;
            const float d = rp - (float)g * mu_step;
            const float a = g < G ? fast_exp2(gscale * d * d) : 0.f;                   // ref :151-154
            const float da = -d * sig2 * a;                                            // ref :242
            const float* wrow = s_w1t + g * W + col;
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                const float b = wrow[cb * 16];
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[cb], 0, 0, 0);
                if constexpr (BWD) dacc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, b, dacc[cb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int cb = 0; cb < NCB; cb++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if constexpr (BWD) {
                    float yv, dact;
                    activate_d_fast<ACT>(acc[cb][q], yv, dact);
                    y1[(grp * 4 + q) * YS + cb * 16 + col] = yv;
                    dacc[cb][q] *= dact;                                               // dY1, kept in registers
                } else {
                    y1[(grp * 4 + q) * YS + cb * 16 + col] = activate_fast<ACT>(acc[cb][q]);
                }
            }
        wave_fence();
        // ---- layer 2 on Y1 ----
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) acc[cb] = f32x4{b2v[cb], b2v[cb], b2v[cb], b2v[cb]};
        mfma_layer<NCB, W>(y1 + col * YS + grp, s_w2t + grp * W + col, W / 4, acc);
        if constexpr (BWD) {
            wave_fence();
            // ---- refill the tile with dY1, layer 2 again ----
#pragma unroll
            for (int cb = 0; cb < NCB; cb++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    y1[(grp * 4 + q) * YS + cb * 16 + col] = dacc[cb][q];
                    dacc[cb][q] = 0.f;
                }
            wave_fence();
            mfma_layer<NCB, W>(y1 + col * YS + grp, s_w2t + grp * W + col, W / 4, dacc);
        }
        // ---- my four pairs of the tile ----
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int rr = grp * 4 + q;
            const int p = 16 * t + rr;
            const float fc = ps[16 + rr];
            if (p < pairs) {                                // uniform over the 16 lanes of a row
                float* frow = filt + (size_t)p * W + col;
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) frow[cb * 16] = fc * acc[cb][q];      // ref :175
                if constexpr (BWD) {
                    const float dfc = ps[32 + rr];
                    const int i = __float_as_int(ps[64 + rr]), j = __float_as_int(ps[80 + rr]);
                    float sc = 0.f;
#pragma unroll
                    for (int cb = 0; cb < NCB; cb++) {
                        const size_t c = (size_t)cb * 16 + col;
                        const float xi = x[(size_t)i * W + c], gi = gout[(size_t)i * W + c];
                        const float xj = x[(size_t)j * W + c], gj = gout[(size_t)j * W + c];
                        const float dy2 = dfc * acc[cb][q] + fc * dacc[cb][q];         // ref :276
                        sc += dy2 * (xj * gi + xi * gj);                               // ref :286
                    }
                    sc += __shfl_xor(sc, 1, 64); sc += __shfl_xor(sc, 2, 64);
                    sc += __shfl_xor(sc, 4, 64); sc += __shfl_xor(sc, 8, 64);
                    if (col == 0) pair_s[p] = sc * ps[48 + rr];
                }
            }
            if constexpr (BWD) __builtin_amdgcn_sched_barrier(0);     // one pair's 4*NCB gathers in flight at a time
        }
        my_r = next_r; my_ij = next_ij;
        wave_fence();
    }
}

// ---------------------------------------------------------------------------------------------
// cfconv_filters_h2: the filters kernel with its dense layers on the half-precision matrix instruction, every fp32
// operand split into two fp16 planes so that the result keeps fp32 accuracy:
//     x = hi + 2^-11 lo'   (hi = fp16(x), lo' = fp16((x - hi) 2^11): 22 significant bits, every plane in normal range)
//     A B = Ahi Bhi + 2^-11 (Ahi Blo' + Alo' Bhi) + O(2^-22)          -- three v_mfma_f32_16x16x32_f16 per 16x16x32
//     block (fp32 accumulation, two accumulators) instead of eight v_mfma_f32_16x16x4_f32: 48 instead of 256 issue cycles.
// Measured on a 16 x 128 x 128 tile (tools/ubench/split_f16_gemm.hip): 2.6x faster than the fp32 form including the
// split, and a SMALLER error against a double-precision product (1.6e-6 against 3.8e-6 at |y| ~ 9: exact fp16
// products summed in fp32 versus a chain of 128 rounded fp32 FMAs).  The host only takes this kernel when the weights
// bound every operand below the fp16 range (nnpops_cfconv_create); $NNPOPS_CFCONV_SPLIT=0 keeps the all-fp32 one.
// This kernel splits layer 2 only; where layer 1 can be split too (G + 1 <= 64 and, at W = 128, G <= 55: plan_conv in cfconv.hip) the
// register-fed kernels take over (cfconv_filters_h2x2 / cfconv_filters_h2b), so it serves the Gaussians beyond and $NNPOPS_CFCONV_SPLIT=1.
//   layer 1   is computed TRANSPOSED (rows = filters, columns = pairs), so a lane ends up with four consecutive filters
//             of one pair -- after the activation exactly the 8-byte groups the A planes of layer 2 are written in.  b1
//             rides along as one more K index against a constant 1.  v_mfma_f32_16x16x4_f32 with the operands swapped.
//   LDS       W2 planes [f2][k] and the per-wave A planes [pair][k] with the 16-byte slot index XORed by the row
//             (h2_slot: conflict-free ds_read_b128); W1^T in fp32.  Same footprint as the fp32 kernel.
// ---------------------------------------------------------------------------------------------
// D = A B for one 16-row tile against all NCB column blocks: acc1 += Ahi Bhi, acc2 += Ahi Blo' + Alo' Bhi
// FRESH1 / FRESH2: the accumulator starts from zero -- passed as the (inline constant) C operand of its first MFMA instead
// of being cleared register by register beforehand.
template <int NCB, int W, bool TIGHT, bool FRESH1, bool FRESH2>   // TIGHT (backward): one K step's plane reads in flight, not two steps'
__device__ __forceinline__ void h2_layer(const char* a_h, const char* a_l, const char* b_h, const char* b_l, int row, int grp, int col,
                                         f32x4 (&acc1)[NCB], f32x4 (&acc2)[NCB]) {
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    auto step = [&](int s, auto first) {
        constexpr bool kFirst = decltype(first)::value;
        const int slot = 4 * s + grp;                       // this lane's 8 consecutive k of the step
        const f16x8 ah = *reinterpret_cast<const f16x8*>(a_h + h2_slot<W>(row, slot));
        const f16x8 al = *reinterpret_cast<const f16x8*>(a_l + h2_slot<W>(row, slot));
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
            const int f2 = cb * 16 + col;
            const f16x8 bh = *reinterpret_cast<const f16x8*>(b_h + h2_slot<W>(f2, slot));
            const f16x8 bl = *reinterpret_cast<const f16x8*>(b_l + h2_slot<W>(f2, slot));
            acc1[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, kFirst && FRESH1 ? zero : acc1[cb], 0, 0, 0);
            acc2[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, kFirst && FRESH2 ? zero : acc2[cb], 0, 0, 0);
            acc2[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc2[cb], 0, 0, 0);
        }
    };
    if constexpr (TIGHT) {                                  // (the caller has cleared / preset the accumulators)
        static_assert(!FRESH1 && !FRESH2, "the loop form does not peel its first step");
#pragma unroll 1
        for (int s = 0; s < W / 32; s++) step(s, std::false_type{});
    } else {
        step(0, std::true_type{});
#pragma unroll
        for (int s = 1; s < W / 32; s++) step(s, std::false_type{});
    }
}

template <int ACT, int NCB, bool BWD>
__global__ __launch_bounds__(64 * kMaxWavesPerBlock) void cfconv_filters_h2(
    ConvParams P, const float* __restrict__ w1b, const _Float16* __restrict__ w1h, const _Float16* __restrict__ w1l,   // (w1h, w1l: not read)
    const _Float16* __restrict__ w2h, const _Float16* __restrict__ w2l, const float* __restrict__ b2, const int* __restrict__ half_off, const float* __restrict__ half_r,
    const int2* __restrict__ half_ij, int pair_cap, const float* __restrict__ x, const float* __restrict__ gout,
    float* __restrict__ filt, float* __restrict__ pair_s) {
    constexpr int W = NCB * 16;
    static_assert(W % 32 == 0, "the K steps of layer 2 are 32 wide");
    extern __shared__ __attribute__((aligned(16))) char ldsb[];
    const int G = P.G, Gq = h2_l1_rows(G);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves_per_block = blockDim.x >> 6;
    char* s_w2h = ldsb;                                      // [W][W] halves, slots rotated
    char* s_w2l = s_w2h + (size_t)W * W * 2;
    float* s_w1t = reinterpret_cast<float*>(s_w2l + (size_t)W * W * 2);     // [Gq][W]: rows < G = W1^T, row G = b1, rest 0
    char* a_h = reinterpret_cast<char*>(s_w1t + (size_t)Gq * W) + (size_t)wave * h2_wave_bytes(W);
    char* a_l = a_h + 16 * W * 2;
    float* ps = reinterpret_cast<float*>(a_l + 16 * W * 2);  // r | fc | dfc | 1/r | i | j, 16 each
    for (int q = tid; q < W * (W / 8); q += blockDim.x) {    // 16-byte slots of the W2 planes
        const int f2 = q / (W / 8), slot = q % (W / 8);
        *reinterpret_cast<f16x8*>(s_w2h + h2_slot<W>(f2, slot)) = *reinterpret_cast<const f16x8*>(w2h + (size_t)f2 * W + slot * 8);
        *reinterpret_cast<f16x8*>(s_w2l + h2_slot<W>(f2, slot)) = *reinterpret_cast<const f16x8*>(w2l + (size_t)f2 * W + slot * 8);
    }
    for (int q = tid; q < Gq * W; q += blockDim.x) s_w1t[q] = w1b[q];
    __syncthreads();
    if (blockIdx.x == 0) {                                  // the all-zero row behind the last slot (entries without a mirror image)
        for (int q = tid; q < W; q += blockDim.x) filt[(size_t)pair_cap * W + q] = 0.f;
        if (BWD && tid == 0) pair_s[pair_cap] = 0.f;
    }

    const int col = lane & 15, grp = lane >> 4;
    float b2v[NCB];                                         // (backward: re-read per tile, the registers are needed)
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) b2v[cb] = b2[cb * 16 + col];
    const float mu_step = P.cutoff / (float)(G - 1);
    const float sig2 = P.sigma_inv * P.sigma_inv;
    const float gscale = -0.5f * kLog2e * sig2;

    const int pairs = min(half_off[P.N], pair_cap);
    const int tiles = (pairs + 15) >> 4;
    const int total_waves = gridDim.x * waves_per_block;
    int t = blockIdx.x * waves_per_block + wave;
    auto request = [&](int tile, float& r, int2& ij) {      // lanes 0..15 (the others mirror them)
        const int p = 16 * tile + (lane & 15);
        r = -1.f;
        ij = make_int2(0, 0);
        if (tile < tiles && p < pairs) {
            r = half_r[p];
            if constexpr (BWD) ij = half_ij[p];
        }
    };
    float my_r;
    int2 my_ij;
    request(t, my_r, my_ij);
    for (; t < tiles; t += total_waves) {
        if (lane < 16) {
            float r = 1.0f, fc = 0.f, dfc = 0.f;
            if (my_r >= 0.f) {
                r = my_r;
                if constexpr (BWD) {
                    float sn, cs;
                    sincospif(r / P.cutoff, &sn, &cs);
                    fc = 0.5f * cs + 0.5f;                                              // ref :301-303
                    dfc = -(0.5f * kPi / P.cutoff) * sn;                                // ref :305-307
                } else {
                    fc = 0.5f * cospif(r / P.cutoff) + 0.5f;
                }
            }
            ps[lane] = r; ps[16 + lane] = fc;
            if constexpr (BWD) {
                ps[32 + lane] = dfc; ps[48 + lane] = 1.0f / r;
                ps[64 + lane] = __int_as_float(my_ij.x); ps[80 + lane] = __int_as_float(my_ij.y);
            }
        }
        float next_r;
        int2 next_ij;
        request(t + total_waves, next_r, next_ij);          // used after the GEMMs
        wave_fence();
        // ---- layer 1, transposed: acc[cb][q] = S1 of filter 16 cb + 4 grp + q for the pair `col` ----
        const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 acc[NCB], dacc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
            acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (BWD) dacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float rp = ps[col];
        for (int s = 0; s < Gq / 4; s++) {
            const int g = 4 * s + grp;
            const float d = rp - (float)g * mu_step;
            float a = g < G ? fast_exp2(gscale * d * d) : 0.f;                     // ref :151-154
            float da = -d * sig2 * a;                                              // ref :242
            if (g == G) { a = 1.0f; da = 0.f; }                                    // the bias row
            const float* wrow = s_w1t + g * W + col;
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                const float w = wrow[cb * 16];
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, a, acc[cb], 0, 0, 0);
                if constexpr (BWD) dacc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, da, dacc[cb], 0, 0, 0);
            }
        }
        // ---- activation, split, A planes: pair `col`, filters 16 cb + 4 grp .. + 3 = half a 16-byte slot ----
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
            f16x4 h, l;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                float yv;
                if constexpr (BWD) {
                    float dact;
                    activate_d_fast<ACT>(acc[cb][q], yv, dact);
                    dacc[cb][q] *= dact;                                               // dY1, kept in registers
                } else {
                    yv = activate_fast<ACT>(acc[cb][q]);
                }
                h[q] = (_Float16)yv;
                l[q] = split_lo(yv, h[q]);
            }
            const int off = h2_slot<W>(col, 2 * cb + (grp >> 1)) + (grp & 1) * 8;
            *reinterpret_cast<f16x4*>(a_h + off) = h;
            *reinterpret_cast<f16x4*>(a_l + off) = l;
        }
        wave_fence();
        // ---- layer 2 on Y1: S2[pair 4 grp + q][filter 16 cb + col] ----
        f32x4 acc2[NCB];
        if constexpr (BWD) {
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                const float bias = b2[cb * 16 + col];
                acc[cb] = f32x4{bias, bias, bias, bias};
                acc2[cb] = zero4;
            }
            h2_layer<NCB, W, true, false, false>(a_h, a_l, s_w2h, s_w2l, col, grp, col, acc, acc2);
        } else {                                            // (zero C operands; the bias joins in the epilogue)
            h2_layer<NCB, W, false, true, true>(a_h, a_l, s_w2h, s_w2l, col, grp, col, acc, acc2);
        }
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) acc[cb] += kLoInv * acc2[cb];
        if constexpr (BWD) {
            wave_fence();
            // ---- refill the planes with dY1, layer 2 again ----
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                f16x4 h, l;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float dv = dacc[cb][q] * P.dy_scale;      // (ConvParams::dy_scale)
                    h[q] = (_Float16)dv;
                    l[q] = split_lo(dv, h[q]);
                }
                const int off = h2_slot<W>(col, 2 * cb + (grp >> 1)) + (grp & 1) * 8;
                *reinterpret_cast<f16x4*>(a_h + off) = h;
                *reinterpret_cast<f16x4*>(a_l + off) = l;
                dacc[cb] = zero4;
                acc2[cb] = zero4;
            }
            wave_fence();
            h2_layer<NCB, W, true, false, false>(a_h, a_l, s_w2h, s_w2l, col, grp, col, dacc, acc2);
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) dacc[cb] = (dacc[cb] + kLoInv * acc2[cb]) * P.dy_unscale;
        }
        // ---- my four pairs of the tile: the filter rows first (backward: and dy2 = dfc S2 + fc dS2 in place of dS2, after
        //      which S2 is dead and its registers serve the gathers), then the pair forces ----
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int rr = grp * 4 + q;
            const int p = 16 * t + rr;
            const float fc = ps[16 + rr];
            if (p < pairs && !(BWD && P.skip_filter_store)) {      // uniform over the 16 lanes of a row
                float* frow = filt + (size_t)p * W + col;
#pragma unroll
                for (int cb = 0; cb < NCB; cb++)
                    frow[cb * 16] = BWD ? fc * acc[cb][q] : fc * (acc[cb][q] + b2v[cb]);      // ref :175
            }
            if constexpr (BWD) {
                const float dfc = ps[32 + rr];
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) dacc[cb][q] = dfc * acc[cb][q] + fc * dacc[cb][q];     // ref :276
            }
        }
        if constexpr (BWD) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int rr = grp * 4 + q;
                const int p = 16 * t + rr;
                // (straight-line loads: a padding row of the last tile carries i = j = 0 and is simply not stored;
                //  with a branch around them the compiler would drain the load queue where the paths meet)
                const int i = __float_as_int(ps[64 + rr]), j = __float_as_int(ps[80 + rr]);
                float sc = 0.f;
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) {
                    const size_t c = (size_t)cb * 16 + col;
                    const float xi = x[(size_t)i * W + c], gi = gout[(size_t)i * W + c];
                    const float xj = x[(size_t)j * W + c], gj = gout[(size_t)j * W + c];
                    sc += dacc[cb][q] * (xj * gi + xi * gj);                           // ref :286
                }
                sc += __shfl_xor(sc, 1, 64); sc += __shfl_xor(sc, 2, 64);
                sc += __shfl_xor(sc, 4, 64); sc += __shfl_xor(sc, 8, 64);
                if (col == 0 && p < pairs) pair_s[p] = sc * ps[48 + rr];
                if (q & 1) __builtin_amdgcn_sched_barrier(0);       // two pairs' gathers in flight at a time
            }
        }
        my_r = next_r; my_ij = next_ij;
        wave_fence();
    }
}

}  // namespace
