// cfconv_weight_grad_second.h -- d/d(weights1, biases1, weights2, biases2) of the scalar the double backward differentiates: the weight
// gradients of a force loss (nnpops_cfconv_double_backward_weights).
//
// Notation of cfconv_second_order.h and cfconv_weight_grad.h.  For a half pair p = (i < j) at stored distance r, u = d / r, with output
// gradient g, input x and cotangents V [N][W] of input_deriv and Q [N][3] of position_deriv, the double backward differentiates
//     M = <V, gx> + <Q, gp> = sum_p F.A + a (F'.B),   A = V_j (.) g_i + V_i (.) g_j,   B = x_j (.) g_i + x_i (.) g_j,   a = u.(Q_j - Q_i)
//     gamma_g = exp(-(r - mu_g)^2 / 2 sigma^2)    gamma'_g = -((r - mu_g) / sigma^2) gamma_g
//     z = b1 + W1 gamma     z' = W1 gamma'     y = act(z)     y' = act'(z) z'
//     F = fc (W2 y + b2)    F' = fc' (W2 y + b2) + fc W2 y'
// With the per-pair coefficients p_c = fc A_c + a fc' B_c and q_c = a fc B_c:
//     db2[c] = sum_p p_c                              dw2[c][a] = sum_p p_c y_a + q_c y'_a
//     P_a = sum_c p_c w2[c][a]   R_a = sum_c q_c w2[c][a]
//     t_a = act'(z_a) P_a + act''(z_a) z'_a R_a       t'_a = act'(z_a) R_a
//     db1[a] = sum_p t_a                              dw1[a][g] = sum_p t_a gamma_g + t'_a gamma'_g
// These are cfconv_weight_grad.h's contractions over a tile twice as tall -- [p; q]^T [y; y'] and [t; t']^T [gamma; gamma'] -- so the
// partial-row layout [dw1 | db1 | dw2 | db2], wgrad_row_floats and cfconv_wgrad_finish are that header's, unchanged.  With Q absent,
// a = 0 and the sums are those of nnpops_cfconv_backprop_weights with V in the place of the input.
//
// The scalar a needs the displacement, which only the full rows {dx, dy, dz, j} hold: cfconv_pair_a walks the rows once (one wave per
// atom) and the entry with j > i writes its pair's value into the slot `pid` gives it.  Slots past the list's count are never read: they
// keep r = 1, fc = a = 0, hence exact zeros, and a list without pairs gives exact zeros.  A zero a is stored as +0, so a rigid
// translation in Q gives the bits of Q = NULL.
//   cfconv_wgrad2_mfma     W a multiple of 16 up to 128 with both weight matrices and the six tiles in LDS: everything on
//                          v_mfma_f32_16x16x4_f32.  One wave per 16-wide block of filters, as cfconv_wgrad_mfma; layer 1 feeds gamma and
//                          gamma' against one read of every W1 fragment, the middle product p and q against one read of every W2 fragment.
//   cfconv_wgrad2_vector   every other layer: weights streamed through the caches, tiles of kWgrad2VectorTile pair slots, the partial row
//                          accumulated in place by the thread that owns each entry.  Functional, not tuned.
// Included by cfconv.hip only.
#pragma once

#include "cfconv_second_order.h"
#include "cfconv_weight_grad.h"

namespace {
using namespace nnpops;

constexpr int kWgrad2VectorTile = 8;    // pair slots per tile of the vector kernel: six tiles of the widest layer (W = 512, G = 256) fit in LDS

// ---- a = u.(Q_j - Q_i) per pair slot ------------------------------------------------------------------------------------------------
// One wave per atom over its full row; bounds as the double backward: min(cnt, cap), ids masked with kIdMask, an id that is no atom skipped.
__global__ __launch_bounds__(256) void cfconv_pair_a(int N, const float4* __restrict__ rows, const int* __restrict__ cnt, int cap,
                                                      const int* __restrict__ pid, int pair_cap, const float* __restrict__ Q,
                                                      float* __restrict__ pair_a) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= N) return;
    const int n = min(cnt[i], cap);
    const float qx = Q[3 * i], qy = Q[3 * i + 1], qz = Q[3 * i + 2];
    for (int s = lane; s < n; s += 64) {
        const float4 rec = rows[(size_t)i * cap + s];
        const int j = __float_as_int(rec.w) & kIdMask;
        if (j <= i || j >= N) continue;
        const int p = pid[(size_t)i * cap + s];
        if (p < 0 || p >= pair_cap) continue;               // (only after a row overflow: check() grows and rebuilds)
        const float r = sqrtf(rec.x * rec.x + rec.y * rec.y + rec.z * rec.z);
        const float a = (rec.x * (Q[3 * j] - qx) + rec.y * (Q[3 * j + 1] - qy) + rec.z * (Q[3 * j + 2] - qz)) / r;
        pair_a[p] = a == 0.f ? 0.f : a;
    }
}

// r, fc, a fc', a fc, i, j of slot p (a padding slot: r = 1, everything else zero)
struct Wgrad2Slot { float r, fc, afd, af; int i, j; };
__device__ __forceinline__ Wgrad2Slot wgrad2_slot(int p, int pairs, float cutoff, const float* __restrict__ half_r,
                                                  const int2* __restrict__ half_ij, const float* __restrict__ pair_a) {
    Wgrad2Slot s{1.0f, 0.f, 0.f, 0.f, 0, 0};
    if (p < pairs) {
        s.r = half_r[p];
        const int2 ij = half_ij[p];
        s.i = ij.x; s.j = ij.y;
        float sn, cs;
        sincospif(s.r / cutoff, &sn, &cs);
        s.fc = 0.5f * cs + 0.5f;
        const float a = pair_a ? pair_a[p] : 0.f;
        s.afd = a * (-0.5f * (kPi / cutoff) * sn);
        s.af = a * s.fc;
    }
    return s;
}

// ---- matrix-core kernel ----------------------------------------------------------------------------------------------------------
// LDS: W2 [out][in] | W1^T [Gp][W] | Y, Y', P, Q, T, T' tiles [16][W + 16] | Gamma, Gamma' tiles [16][16 NGB] | r, fc, a fc', a fc, i, j of the tile
__host__ __device__ inline size_t wgrad2_mfma_floats(int W, int G) {
    const size_t Gp = (size_t)(G + 3) & ~(size_t)3;
    return (size_t)W * W + Gp * W + (size_t)6 * kWgradTile * (W + 16) + (size_t)2 * kWgradTile * 16 * wgrad_gamma_blocks(G) + 6 * kWgradTile;
}

template <int NCB, int NGB>
__global__ __launch_bounds__(64 * NCB) void cfconv_wgrad2_mfma(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2,
    const int* __restrict__ half_off, const float* __restrict__ half_r, const int2* __restrict__ half_ij, int pair_cap,
    const float* __restrict__ pair_a, const float* __restrict__ x, const float* __restrict__ gout, const float* __restrict__ V,
    float* __restrict__ partials) {
    constexpr int W = NCB * 16, TS = W + 16, GS = NGB * 16, TP = kWgradTile;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int G = P.G, Gp = (G + 3) & ~3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* s_w2 = lds;                                      // [c][a]: the core layout
    float* s_w1t = s_w2 + W * W;                            // [g][a]
    float* tY = s_w1t + Gp * W;
    float* tYd = tY + TP * TS;                              // y'
    float* tP = tYd + TP * TS;
    float* tQ = tP + TP * TS;
    float* tT = tQ + TP * TS;
    float* tTd = tT + TP * TS;                              // t'
    float* tG = tTd + TP * TS;                              // [pair][GS]; columns G .. GS-1 stay zero
    float* tGd = tG + TP * GS;                              // gamma'
    float* ps = tGd + TP * GS;                              // r | fc | a fc' | a fc | i | j, 16 each
    for (int q = tid; q < W * W; q += blockDim.x) s_w2[q] = w2[q];
    for (int q = tid; q < Gp * W; q += blockDim.x) s_w1t[q] = q < G * W ? w1t[q] : 0.f;
    for (int q = tid; q < 2 * TP * GS; q += blockDim.x) tG[q] = 0.f;

    const int col = lane & 15, grp = lane >> 4;
    const int mycol = wave * 16 + col;                      // my column of every tile; my row offset of the accumulators is 16 * wave
    const float b1v = b1[mycol];
    const float mu_step = P.cutoff / (float)(G - 1);
    const float sig2 = P.sigma_inv * P.sigma_inv;
    const float gscale = -0.5f * kLog2e * sig2;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc2[NCB], acc1[NGB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) acc2[cb] = zero;
#pragma unroll
    for (int gb = 0; gb < NGB; gb++) acc1[gb] = zero;
    float sum_p = 0.f, sum_t = 0.f;                         // my share of db2[mycol], db1[mycol]: pairs 4 grp .. 4 grp + 3 of every tile

    const int pairs = min(half_off[P.N], pair_cap);
    const int tiles = (pairs + TP - 1) / TP;
    const int per_block = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int t_end = min(tiles, ((int)blockIdx.x + 1) * per_block);
    __syncthreads();                                        // the weights are in
    for (int t = blockIdx.x * per_block; t < t_end; t++) {
        // (no barrier here: the last tile's products do not read `ps`, and nothing else is written before the next barrier)
        if (tid < TP) {
            const Wgrad2Slot s = wgrad2_slot(TP * t + tid, pairs, P.cutoff, half_r, half_ij, pair_a);
            ps[tid] = s.r; ps[16 + tid] = s.fc; ps[32 + tid] = s.afd; ps[48 + tid] = s.af;
            ps[64 + tid] = __int_as_float(s.i); ps[80 + tid] = __int_as_float(s.j);
        }
        __syncthreads();
        // ---- Z = b1 + Gamma W1^T and Z' = Gamma' W1^T, my 16 columns; the Gaussians straight in operand layout (pair = col, g = 4 s + grp) ----
        f32x4 z = f32x4{b1v, b1v, b1v, b1v}, zd = zero;
        const float rp = ps[col];
        for (int s = 0; s < Gp / 4; s++) {
            const int g = 4 * s + grp;
            const float d = rp - (float)g * mu_step;
            const float a = g < G ? fast_exp2(gscale * d * d) : 0.f;
            const float ad = -d * sig2 * a;
            if (s % NCB == wave && g < G) { tG[col * GS + g] = a; tGd[col * GS + g] = ad; }
            const float w = s_w1t[g * W + mycol];
            z = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, z, 0, 0, 0);
            zd = __builtin_amdgcn_mfma_f32_16x16x4f32(ad, w, zd, 0, 0, 0);
        }
        // ---- Y, Y', act', act'' z', P, Q in result layout: pair = 4 grp + q, column = mycol ----
        f32x4 d1v, d2zv;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int pr = 4 * grp + q;
            float yv, d1, d2;
            if (P.activation == 0) activate_d2<0>(z[q], yv, d1, d2); else activate_d2<1>(z[q], yv, d1, d2);
            d1v[q] = d1;
            d2zv[q] = d2 * zd[q];
            tY[pr * TS + mycol] = yv;
            tYd[pr * TS + mycol] = d1 * zd[q];
            const float fc = ps[16 + pr];
            float pv = 0.f, qv = 0.f;
            if (fc != 0.f) {                                // (uniform over the 16 lanes of a pair; empty slots gather nothing)
                const size_t i = (size_t)__float_as_int(ps[64 + pr]), j = (size_t)__float_as_int(ps[80 + pr]);
                const float gi = gout[i * W + mycol], gj = gout[j * W + mycol];
                const float A = V ? V[j * W + mycol] * gi + V[i * W + mycol] * gj : 0.f;
                const float B = x[j * W + mycol] * gi + x[i * W + mycol] * gj;
                pv = fc * A + ps[32 + pr] * B;
                qv = ps[48 + pr] * B;
            }
            tP[pr * TS + mycol] = pv;
            tQ[pr * TS + mycol] = qv;
            sum_p += pv;
        }
        __syncthreads();
        // ---- U = P W2 and R = Q W2, my 16 columns; T = act' U + act'' z' R, T' = act' R ----
        f32x4 u = zero, rr = zero;
        {
            const float* a_lane = tP + col * TS + grp;
            const float* c_lane = tQ + col * TS + grp;
            const float* b_lane = s_w2 + grp * W + mycol;
#pragma unroll 4
            for (int s = 0; s < W / 4; s++) {
                const float w = b_lane[4 * s * W];
                u = __builtin_amdgcn_mfma_f32_16x16x4f32(a_lane[4 * s], w, u, 0, 0, 0);
                rr = __builtin_amdgcn_mfma_f32_16x16x4f32(c_lane[4 * s], w, rr, 0, 0, 0);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float tv = d1v[q] * u[q] + d2zv[q] * rr[q];
            tT[(4 * grp + q) * TS + mycol] = tv;
            tTd[(4 * grp + q) * TS + mycol] = d1v[q] * rr[q];
            sum_t += tv;
        }
        __syncthreads();
        // ---- dw2[16 wave + row][:] += P^T Y + Q^T Y' and dw1[16 wave + row][:] += T^T Gamma + T'^T Gamma': K = twice the tile's pairs ----
#pragma unroll
        for (int s = 0; s < TP / 4; s++) {
            const int pr = 4 * s + grp;
            const float pa = tP[pr * TS + mycol], qa = tQ[pr * TS + mycol], ta = tT[pr * TS + mycol], tda = tTd[pr * TS + mycol];
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                acc2[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, tY[pr * TS + cb * 16 + col], acc2[cb], 0, 0, 0);
                acc2[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa, tYd[pr * TS + cb * 16 + col], acc2[cb], 0, 0, 0);
            }
#pragma unroll
            for (int gb = 0; gb < NGB; gb++) {
                acc1[gb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ta, tG[pr * GS + gb * 16 + col], acc1[gb], 0, 0, 0);
                acc1[gb] = __builtin_amdgcn_mfma_f32_16x16x4f32(tda, tGd[pr * GS + gb * 16 + col], acc1[gb], 0, 0, 0);
            }
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
    sum_p += __shfl_xor(sum_p, 16, 64); sum_p += __shfl_xor(sum_p, 32, 64);
    sum_t += __shfl_xor(sum_t, 16, 64); sum_t += __shfl_xor(sum_t, 32, 64);
    if (grp == 0) { p_b2[mycol] = sum_p; p_b1[mycol] = sum_t; }
}

// ---- vector kernel ---------------------------------------------------------------------------------------------------------------
// LDS: Y, Y', P, Q, T, T' tiles [8][W] | Gamma, Gamma' tiles [8][G] | r, fc, a fc', a fc, i, j of the tile
__host__ __device__ inline size_t wgrad2_vector_floats(int W, int G) {
    return (size_t)kWgrad2VectorTile * (6 * (size_t)W + 2 * (size_t)G) + 6 * kWgrad2VectorTile;
}

__global__ __launch_bounds__(kWgradVectorThreads) void cfconv_wgrad2_vector(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2,
    const int* __restrict__ half_off, const float* __restrict__ half_r, const int2* __restrict__ half_ij, int pair_cap,
    const float* __restrict__ pair_a, const float* __restrict__ x, const float* __restrict__ gout, const float* __restrict__ V,
    float* __restrict__ partials) {
    constexpr int TP = kWgrad2VectorTile;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int W = P.W, G = P.G, tid = threadIdx.x, nthreads = blockDim.x;
    float* tY = lds;
    float* tYd = tY + TP * W;
    float* tP = tYd + TP * W;
    float* tQ = tP + TP * W;
    float* tT = tQ + TP * W;                                // act' first, then T
    float* tTd = tT + TP * W;                               // act'' z' first, then T'
    float* tG = tTd + TP * W;
    float* tGd = tG + TP * G;
    float* ps = tGd + TP * G;                               // r | fc | a fc' | a fc | i | j, TP each
    const float mu_step = P.cutoff / (float)(G - 1);
    const float sig2 = P.sigma_inv * P.sigma_inv;
    const float gscale = -0.5f * kLog2e * sig2;
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
            const Wgrad2Slot s = wgrad2_slot(TP * t + tid, pairs, P.cutoff, half_r, half_ij, pair_a);
            ps[tid] = s.r; ps[TP + tid] = s.fc; ps[2 * TP + tid] = s.afd; ps[3 * TP + tid] = s.af;
            ps[4 * TP + tid] = __int_as_float(s.i); ps[5 * TP + tid] = __int_as_float(s.j);
        }
        __syncthreads();
        for (int e = tid; e < TP * G; e += nthreads) {
            const int pr = e / G, g = e - pr * G;
            const float d = ps[pr] - (float)g * mu_step;
            const float a = fast_exp2(gscale * d * d);
            tG[e] = a;
            tGd[e] = -d * sig2 * a;
        }
        __syncthreads();
        for (int e = tid; e < TP * W; e += nthreads) {      // Y, Y', act', act'' z', P, Q
            const int pr = e / W, a = e - pr * W;
            float z = b1[a], zd = 0.f;
            for (int g = 0; g < G; g++) {
                const float w = w1t[(size_t)g * W + a];
                z = fmaf(w, tG[pr * G + g], z);
                zd = fmaf(w, tGd[pr * G + g], zd);
            }
            float yv, d1, d2;
            if (P.activation == 0) activate_d2<0>(z, yv, d1, d2); else activate_d2<1>(z, yv, d1, d2);
            tY[e] = yv;
            tYd[e] = d1 * zd;
            tT[e] = d1;
            tTd[e] = d2 * zd;
            const float fc = ps[TP + pr];
            float pv = 0.f, qv = 0.f;
            if (fc != 0.f) {
                const size_t i = (size_t)__float_as_int(ps[4 * TP + pr]), j = (size_t)__float_as_int(ps[5 * TP + pr]);
                const float gi = gout[i * W + a], gj = gout[j * W + a];
                const float A = V ? V[j * W + a] * gi + V[i * W + a] * gj : 0.f;
                const float B = x[j * W + a] * gi + x[i * W + a] * gj;
                pv = fc * A + ps[2 * TP + pr] * B;
                qv = ps[3 * TP + pr] * B;
            }
            tP[e] = pv;
            tQ[e] = qv;
        }
        __syncthreads();
        for (int e = tid; e < TP * W; e += nthreads) {      // T = act' (P W2) + act'' z' (Q W2), T' = act' (Q W2)
            const int pr = e / W, a = e - pr * W;
            float u = 0.f, rr = 0.f;
            for (int c = 0; c < W; c++) {
                const float w = w2[(size_t)c * W + a];
                u = fmaf(tP[pr * W + c], w, u);
                rr = fmaf(tQ[pr * W + c], w, rr);
            }
            const float d1 = tT[e];
            tT[e] = d1 * u + tTd[e] * rr;
            tTd[e] = d1 * rr;
        }
        __syncthreads();
        for (int e = tid; e < row_len; e += nthreads) {     // the tile's share of every entry, added in place by its owner
            float sum = 0.f;
            if (e < n_w1) {
                const int a = e / G, g = e - a * G;
                for (int pr = 0; pr < TP; pr++) sum = fmaf(tT[pr * W + a], tG[pr * G + g], fmaf(tTd[pr * W + a], tGd[pr * G + g], sum));
            } else if (e < n_w1 + W) {
                const int a = e - n_w1;
                for (int pr = 0; pr < TP; pr++) sum += tT[pr * W + a];
            } else if (e < n_w1 + W + n_w2) {
                const int q = e - n_w1 - W, c = q / W, a = q - c * W;
                for (int pr = 0; pr < TP; pr++) sum = fmaf(tP[pr * W + c], tY[pr * W + a], fmaf(tQ[pr * W + c], tYd[pr * W + a], sum));
            } else {
                const int c = e - n_w1 - W - n_w2;
                for (int pr = 0; pr < TP; pr++) sum += tP[pr * W + c];
            }
            row[e] += sum;
        }
    }
}

}  // namespace
