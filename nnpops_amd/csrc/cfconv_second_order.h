// cfconv_second_order.h -- second derivatives of the CFConv with respect to positions and input: the backward of the backward pass
// (nnpops_cfconv_double_backward).
//
// For a row entry {i -> j}: d = x_j - x_i (+ n B, as the build stored it), r = |d|, u = d / r, and the filter row
//     F(r) = fc(r) (W2 act(W1 gamma(r) + b1) + b2),   F', F'' its derivatives in r.
// The backward pass returns gx_i = sum_j F (.) g_j and gp_i = -sum_j (F'.B) u with B = x_j (.) g_i + x_i (.) g_j.  With cotangents
// V [N][W] of gx and Q [N][3] of gp, M = <V, gx> + <Q, gp> = sum over pairs of F.A + a (F'.B), A = V_j (.) g_i + V_i (.) g_j,
// a = u.(Q_j - Q_i), and
//     dM/dg_i   = sum_j  F (.) V_j + a F' (.) x_j
//     dM/dx_i   = sum_j  a F' (.) g_j
//     dM/dpos_i = -sum_j [F'.A + a (F''.B) - (a / r)(F'.B)] u + ((F'.B) / r)(Q_j - Q_i)
// with   gamma'' = ((r - mu)^2 / sigma^2 - 1) gamma / sigma^2,   y1'' = act'' (s1')^2 + act' s1'',   fc'' = -(pi / c)^2 cos(pi r / c) / 2,
//        F'' = fc'' S2 + 2 fc' S2' + fc S2''.
// One owner-computes pass over the FULL rows {dx, dy, dz, j} that every build leaves: the wave of atom i evaluates the filter network
// and its two derivatives for every entry of its row, keeps its three outputs in registers and writes each once.  No atomics, no half
// list, no filter rows: the kernels read the rows, the fp32 weights and the per-atom arrays x, g, V, Q and nothing a forward or backward
// call keeps, so they serve every ConvPath and two calls agree bit for bit.  Bounds as the box pass: min(cnt, cap), ids masked with
// kIdMask, an entry with j >= N turned into a padding slot (every term an exact zero), a cell-ordered build walked through sorted_pos.
//   cfconv_second_mfma     W = 16 NCB <= 128, weights resident in LDS: tiles of 16 row entries x W on v_mfma_f32_16x16x4_f32.  Layer 1
//                          takes gamma, gamma', gamma'' as three A operands against one read of every W1 fragment; layer 2 runs over
//                          Y1, Y1', Y1'' (one LDS tile, refilled from registers, mfma_layer of cfconv_fallback_kernels.h)
//   cfconv_second_vector   every other shape: cfconv_kernel's tiling (8 entries at a time, lane = filter channel(s)), weights in LDS
//                          or streamed through the caches
// V or Q may be NULL (= zero).  Included by cfconv.hip only.
#pragma once

#include "cfconv_fallback_kernels.h"

namespace {
using namespace nnpops;

// activation with its first and second derivative (plain domain: the weights are those of the vector kernel)
template <int ACT>
__device__ __forceinline__ void activate_d2(float s, float& y, float& d1, float& d2) {
    if (ACT == 0) {
        const float e = expf(s);
        y = logf(0.5f * e + 0.5f);
        d1 = e / (e + 1.0f);
        d2 = d1 * (1.0f - d1);
    } else {
        const float th = tanhf(s);
        y = th;
        d1 = 1.0f - th * th;
        d2 = -2.0f * th * d1;
    }
}

// What lane p of a tile knows about its row entry.  A padding slot (past the row's end, or an id that is no atom) has j = i, r = 1
// and fc = fc' = fc'' = a = 0: every term it enters is an exact zero.
struct SecondEntry {
    float r, rinv, fc, dfc, ddfc, a, dx, dy, dz, qx, qy, qz;
    int j;
};
__device__ __forceinline__ SecondEntry second_entry(const float4* __restrict__ row, int e, int n, int i, int N, float cutoff,
                                                    const float* __restrict__ Q) {
    SecondEntry s;
    float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
    bool valid = e < n;
    s.j = i;
    if (valid) {
        rec = row[e];
        s.j = __float_as_int(rec.w) & kIdMask;
        if (s.j >= N) { valid = false; s.j = i; rec = make_float4(0.f, 0.f, 0.f, 0.f); }
    }
    s.dx = rec.x; s.dy = rec.y; s.dz = rec.z;
    s.r = valid ? sqrtf(rec.x * rec.x + rec.y * rec.y + rec.z * rec.z) : 1.0f;
    s.rinv = 1.0f / s.r;
    float sn, cs;
    sincospif(s.r / cutoff, &sn, &cs);
    const float k = kPi / cutoff;
    s.fc = valid ? 0.5f * cs + 0.5f : 0.f;
    s.dfc = valid ? -0.5f * k * sn : 0.f;
    s.ddfc = valid ? -0.5f * k * k * cs : 0.f;
    s.qx = s.qy = s.qz = 0.f;
    if (Q && valid) {
        s.qx = Q[3 * s.j] - Q[3 * i]; s.qy = Q[3 * s.j + 1] - Q[3 * i + 1]; s.qz = Q[3 * s.j + 2] - Q[3 * i + 2];
    }
    s.a = (rec.x * s.qx + rec.y * s.qy + rec.z * s.qz) * s.rinv;
    return s;
}

// ---------------------------------------------------------------------------------------------
// vector family
// ---------------------------------------------------------------------------------------------
// LDS: the weights as cfconv_kernel keeps them | per wave: entry scalars [16][8], gamma / gamma' / gamma'' [3][G][8], y1 / y1' / y1'' [3][W][8]
__host__ __device__ inline size_t second_wave_floats(int W, int G) { return (size_t)3 * ((size_t)G + W) * kPairTile + 16 * kPairTile; }

template <int ACT, int CPL, bool WLDS>
__global__ __launch_bounds__(64 * kMaxWavesPerBlock) void cfconv_second_vector(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2t,
    const float* __restrict__ b2, const float4* __restrict__ rows, const int* __restrict__ cnt, int cap,
    const float4* __restrict__ sorted_pos,     // atoms in cell order (id in .w), or NULL
    const float* __restrict__ x, const float* __restrict__ gout, const float* __restrict__ V, const float* __restrict__ Q,
    float* __restrict__ out_g, float* __restrict__ out_x, float* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int W = P.W, G = P.G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* s_w2t = WLDS ? lds : w2t;                    // [W][W]   s_w2t[b*W + a] = w2[a][b]
    const float* s_w1t = WLDS ? lds + (size_t)W * W : w1t;    // [G][W]   s_w1t[g*W + a] = w1[a][g]
    const int waves_per_block = blockDim.x >> 6;
    float* ps = lds + (WLDS ? conv_weight_floats(W, G) : 0) + (size_t)wave * second_wave_floats(W, G);
    float* gam = ps + 16 * kPairTile;                         // [3][G][8]
    float* y1b = gam + (size_t)3 * G * kPairTile;             // [3][W][8]
    const size_t gs = (size_t)G * kPairTile, ys = (size_t)W * kPairTile;

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
    const float mu_step = P.cutoff / (float)(G - 1);
    const float sig2 = P.sigma_inv * P.sigma_inv;

    for (int w = blockIdx.x * waves_per_block + wave; w < P.N; w += gridDim.x * waves_per_block) {
        const int i = sorted_pos ? __float_as_int(sorted_pos[w].w) & kIdMask : w;
        if (i >= P.N) continue;                               // (a grid that could not be built: check() reports it)
        const int n = min(cnt[i], cap);                       // (an overflowed build stays in bounds and is incomplete, as its forces are)
        const float4* row = rows + (size_t)i * cap;
        float acc_g[CPL], acc_x[CPL], xi[CPL], gi[CPL], vi[CPL];
#pragma unroll
        for (int c = 0; c < CPL; c++) {
            acc_g[c] = 0.f; acc_x[c] = 0.f;
            xi[c] = x[(size_t)i * W + ch[c]];
            gi[c] = gout[(size_t)i * W + ch[c]];
            vi[c] = V ? V[(size_t)i * W + ch[c]] : 0.f;
        }
        float fx = 0.f, fy = 0.f, fz = 0.f;
        for (int t0 = 0; t0 < n; t0 += kPairTile) {
            if (lane < kPairTile) {
                const SecondEntry s = second_entry(row, t0 + lane, n, i, P.N, P.cutoff, Q);
                ps[0 * 8 + lane] = s.r; ps[1 * 8 + lane] = s.fc; ps[2 * 8 + lane] = s.dfc; ps[3 * 8 + lane] = s.ddfc;
                ps[4 * 8 + lane] = s.rinv; ps[5 * 8 + lane] = __int_as_float(s.j); ps[6 * 8 + lane] = s.a;
                ps[7 * 8 + lane] = s.dx; ps[8 * 8 + lane] = s.dy; ps[9 * 8 + lane] = s.dz;
                ps[10 * 8 + lane] = s.qx; ps[11 * 8 + lane] = s.qy; ps[12 * 8 + lane] = s.qz;
            }
            wave_fence();
            // ---- Gaussians and their two derivatives for the 8 entries ----
            for (int q = lane; q < G * kPairTile; q += 64) {
                const int g = q >> 3, p = q & 7;
                const float d = ps[p] - (float)g * mu_step;
                const float xg = d * P.sigma_inv;
                const float gm = expf(-0.5f * xg * xg);
                gam[q] = gm;
                gam[gs + q] = -d * sig2 * gm;
                gam[2 * gs + q] = (xg * xg - 1.0f) * sig2 * gm;
            }
            wave_fence();
            // ---- dense 1 + activation ----
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                float s[kPairTile], ds[kPairTile], dds[kPairTile];
#pragma unroll
                for (int p = 0; p < kPairTile; p++) { s[p] = bias1[c]; ds[p] = 0.f; dds[p] = 0.f; }
                for (int g = 0; g < G; g++) {
                    const float wt = s_w1t[g * W + ch[c]];
                    const float* ga = gam + g * 8;
#pragma unroll
                    for (int p = 0; p < kPairTile; p++) {
                        s[p] += ga[p] * wt; ds[p] += ga[gs + p] * wt; dds[p] += ga[2 * gs + p] * wt;
                    }
                }
                if (live[c]) {
#pragma unroll
                    for (int p = 0; p < kPairTile; p++) {
                        float y, d1, d2;
                        activate_d2<ACT>(s[p], y, d1, d2);
                        y1b[ch[c] * 8 + p] = y;
                        y1b[ys + ch[c] * 8 + p] = d1 * ds[p];
                        y1b[2 * ys + ch[c] * 8 + p] = d2 * ds[p] * ds[p] + d1 * dds[p];
                    }
                }
            }
            wave_fence();
            // ---- dense 2, cutoff, the sums of every entry ----
            float sA[kPairTile], sB1[kPairTile], sB2[kPairTile];
#pragma unroll
            for (int p = 0; p < kPairTile; p++) { sA[p] = 0.f; sB1[p] = 0.f; sB2[p] = 0.f; }
#pragma unroll
            for (int c = 0; c < CPL; c++) {
                float s[kPairTile], ds[kPairTile], dds[kPairTile];
#pragma unroll
                for (int p = 0; p < kPairTile; p++) { s[p] = bias2[c]; ds[p] = 0.f; dds[p] = 0.f; }
                for (int b = 0; b < W; b++) {
                    const float wt = s_w2t[b * W + ch[c]];
                    const float* ya = y1b + b * 8;
#pragma unroll
                    for (int p = 0; p < kPairTile; p++) {
                        s[p] += ya[p] * wt; ds[p] += ya[ys + p] * wt; dds[p] += ya[2 * ys + p] * wt;
                    }
                }
                if (live[c]) {
#pragma unroll
                    for (int p = 0; p < kPairTile; p++) {
                        const float fc = ps[1 * 8 + p], dfc = ps[2 * 8 + p], ddfc = ps[3 * 8 + p], a = ps[6 * 8 + p];
                        const int j = __float_as_int(ps[5 * 8 + p]);
                        const float F = fc * s[p];
                        const float F1 = dfc * s[p] + fc * ds[p];
                        const float F2 = ddfc * s[p] + 2.0f * dfc * ds[p] + fc * dds[p];
                        const float xj = x[(size_t)j * W + ch[c]], gj = gout[(size_t)j * W + ch[c]];
                        const float vj = V ? V[(size_t)j * W + ch[c]] : 0.f;
                        acc_g[c] += F * vj + a * F1 * xj;
                        acc_x[c] += a * F1 * gj;
                        const float B = xj * gi[c] + xi[c] * gj;
                        sA[p] += F1 * (vj * gi[c] + vi[c] * gj);
                        sB1[p] += F1 * B;
                        sB2[p] += F2 * B;
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < kPairTile; p++) {
                const float tA = wave_sum(sA[p]), tB1 = wave_sum(sB1[p]), tB2 = wave_sum(sB2[p]);
                const float rinv = ps[4 * 8 + p], a = ps[6 * 8 + p];
                const float cu = (tA + a * tB2 - a * rinv * tB1) * rinv, cq = tB1 * rinv;
                fx -= cu * ps[7 * 8 + p] + cq * ps[10 * 8 + p];
                fy -= cu * ps[8 * 8 + p] + cq * ps[11 * 8 + p];
                fz -= cu * ps[9 * 8 + p] + cq * ps[12 * 8 + p];
            }
            wave_fence();
        }
#pragma unroll
        for (int c = 0; c < CPL; c++)
            if (live[c]) {
                out_g[(size_t)i * W + ch[c]] = acc_g[c];
                out_x[(size_t)i * W + ch[c]] = acc_x[c];
            }
        if (lane == 0) { out_pos[3 * i] = fx; out_pos[3 * i + 1] = fy; out_pos[3 * i + 2] = fz; }
    }
}

// ---------------------------------------------------------------------------------------------
// fp32 matrix instruction family
// ---------------------------------------------------------------------------------------------
// LDS: W2^T [W][W] | W1^T [Gp][W] (rows past G zero) | per wave: the Y1 tile [16][W + 1], the entry scalars [13][16]
__host__ __device__ inline size_t second_mfma_wave_floats(int W) { return (size_t)16 * (W + 1) + 16 * 14; }

// WAVES = the largest workgroup, in waves: 8 up to W = 64; 4 above, one wave per SIMD with all 512 registers of its lanes -- the three
// accumulator sets, the rows of atom i and the two output rows are ~400 registers at W = 128 (256 vector + 146 accumulation), and with
// two waves per SIMD (256 each) the kernel spills up to 492 bytes per lane.
template <int ACT, int NCB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void cfconv_second_mfma(
    ConvParams P, const float* __restrict__ w1t, const float* __restrict__ b1, const float* __restrict__ w2t,
    const float* __restrict__ b2, const float4* __restrict__ rows, const int* __restrict__ cnt, int cap,
    const float4* __restrict__ sorted_pos, const float* __restrict__ x, const float* __restrict__ gout, const float* __restrict__ V,
    const float* __restrict__ Q, float* __restrict__ out_g, float* __restrict__ out_x, float* __restrict__ out_pos) {
    constexpr int W = NCB * 16, YS = W + 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int G = P.G, Gp = (G + 3) & ~3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves_per_block = blockDim.x >> 6;
    float* s_w2t = lds;
    float* s_w1t = s_w2t + (size_t)W * W;
    float* y1 = s_w1t + (size_t)Gp * W + (size_t)wave * second_mfma_wave_floats(W);   // [16][YS]
    float* ps = y1 + 16 * YS;                              // r | fc | fc' | fc'' | 1/r | j | a | d | Q_j - Q_i, 16 each
    for (int q = tid; q < W * W; q += blockDim.x) s_w2t[q] = w2t[q];
    for (int q = tid; q < Gp * W; q += blockDim.x) s_w1t[q] = q < G * W ? w1t[q] : 0.f;
    __syncthreads();

    const int col = lane & 15, grp = lane >> 4;
    float b1v[NCB], b2v[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) { b1v[cb] = b1[cb * 16 + col]; b2v[cb] = b2[cb * 16 + col]; }
    const float mu_step = P.cutoff / (float)(G - 1);
    const float sig2 = P.sigma_inv * P.sigma_inv;

    for (int w = blockIdx.x * waves_per_block + wave; w < P.N; w += gridDim.x * waves_per_block) {
        const int i = sorted_pos ? __float_as_int(sorted_pos[w].w) & kIdMask : w;
        if (i >= P.N) continue;                             // (a grid that could not be built: check() reports it)
        const int n = min(cnt[i], cap);                     // (an overflowed build stays in bounds and is incomplete, as its forces are)
        const float4* row = rows + (size_t)i * cap;
        float acc_g[NCB], acc_x[NCB], xi[NCB], gi[NCB], vi[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
            const size_t c = (size_t)i * W + cb * 16 + col;
            acc_g[cb] = 0.f; acc_x[cb] = 0.f;
            xi[cb] = x[c]; gi[cb] = gout[c];
            vi[cb] = V ? V[c] : 0.f;
        }
        float fx = 0.f, fy = 0.f, fz = 0.f;
        for (int t0 = 0; t0 < n; t0 += 16) {
            if (lane < 16) {
                const SecondEntry s = second_entry(row, t0 + lane, n, i, P.N, P.cutoff, Q);
                ps[lane] = s.r; ps[16 + lane] = s.fc; ps[32 + lane] = s.dfc; ps[48 + lane] = s.ddfc;
                ps[64 + lane] = s.rinv; ps[80 + lane] = __int_as_float(s.j); ps[96 + lane] = s.a;
                ps[112 + lane] = s.dx; ps[128 + lane] = s.dy; ps[144 + lane] = s.dz;
                ps[160 + lane] = s.qx; ps[176 + lane] = s.qy; ps[192 + lane] = s.qz;
            }
            wave_fence();
            // ---- layer 1: value, d/dr and d2/dr2 against one read of every W1 fragment ----
            f32x4 acc[NCB], dacc[NCB], ddacc[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) {
                acc[cb] = f32x4{b1v[cb], b1v[cb], b1v[cb], b1v[cb]};
                dacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
                ddacc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float rp = ps[col];
            for (int s = 0; s < Gp / 4; s++) {
                const int g = 4 * s + grp;
                const float d = rp - (float)g * mu_step;
                const float a = g < G ? expf(-0.5f * d * d * sig2) : 0.f;
                const float da = -d * sig2 * a;
                const float dda = (d * d * sig2 - 1.0f) * sig2 * a;
                const float* wrow = s_w1t + g * W + col;
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) {
                    const float b = wrow[cb * 16];
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[cb], 0, 0, 0);
                    dacc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, b, dacc[cb], 0, 0, 0);
                    ddacc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(dda, b, ddacc[cb], 0, 0, 0);
                }
            }
#pragma unroll
            for (int cb = 0; cb < NCB; cb++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float y, d1, d2;
                    activate_d2<ACT>(acc[cb][q], y, d1, d2);
                    y1[(grp * 4 + q) * YS + cb * 16 + col] = y;
                    const float s1 = dacc[cb][q];
                    dacc[cb][q] = d1 * s1;                                  // Y1', Y1'': kept in registers
                    ddacc[cb][q] = d2 * s1 * s1 + d1 * ddacc[cb][q];
                }
            wave_fence();
            // ---- layer 2 on Y1, then the tile refilled with Y1' and with Y1'' ----
#pragma unroll
            for (int cb = 0; cb < NCB; cb++) acc[cb] = f32x4{b2v[cb], b2v[cb], b2v[cb], b2v[cb]};
            mfma_layer<NCB, W>(y1 + col * YS + grp, s_w2t + grp * W + col, W / 4, acc);
            wave_fence();
#pragma unroll
            for (int cb = 0; cb < NCB; cb++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    y1[(grp * 4 + q) * YS + cb * 16 + col] = dacc[cb][q];
                    dacc[cb][q] = 0.f;
                }
            wave_fence();
            mfma_layer<NCB, W>(y1 + col * YS + grp, s_w2t + grp * W + col, W / 4, dacc);
            wave_fence();
#pragma unroll
            for (int cb = 0; cb < NCB; cb++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    y1[(grp * 4 + q) * YS + cb * 16 + col] = ddacc[cb][q];
                    ddacc[cb][q] = 0.f;
                }
            wave_fence();
            mfma_layer<NCB, W>(y1 + col * YS + grp, s_w2t + grp * W + col, W / 4, ddacc);
            // ---- my four entries of the tile ----
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int rr = grp * 4 + q;
                const float fc = ps[16 + rr], dfc = ps[32 + rr], ddfc = ps[48 + rr], rinv = ps[64 + rr], a = ps[96 + rr];
                const int j = __float_as_int(ps[80 + rr]);
                float sA = 0.f, sB1 = 0.f, sB2 = 0.f;
#pragma unroll
                for (int cb = 0; cb < NCB; cb++) {
                    const size_t c = (size_t)j * W + cb * 16 + col;
                    const float xj = x[c], gj = gout[c];
                    const float vj = V ? V[c] : 0.f;
                    const float s2 = acc[cb][q], d2 = dacc[cb][q], dd2 = ddacc[cb][q];
                    const float F = fc * s2;
                    const float F1 = dfc * s2 + fc * d2;
                    const float F2 = ddfc * s2 + 2.0f * dfc * d2 + fc * dd2;
                    acc_g[cb] += F * vj + a * F1 * xj;
                    acc_x[cb] += a * F1 * gj;
                    const float B = xj * gi[cb] + xi[cb] * gj;
                    sA += F1 * (vj * gi[cb] + vi[cb] * gj);
                    sB1 += F1 * B;
                    sB2 += F2 * B;
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    sA += __shfl_xor(sA, off, 64); sB1 += __shfl_xor(sB1, off, 64); sB2 += __shfl_xor(sB2, off, 64);
                }
                const float cu = (sA + a * sB2 - a * rinv * sB1) * rinv, cq = sB1 * rinv;
                fx -= cu * ps[112 + rr] + cq * ps[160 + rr];
                fy -= cu * ps[128 + rr] + cq * ps[176 + rr];
                fz -= cu * ps[144 + rr] + cq * ps[192 + rr];
            }
            wave_fence();
        }
        // the four lane groups hold four rows of every tile each: their sums, then one store per output
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
            acc_g[cb] += __shfl_xor(acc_g[cb], 16, 64); acc_g[cb] += __shfl_xor(acc_g[cb], 32, 64);
            acc_x[cb] += __shfl_xor(acc_x[cb], 16, 64); acc_x[cb] += __shfl_xor(acc_x[cb], 32, 64);
            if (grp == 0) {
                out_g[(size_t)i * W + cb * 16 + col] = acc_g[cb];
                out_x[(size_t)i * W + cb * 16 + col] = acc_x[cb];
            }
        }
        fx += __shfl_xor(fx, 16, 64); fx += __shfl_xor(fx, 32, 64);
        fy += __shfl_xor(fy, 16, 64); fy += __shfl_xor(fy, 32, 64);
        fz += __shfl_xor(fz, 16, 64); fz += __shfl_xor(fz, 32, 64);
        if (lane == 0) { out_pos[3 * i] = fx; out_pos[3 * i + 1] = fy; out_pos[3 * i + 2] = fz; }
    }
}

}  // namespace
