// ani_tangent.h -- the tangent J.v of the AEV: its directional derivative along a per-atom vector field v.
//
// With F = -J^T g(theta, aev) the parameter gradient of a force loss is (dg/dtheta)^T (J.v), v = dL/dF: all the AEV has to add to
// the networks' own backward is J.v = d/dt aev(x + t v) at t = 0, on the lists the last compute() left behind.  Every displacement
// is d = x_j - x_i + n B with the shifts and the box held fixed, so its tangent is u' = v_j - v_i whatever the handle (vacuum,
// periodic, a batch of molecules): one kernel.  With r' = d.u' / r
//   radial   [i][species j][k]:  sum_j  scale (dfc/dr - 2 eta_k (r - Rs_k) fc) exp(-eta_k (r - Rs_k)^2) r'       (dR_k/dr of ani_radial_bwd.h)
//   angular  [i][bucket][m]:     sum over the bucket's triples of the dual part of  fcfc 2^(1-zeta) (1+cos(theta-ths))^zeta exp(-eta (rbar-Rs)^2):
//       E = 2^(1-zeta) x^(zeta-1) exp(-eta sh^2),  x = 1 + cos(theta - ths),  sh = rbar - Rs
//       term' = E ( fcfc' x  +  fcfc ( -zeta sin(theta - ths) theta'  -  2 eta sh x rbar' ) )
//     from the three per-triple scalars fcfc' = dfc_u r_u' fc_w + fc_u dfc_w r_w', rbar' = (r_u' + r_w') / 2 and
//     theta' = -damp cos(phi)' / sin(theta) -- the derivative the angular backward uses (ani_angular_generic.h: triple_forces_generic),
//     cos(phi)' = (u'.w + u.w') / (r_u r_w) - cos(phi) (r_u' / r_u + r_w' / r_w) -- for both angle conventions.
//
// Shape: one wave per atom, walking the atom's row by POSITION as the radial backward does (`order` gives the atom).
//   * radial: lane = neighbour stages {r, fc r', dfc r', species} in LDS; lane = output element (species, k) then walks the staged
//     row in row order and sums what carries its species.
//   * angular: per chunk of kTangentChunk triples, lane = triple stages the geometry and its three tangent scalars (8 floats);
//     lane = output element (bucket, m) then walks the part of ITS bucket that lies in the chunk, in the order of the triple list
//     (the list is bucket-major: bucket_offsets).  A bucket that straddles chunks is continued from the value its owner stored.
//   Every output element has one owner (element e belongs to lane e % 64 of its atom's wave), no atomics, no partial sums whose
//   order depends on timing: two calls give the same bits.  Every element is written: empty buckets and atoms without neighbours
//   get zeros.
// Each function is evaluated as given (AniParams::af_*), one log2 and one exp2 per (triple, function): the list need not factor, so
// the generic lists of the C ABI are served by the same kernel.  The factored matrix-core route of the forward (ani_angular_mfma.h)
// would share the transcendentals of a triple between its functions; it is the follow-up if this kernel ever shows in a profile.
// Reads rows, cnt_pos, recA / recB, ids, tri, bucket_offsets and the position tangent; writes its two outputs and nothing else --
// leg_force, centre_force and everything backprop() reads or leaves stay as they are.  Counts are clamped as everywhere else.
#pragma once

#include "ani_kernels.h"

namespace nnpops {

constexpr int kTangentChunk = 256;      // triples staged per pass (8 KB of LDS)

// LDS of the one wave: the staged row [cap] float4 (radial phase) shares the space of the angular phase's
// records [3][capA] float4 | staged triples [2][kTangentChunk] float4 | bucket offsets [NB + 1]
__host__ __device__ inline size_t ani_tangent_lds_bytes(int cap, int capA, int NB) {
    const size_t radial = (size_t)cap * sizeof(float4);
    const size_t angular = (size_t)capA * 3 * sizeof(float4) + (size_t)kTangentChunk * 2 * sizeof(float4) + (size_t)(NB + 1) * sizeof(int);
    return radial > angular ? radial : angular;
}

template <bool TORCHANI>
__global__ __launch_bounds__(64) void ani_tangent(const AniParams* __restrict__ P, const float4* __restrict__ nbr, int cap, int capA,
                                                  const int* __restrict__ cnt_pos, const float4* __restrict__ recA_g,
                                                  const float4* __restrict__ recB_g, const int* __restrict__ ids_g,
                                                  const int* __restrict__ tri_g,
                                                  const int* __restrict__ order,      // atoms in cell order, or NULL
                                                  const float* __restrict__ vel,      // [N][3] the position tangent
                                                  float* __restrict__ radial_t, int ld_radial, float* __restrict__ angular_t, int ld_angular) {
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    const int lane = lane_id();
    const int N = P->N, S = P->S, nR = P->nR, nA = P->nA, NB = P->NB;
    const int w = blockIdx.x;
    if (w >= N) return;
    int i = order ? order[w] : w;
    if ((unsigned)i >= (unsigned)N) i = w;                  // (a void grid build leaves no valid order: stay in bounds)
    int raw_a, raw_ro, my_species, na, nro;
    unpack_cnt_pos(cnt_pos[w], raw_a, raw_ro, my_species);
    clamp_counts(raw_a, raw_ro, cap, capA, na, nro);       // (an overflowed frame stays in bounds and is incomplete, as its forces are)
    const float vix = vel[3 * i], viy = vel[3 * i + 1], viz = vel[3 * i + 2];

    // ---- radial ----
    {
        float4* staged = (float4*)lds_raw;                  // [cap] {r, fc r', dfc r', species}
        const int total = na + nro;
        const float4* row = nbr + (size_t)w * cap;
        const float inv_rcr = P->inv_rcr;
        for (int e = lane; e < total; e += 64) {
            const float4 rec = row[e];
            const int word = __float_as_int(rec.w), j = word & kIdMask, sp = word >> kTagShift;
            float4 out = make_float4(1.f, 0.f, 0.f, __int_as_float(-1));
            if (j < N && (unsigned)sp < (unsigned)S) {
                const float ux = vel[3 * j] - vix, uy = vel[3 * j + 1] - viy, uz = vel[3 * j + 2] - viz;
                const float r = fast_sqrt(rec.x * rec.x + rec.y * rec.y + rec.z * rec.z);
                const float rdot = (rec.x * ux + rec.y * uy + rec.z * uz) * fast_rcp(r);
                float sn, cs;
                sincospi_unit(r * inv_rcr, sn, cs);
                out = make_float4(r, (0.5f * cs + 0.5f) * rdot, -(0.5f * kPi * inv_rcr) * sn * rdot, __int_as_float(sp));
            }
            staged[e] = out;
        }
        wave_fence();
        const float scale = P->radial_scale;
        float* dst = radial_t + (size_t)i * ld_radial;
        for (int q = lane; q < S * nR; q += 64) {           // q = species * nR + k
            const int sp = q / nR, k = q - sp * nR;
            const float ck = P->rad_c[k], rs = P->rad_rs[k], m2eta = -2.0f * P->rad_eta[k];
            float acc = 0.f;
            for (int e = 0; e < total; e++) {
                const float4 t = staged[e];
                const float sh = t.x - rs;
                const float term = fast_exp2(ck * sh * sh) * fmaf(m2eta * sh, t.y, t.z);
                acc += __float_as_int(t.w) == sp ? term : 0.f;
            }
            dst[q] = acc * scale;
        }
        wave_fence();                                       // (the angular phase reuses the space)
    }

    // ---- angular ----
    float4* recA = (float4*)lds_raw;                        // {dx, dy, dz, r}
    float4* recB = recA + capA;                             // {fc, dfc, 1/r, word}
    float4* udot = recB + capA;                             // {u'x, u'y, u'z, r'}
    float4* geo0 = udot + capA;                             // [chunk] {cos, sin, rbar, fcfc}
    float4* geo1 = geo0 + kTangentChunk;                    // [chunk] {fcfc', theta', rbar', -}
    int* boff = (int*)(geo1 + kTangentChunk);               // [NB + 1]
    const int n = na;
    const int T = n * (n - 1) / 2;
    {
        const float4* ra = recA_g + (size_t)i * capA;
        const float4* rb = recB_g + (size_t)i * capA;
        const int* id = ids_g + (size_t)i * capA;
        for (int e = lane; e < n; e += 64) {
            const float4 a = ra[e], b = rb[e];
            const int j = id[e];
            float ux = 0.f, uy = 0.f, uz = 0.f;
            if ((unsigned)j < (unsigned)N) { ux = vel[3 * j] - vix; uy = vel[3 * j + 1] - viy; uz = vel[3 * j + 2] - viz; }
            recA[e] = a;
            recB[e] = b;
            udot[e] = make_float4(ux, uy, uz, (a.x * ux + a.y * uy + a.z * uz) * b.z);
        }
        const int* bo = P->bucket_offsets + (size_t)i * (NB + 1);
        for (int b = lane; b <= NB; b += 64) boff[b] = max(0, min(bo[b], T));
    }
    wave_fence();
    float* out = angular_t + (size_t)i * ld_angular;
    const int* tri = tri_g + (size_t)i * triples_capacity(capA);
    const int W = NB * nA;
    for (int e = lane; e < W; e += 64) {                    // empty buckets (an atom without triples: all of them)
        const int b = e / nA;
        if (boff[b + 1] <= boff[b]) out[e] = 0.f;
    }
    const float damp = TORCHANI ? 0.95f : 1.0f;
    for (int base = 0; base < T; base += kTangentChunk) {
        const int end = min(T, base + kTangentChunk);
        for (int t = base + lane; t < end; t += 64) {       // lane = triple: what does not depend on the function
            const int word = tri[t];
            const int p = min(word & 0xff, n - 1), q = min((word >> 8) & 0xff, n - 1);
            const float4 A = recA[p], A2 = recB[p], B = recA[q], B2 = recB[q], U = udot[p], V = udot[q];
            const TripleGeom g = triple_geometry<TORCHANI>(A, A2, B, B2);
            const float iprod = A2.z * B2.z;
            const float cosphi = (A.x * B.x + A.y * B.y + A.z * B.z) * iprod;
            const float mixed = (U.x * B.x + U.y * B.y + U.z * B.z) + (A.x * V.x + A.y * V.y + A.z * V.z);
            const float cosdot = mixed * iprod - cosphi * (U.w * A2.z + V.w * B2.z);
            const float thdot = -damp * fast_rcp(g.s) * cosdot;
            const float fcfcdot = A2.y * U.w * B2.x + A2.x * B2.y * V.w;
            geo0[t - base] = make_float4(g.c, g.s, g.rbar, g.fcfc);
            geo1[t - base] = make_float4(fcfcdot, thdot, 0.5f * (U.w + V.w), 0.f);
        }
        wave_fence();
        for (int e = lane; e < W; e += 64) {                // lane = output element (bucket, function): the owner of out[e]
            const int b = e / nA, m = e - b * nA;
            const int first = boff[b], lo = max(first, base), hi = min(boff[b + 1], end);
            if (lo >= hi) continue;
            const float cm = P->af_c[m], rs = P->af_rs[m], zeta = P->af_zeta[m], zc = P->af_cos[m], zs = P->af_sin[m];
            const float m2eta = -2.0f * P->af_eta[m];
            float acc = first < base ? out[e] : 0.f;        // (a bucket that began in an earlier chunk: this lane stored its sum so far)
            for (int t = lo - base; t < hi - base; t++) {
                const float4 g = geo0[t], d = geo1[t];
                const float x = fmaxf(1.0f + (g.x * zc + g.y * zs), 1e-30f);      // 1 + cos(theta - thetas_m)
                const float sz = g.y * zc - g.x * zs;                              // sin(theta - thetas_m)
                const float sh = g.z - rs;
                const float E = fast_exp2(fmaf(zeta - 1.0f, fast_log2(x), (1.0f - zeta) + cm * sh * sh));
                acc += E * fmaf(d.x, x, g.w * fmaf(m2eta * sh * x, d.z, -zeta * sz * d.y));
            }
            out[e] = acc;
        }
        wave_fence();
    }
}

}  // namespace nnpops
