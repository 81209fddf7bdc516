// pme_recip_common.h -- what the reciprocal-space passes of pme_recip.hip (one system) and pme_frames.hip (a batch of frames) share:
// the reciprocal box, an atom's base grid index and B-spline weights, and the weight of an atom at a grid point.  One definition, so
// that a frame's float expressions are the single system's.
#pragma once

#include "device_common.h"

namespace {

struct RecipBox { float r00, r10, r11, r20, r21, r22; };

// the reciprocal box of a reduced triclinic box (lower triangular), the same float expressions as the reference's invertBoxVectors
__device__ __forceinline__ RecipBox recip_box(const float* __restrict__ b) {
    const float det = b[0] * b[4] * b[8];
    const float s = 1.0f / det;
    RecipBox r;
    r.r00 = b[4] * b[8] * s;
    r.r10 = -b[3] * b[8] * s;
    r.r11 = b[0] * b[8] * s;
    r.r20 = (b[3] * b[7] - b[4] * b[6]) * s;
    r.r21 = -b[0] * b[7] * s;
    r.r22 = b[0] * b[4] * s;
    return r;
}

// one atom: wrapped into the reduced box (c then b then a), its base grid index gi and the ORDER x 3 B-spline weights th and their
// derivatives dth (the reference's computeSpline, pmeCPU.cpp:26-70, restated): the float expressions of pme_recip_spline, statement
// for statement.  That kernel keeps its own copy: calling this function from it changed how the compiler packs the arithmetic of
// pme_recip.hip, whose bits fixtures pin.
template <int ORDER>
__device__ __forceinline__ void spline_atom(const float* __restrict__ pos, int atom, const float (&b)[9], const RecipBox& r, const int (&K)[3],
                                            int (&gi)[3], float* __restrict__ th, float* __restrict__ dth) {
    float p[3] = {pos[3 * atom], pos[3 * atom + 1], pos[3 * atom + 2]};
    const float rdiag[3] = {r.r00, r.r11, r.r22};
#pragma unroll
    for (int i = 2; i >= 0; i--) {
        const float s = floorf(p[i] * rdiag[i]);
#pragma unroll
        for (int j = 0; j < 3; j++) p[j] -= s * b[3 * i + j];
    }
    const float t3[3] = {p[0] * r.r00 + p[1] * r.r10 + p[2] * r.r20,
                         p[0] * 0.0f + p[1] * r.r11 + p[2] * r.r21,
                         p[0] * 0.0f + p[1] * 0.0f + p[2] * r.r22};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float t = (t3[i] - floorf(t3[i])) * K[i];
        const int ti = (int)t;
        const float dr = t - ti;
        gi[i] = min(max(ti % K[i], 0), K[i] - 1);          // (t can round up to exactly K; a NaN position must not index outside)
        // weights of order 2 .. ORDER-1, then the derivatives from order ORDER-1, then order ORDER
        float w[ORDER];
        w[ORDER - 1] = 0.f;
        w[1] = dr;
        w[0] = 1.f - dr;
#pragma unroll
        for (int j = 3; j < ORDER; j++) {
            const float div = 1.0f / (j - 1);
            w[j - 1] = div * dr * w[j - 2];
#pragma unroll
            for (int k = 1; k < j - 1; k++) w[j - k - 1] = div * ((dr + k) * w[j - k - 2] + (j - k - dr) * w[j - k - 1]);
            w[0] = div * (1.f - dr) * w[0];
        }
        dth[i * ORDER] = -w[0];
#pragma unroll
        for (int j = 1; j < ORDER; j++) dth[i * ORDER + j] = w[j - 1] - w[j];
        const float scale = 1.0f / (ORDER - 1);
        w[ORDER - 1] = scale * dr * w[ORDER - 2];
#pragma unroll
        for (int j = 1; j < ORDER - 1; j++) w[ORDER - j - 1] = scale * ((dr + j) * w[ORDER - j - 2] + (ORDER - j - dr) * w[ORDER - j - 1]);
        w[0] = scale * (1.f - dr) * w[0];
#pragma unroll
        for (int j = 0; j < ORDER; j++) th[i * ORDER + j] = w[j];
    }
}

// weight of the atom with base `g0` at point `g` along one axis: every stencil slot i with (g0 + i) mod K == g (a grid smaller
// than the order folds the stencil onto itself)
template <int ORDER>
__device__ __forceinline__ float axis_weight(int g, int g0, int K, const float* th) {
    int dd = g - g0;
    dd += dd < 0 ? K : 0;
    float w = 0.f;
    for (int i = dd; i < ORDER; i += K) w += th[i];
    return w;
}

}  // namespace
