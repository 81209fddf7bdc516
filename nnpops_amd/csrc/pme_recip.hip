// pme_recip.hip -- reciprocal-space part of Particle Mesh Ewald (smooth PME, Essmann et al. 1995).
//
// Replaces the reference's computeReciprocal (reference src/pytorch/pme/pmeCUDA.cu:102-430, CPU form
// src/pytorch/pme/pmeCPU.cpp:174-364).  The caller runs the two FFTs (torch.fft / hipFFT); this file holds the passes around
// them:
//   spread       positions, charges -> real grid Q[Kx][Ky][Kz] = sum_atoms q sqrt(coulomb) thx thy thz at (base + i) mod K
//   convolve     complex grid [Kx][Ky][Kz/2+1] (rfftn of Q, default norm) *= eterm in place; energy = 0.5 sum w eterm |S|^2
//   interpolate  real grid (irfftn of the scaled complex grid, norm="forward") -> dE/dpositions, dE/dcharges
//
// Layout for MI355X: NO float atomics, everything bitwise reproducible (the reference scatters order^3 float atomics per atom).
//   pme_recip_spline     one lane per atom: wraps the atom into the box (z -> y -> x), stores the base grid index and the order x 3
//                        B-spline weights and derivative weights in the workspace (the backward reuses them), and counts the atom
//                        into the BRICK (4 x 4 x 16 grid points) of its base index with one integer atomic.
//   pme_recip_scan       one workgroup: exclusive prefix of the brick counts.
//   pme_recip_scatter    one lane per atom: a slot inside its brick's range (integer atomic: the order inside a brick is arbitrary)
//   pme_recip_order      one wave per brick: the brick's atoms re-placed in ascending atom index (rank sort) -- the order the
//                        spread adds them in no longer depends on the atomics.
//   pme_recip_gather     one workgroup per brick of grid points, one lane per point (OWNER COMPUTES): the atoms whose base lies in
//                        the brick or in its (order - 1) halo below are staged in LDS, brick after brick in a fixed order and in
//                        ascending atom index inside a brick; every lane adds what reaches its point.  Every point is written
//                        exactly once, so the grid needs no clearing.
//   pme_recip_convolve   one lane per complex point; energy in double per workgroup, the partials summed in a fixed order.
//   pme_recip_interp     one lane per atom: order^3 gather with the stored weights, owner computes.
// The box gradient: with E = 0.5 sum_k w E'_k, b = pi^2 / alpha^2, g_j = dE/dx_j,
//     dE/dB = - B^-T (Pi + X),   Pi = 0.5 sum_k w E'_k [I - 2 (b + 1/|m|^2) m m^T],   X = sum_j x_j (x) g_j
//   pme_recip_box_pi          after the convolution, one lane per complex point: Pi in double per workgroup from the scaled grid;
//   pme_recip_box_atoms       one lane per atom: X in double per workgroup from the positions and the interpolated g;
//   pme_recip_box_finish      one workgroup: both sums in a fixed order, then - B^-T (Pi + X).
// Second derivatives with respect to positions and charges: pme_recip_spline2, pme_recip_gather_dir and pme_recip_interp2,
// described where they stand below; they read what the passes above left in the workspace and leave those passes as they are.
// The box is read on the device by every pass (never copied to the host): a captured graph follows new box values written in place.
#include <cmath>

#include "device_common.h"
#include "host_common.h"

using namespace nnpops;

namespace {

constexpr int kBlock = 256;
constexpr int kBX = 4, kBY = 4, kBZ = 16;              // brick of grid points = one gather workgroup (kBX * kBY * kBZ == kBlock)
constexpr int kMaxBinsPerAxis = 4;                     // bricks a cyclic window of (brick + order - 1) cells can touch
constexpr int kConvBlocksMax = 1024;
static_assert(kBX * kBY * kBZ == kBlock, "one lane per grid point of a brick");

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

struct Dims {
    int kx, ky, kz;          // grid
    int nbx, nby, nbz;       // bricks per axis
    long long nbins;
};

Dims make_dims(int gx, int gy, int gz) {
    Dims d{gx, gy, gz, div_up(gx, kBX), div_up(gy, kBY), div_up(gz, kBZ), 0};
    d.nbins = (long long)d.nbx * d.nby * d.nbz;
    return d;
}

int conv_blocks(int gx, int gy, int gz) {
    const long long points = (long long)gx * gy * (gz / 2 + 1);
    return (int)std::min<long long>(std::max<long long>(1, (points + kBlock - 1) / kBlock), kConvBlocksMax);
}

// ---- workspace: ONE carve, used by the size query and by every entry point (they must agree) ----
struct RecipWorkspace {
    double* partial;      // [conv_blocks]
    int* bin_count;       // [nbins]        integer histogram (zeroed by spread)
    int* bin_start;       // [nbins + 1]    exclusive prefix
    int* cursor;          // [nbins]        scatter cursors
    int* unsorted;        // [N]            atoms by brick, arbitrary order inside a brick
    int* sorted;          // [N]            atoms by brick, ascending inside a brick
    int4* base;           // [N]            base grid index (x, y, z, brick)
    float* theta;         // [N][3][order]  B-spline weights
    float* dtheta;        // [N][3][order]  their derivatives
    size_t bytes;
};

RecipWorkspace carve(void* workspace, int num_atoms, int gx, int gy, int gz, int order) {
    const Dims d = make_dims(gx, gy, gz);
    RecipWorkspace w{};
    uintptr_t p = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    auto take = [&](size_t bytes) { const uintptr_t at = p; p += (bytes + 255) & ~(size_t)255; return at; };
    const size_t n = (size_t)num_atoms;
    w.partial = (double*)take(sizeof(double) * conv_blocks(gx, gy, gz));
    w.bin_count = (int*)take(sizeof(int) * (size_t)d.nbins);
    w.bin_start = (int*)take(sizeof(int) * ((size_t)d.nbins + 1));
    w.cursor = (int*)take(sizeof(int) * (size_t)d.nbins);
    w.unsorted = (int*)take(sizeof(int) * n);
    w.sorted = (int*)take(sizeof(int) * n);
    w.base = (int4*)take(sizeof(int4) * n);
    w.theta = (float*)take(sizeof(float) * 3 * (size_t)order * n);
    w.dtheta = (float*)take(sizeof(float) * 3 * (size_t)order * n);
    w.bytes = (size_t)(p - (uintptr_t)workspace) + 256;
    return w;
}

// ---- the box gradient's own workspace (the one above keeps its size): Pi from the convolution, X from the atoms ----
struct BoxWorkspace {
    double* pi_partial;   // [conv_blocks][6]
    double* x_partial;    // [ceil(N / kBlock)][9]
    size_t bytes;
};

BoxWorkspace box_carve(void* workspace, int num_atoms, int gx, int gy, int gz) {
    BoxWorkspace w{};
    uintptr_t p = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    auto take = [&](size_t bytes) { const uintptr_t at = p; p += (bytes + 255) & ~(size_t)255; return at; };
    w.pi_partial = (double*)take(sizeof(double) * 6 * conv_blocks(gx, gy, gz));
    w.x_partial = (double*)take(sizeof(double) * 9 * (size_t)std::max(1, div_up(num_atoms, kBlock)));
    w.bytes = (size_t)(p - (uintptr_t)workspace) + 256;
    return w;
}

// ---- pass 1: wrap, base index, B-spline weights (the reference's computeSpline, pmeCPU.cpp:26-70, restated) ----
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_spline(int num_atoms, const float* __restrict__ pos, const float* __restrict__ box,
                                                           Dims d, int4* __restrict__ base, float* __restrict__ theta,
                                                           float* __restrict__ dtheta, int* __restrict__ bin_count) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= num_atoms) return;
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = box[i];
    const RecipBox r = recip_box(b);
    float p[3] = {pos[3 * atom], pos[3 * atom + 1], pos[3 * atom + 2]};
    // into the reduced box, c then b then a
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
    const int K[3] = {d.kx, d.ky, d.kz};
    int gi[3];
    float* th = theta + (size_t)atom * 3 * ORDER;
    float* dth = dtheta + (size_t)atom * 3 * ORDER;
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
    const int bin = (int)(((long long)(gi[0] / kBX) * d.nby + gi[1] / kBY) * d.nbz + gi[2] / kBZ);
    base[atom] = make_int4(gi[0], gi[1], gi[2], bin);
    atomicAdd(&bin_count[bin], 1);                        // integer: the counts are exact whatever the order
}

// ---- pass 2: exclusive prefix of the brick counts (one workgroup of 1 024 lanes walking the counts 1 024 at a time, coalesced) ----
__global__ __launch_bounds__(1024) void pme_recip_scan(long long nbins, const int* __restrict__ count, int* __restrict__ start,
                                                       int* __restrict__ cursor) {
    __shared__ int wave_sums[1024 / 64];
    int carry = 0;
    for (long long c0 = 0; c0 < nbins; c0 += 1024) {
        const long long i = c0 + threadIdx.x;
        const int v = i < nbins ? count[i] : 0;
        int incl = v;                                     // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int u = __shfl_up(incl, off, 64);
            if (lane_id() >= off) incl += u;
        }
        if (lane_id() == 63) wave_sums[threadIdx.x >> 6] = incl;
        __syncthreads();
        int before = carry, all = 0;                      // (16 wave sums: every lane adds them up itself)
        for (int w = 0; w < 1024 / 64; w++) {
            const int ws = wave_sums[w];
            before += w < (int)(threadIdx.x >> 6) ? ws : 0;
            all += ws;
        }
        if (i < nbins) {
            start[i] = before + incl - v;
            cursor[i] = before + incl - v;
        }
        carry += all;
        __syncthreads();                                  // (wave_sums is rewritten by the next chunk)
    }
    if (threadIdx.x == 0) start[nbins] = carry;
}

// ---- pass 3: every atom into its brick's range (arbitrary order inside the brick) ----
__global__ __launch_bounds__(kBlock) void pme_recip_scatter(int num_atoms, const int4* __restrict__ base, int* __restrict__ cursor,
                                                            int* __restrict__ unsorted) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= num_atoms) return;
    unsorted[atomicAdd(&cursor[base[atom].w], 1)] = atom;
}

// ---- pass 4: inside every brick, ascending atom index (rank sort, one wave per brick; atom indices are distinct) ----
__global__ __launch_bounds__(kBlock) void pme_recip_order(long long nbins, const int* __restrict__ start, const int* __restrict__ unsorted,
                                                          int* __restrict__ sorted) {
    const long long waves = (long long)gridDim.x * (kBlock / 64);
    for (long long bin = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); bin < nbins; bin += waves) {
        const int s = start[bin], e = start[bin + 1];
        for (int k = s + lane_id(); k < e; k += 64) {
            const int a = unsorted[k];
            int rank = 0;
            for (int j = s; j < e; j++) rank += unsorted[j] < a;
            sorted[s + rank] = a;
        }
    }
}

// bricks along one axis whose cells hold the base index of an atom that reaches a point of brick `b`: the cyclic window
// [b*B - (order-1), b*B + B - 1] mod K, in window order (a fixed order: the gather's sum order follows it)
__device__ int window_bins(int b, int B, int K, int nb, int order, int* out) {
    const int len = B + order - 1;
    if (len >= K) {                                       // the window covers the whole axis
        for (int i = 0; i < nb; i++) out[i] = i;
        return nb;
    }
    int n = 0;
    const int first = ((b * B - (order - 1)) % K + K) % K;
    for (int j = 0; j < len; j++) {
        const int bin = ((first + j) % K) / B;
        bool seen = false;
        for (int i = 0; i < n; i++) seen |= out[i] == bin;
        if (!seen && n < kMaxBinsPerAxis) out[n++] = bin;       // (never more than kMaxBinsPerAxis: see kMaxBinsPerAxis)
    }
    return n;
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

// ---- pass 5: the spread as a gather, one workgroup per brick of grid points ----
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_gather(Dims d, const int* __restrict__ start, const int* __restrict__ sorted,
                                                           const int4* __restrict__ base, const float* __restrict__ theta,
                                                           const float* __restrict__ charge, float sqrt_coulomb,
                                                           float* __restrict__ grid) {
    __shared__ int s_bx[kMaxBinsPerAxis], s_by[kMaxBinsPerAxis], s_bz[kMaxBinsPerAxis];
    __shared__ int s_first[kMaxBinsPerAxis * kMaxBinsPerAxis * kMaxBinsPerAxis];
    __shared__ int s_prefix[kMaxBinsPerAxis * kMaxBinsPerAxis * kMaxBinsPerAxis + 1];
    __shared__ int s_ntrip;
    __shared__ int s_base[3][kBlock];
    __shared__ float s_th[3 * ORDER][kBlock];              // [axis * ORDER + i][slot]: x weights carry q sqrt(coulomb)

    const int brick = blockIdx.x;
    const int bz = brick % d.nbz, by = (brick / d.nbz) % d.nby, bx = brick / (d.nbz * d.nby);
    __shared__ int s_n[3], s_count[kMaxBinsPerAxis * kMaxBinsPerAxis * kMaxBinsPerAxis];
    // three lanes find the windows along x, y, z; one lane per brick of the window reads its range; one lane adds them up
    if (threadIdx.x == 0) s_n[0] = window_bins(bx, kBX, d.kx, d.nbx, ORDER, s_bx);
    if (threadIdx.x == 64) s_n[1] = window_bins(by, kBY, d.ky, d.nby, ORDER, s_by);
    if (threadIdx.x == 128) s_n[2] = window_bins(bz, kBZ, d.kz, d.nbz, ORDER, s_bz);
    __syncthreads();
    const int nx = s_n[0], ny = s_n[1], nz = s_n[2];
    if ((int)threadIdx.x < nx * ny * nz) {                // window order: x outermost, z innermost
        const int i = threadIdx.x / (ny * nz), j = (threadIdx.x / nz) % ny, k = threadIdx.x % nz;
        const long long bin = ((long long)s_bx[i] * d.nby + s_by[j]) * d.nbz + s_bz[k];
        const int first = start[bin];
        s_first[threadIdx.x] = first;
        s_count[threadIdx.x] = start[bin + 1] - first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        const int t = nx * ny * nz;
        for (int u = 0; u < t; u++) { s_prefix[u] = total; total += s_count[u]; }
        s_prefix[t] = total;
        s_ntrip = t;
    }
    __syncthreads();
    const int ntrip = s_ntrip, total = s_prefix[ntrip];
    const int gx = bx * kBX + (threadIdx.x / (kBY * kBZ)), gy = by * kBY + (threadIdx.x / kBZ) % kBY, gz = bz * kBZ + threadIdx.x % kBZ;
    const bool live = gx < d.kx && gy < d.ky && gz < d.kz;
    float acc = 0.f;
    for (int c0 = 0; c0 < total; c0 += kBlock) {
        const int f = c0 + threadIdx.x;
        if (f < total) {
            int t = 0;
            while (s_prefix[t + 1] <= f) t++;
            const int atom = sorted[s_first[t] + (f - s_prefix[t])];
            const int4 b0 = base[atom];
            s_base[0][threadIdx.x] = b0.x; s_base[1][threadIdx.x] = b0.y; s_base[2][threadIdx.x] = b0.z;
            const float qs = charge[atom] * sqrt_coulomb;
            const float* th = theta + (size_t)atom * 3 * ORDER;
#pragma unroll
            for (int i = 0; i < ORDER; i++) s_th[i][threadIdx.x] = qs * th[i];
#pragma unroll
            for (int i = ORDER; i < 3 * ORDER; i++) s_th[i][threadIdx.x] = th[i];
        }
        __syncthreads();
        const int m = min(kBlock, total - c0);
        if (live) {
            for (int k = 0; k < m; k++) {
                float tx[ORDER], ty[ORDER], tz[ORDER];
#pragma unroll
                for (int i = 0; i < ORDER; i++) { tx[i] = s_th[i][k]; ty[i] = s_th[ORDER + i][k]; tz[i] = s_th[2 * ORDER + i][k]; }
                const float wx = axis_weight<ORDER>(gx, s_base[0][k], d.kx, tx);
                const float wy = axis_weight<ORDER>(gy, s_base[1][k], d.ky, ty);
                const float wz = axis_weight<ORDER>(gz, s_base[2][k], d.kz, tz);
                acc += wx * wy * wz;
            }
        }
        __syncthreads();
    }
    if (live) grid[((size_t)gx * d.ky + gy) * d.kz + gz] = acc;
}

// ---- convolution with the Ewald kernel (pmeCPU.cpp:229-262 semantics), energy in double ----
__global__ __launch_bounds__(kBlock) void pme_recip_convolve(int gx, int gy, int gz, const float* __restrict__ box, float recip_exp_factor,
                                                            const float* __restrict__ xmod, const float* __restrict__ ymod,
                                                            const float* __restrict__ zmod, float2* __restrict__ cgrid,
                                                            double* __restrict__ partial) {
    __shared__ double red[kBlock / 64];
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = box[i];
    const RecipBox r = recip_box(b);
    const float scale_factor = (float)M_PI * b[0] * b[4] * b[8];
    const int zsize = gz / 2 + 1;
    const long long points = (long long)gx * gy * zsize;
    double energy = 0.0;
    for (long long idx = (long long)blockIdx.x * kBlock + threadIdx.x; idx < points; idx += (long long)gridDim.x * kBlock) {
        const int kx = (int)(idx / ((long long)gy * zsize));
        const int rem = (int)(idx - (long long)kx * gy * zsize);
        const int ky = rem / zsize, kz = rem - ky * zsize;
        const int mx = kx < (gx + 1) / 2 ? kx : kx - gx;
        const int my = ky < (gy + 1) / 2 ? ky : ky - gy;
        const int mz = kz < (gz + 1) / 2 ? kz : kz - gz;
        const float mhx = mx * r.r00;
        const float mhy = mx * r.r10 + my * r.r11;
        const float mhz = mx * r.r20 + my * r.r21 + mz * r.r22;
        const float m2 = mhx * mhx + mhy * mhy + mhz * mhz;
        const float denom = m2 * (scale_factor * xmod[kx]) * ymod[ky] * zmod[kz];
        const float eterm = idx == 0 ? 0.f : expf(-recip_exp_factor * m2) / denom;
        const float w = (kz > 0 && kz <= (gz - 1) / 2) ? 2.f : 1.f;
        float2 g = cgrid[idx];
        energy += (double)(w * eterm * (g.x * g.x + g.y * g.y));
        g.x *= eterm; g.y *= eterm;
        cgrid[idx] = g;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) energy += __shfl_xor(energy, off, 64);
    if (lane_id() == 0) red[threadIdx.x >> 6] = energy;
    __syncthreads();
    if (threadIdx.x == 0) {
        double e = 0.0;
        for (int w = 0; w < kBlock / 64; w++) e += red[w];
        partial[blockIdx.x] = e;
    }
}

// ---- box gradient: Pi = 0.5 sum_{k != 0} w E'_k [I - 2 (b + 1/|m|^2) m m^T] (E'_k = eterm |S|^2, b = pi^2 / alpha^2) ----
// A pass of its own over the grid pme_recip_convolve has scaled (g' = eterm S, so w E'_k = w |g'|^2 / eterm), leaving that kernel and
// its bits exactly as they are: a variant that also formed Pi from the same float values was compiled with other contractions of |m|^2
// (the extra uses change how the vectoriser packs them), so its eterm, and the grid, could differ in the last bit.  Per workgroup, in
// double, into pi_partial [gridDim][6] (xx, yy, zz, xy, xz, yz; without the 1/2).  Points whose eterm underflows add nothing.
__global__ __launch_bounds__(kBlock) void pme_recip_box_pi(int gx, int gy, int gz, const float* __restrict__ box, float recip_exp_factor,
                                                          const float* __restrict__ xmod, const float* __restrict__ ymod,
                                                          const float* __restrict__ zmod, const float2* __restrict__ cgrid,
                                                          double* __restrict__ pi_partial) {
    __shared__ double red[kBlock / 64][6];
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = box[i];
    const RecipBox r = recip_box(b);
    const float scale_factor = (float)M_PI * b[0] * b[4] * b[8];
    const int zsize = gz / 2 + 1;
    const long long points = (long long)gx * gy * zsize;
    double pi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long idx = (long long)blockIdx.x * kBlock + threadIdx.x; idx < points; idx += (long long)gridDim.x * kBlock) {
        if (idx == 0) continue;
        const int kx = (int)(idx / ((long long)gy * zsize));
        const int rem = (int)(idx - (long long)kx * gy * zsize);
        const int ky = rem / zsize, kz = rem - ky * zsize;
        const int mx = kx < (gx + 1) / 2 ? kx : kx - gx;
        const int my = ky < (gy + 1) / 2 ? ky : ky - gy;
        const int mz = kz < (gz + 1) / 2 ? kz : kz - gz;
        const float mhx = mx * r.r00;
        const float mhy = mx * r.r10 + my * r.r11;
        const float mhz = mx * r.r20 + my * r.r21 + mz * r.r22;
        const float m2 = mhx * mhx + mhy * mhy + mhz * mhz;
        const float denom = m2 * (scale_factor * xmod[kx]) * ymod[ky] * zmod[kz];
        const float eterm = expf(-recip_exp_factor * m2) / denom;
        if (!(eterm > 0.f)) continue;
        const float w = (kz > 0 && kz <= (gz - 1) / 2) ? 2.f : 1.f;
        const float2 g = cgrid[idx];
        const double t = (double)w * ((double)g.x * g.x + (double)g.y * g.y) / (double)eterm;
        const double c = 2.0 * ((double)recip_exp_factor + 1.0 / (double)m2);
        const double hx = mhx, hy = mhy, hz = mhz;
        pi[0] += t * (1.0 - c * hx * hx); pi[1] += t * (1.0 - c * hy * hy); pi[2] += t * (1.0 - c * hz * hz);
        pi[3] -= t * c * hx * hy;         pi[4] -= t * c * hx * hz;         pi[5] -= t * c * hy * hz;
    }
#pragma unroll
    for (int q = 0; q < 6; q++)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) pi[q] += __shfl_xor(pi[q], off, 64);
    if (lane_id() == 0) {
#pragma unroll
        for (int q = 0; q < 6; q++) red[threadIdx.x >> 6][q] = pi[q];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; w++) s += red[w][threadIdx.x];
        pi_partial[(size_t)blockIdx.x * 6 + threadIdx.x] = s;
    }
}

// ---- box gradient: X = sum_j x_j (x) g_j from the positions and the interpolated dE/dpositions, float64 per workgroup ----
__global__ __launch_bounds__(kBlock) void pme_recip_box_atoms(int num_atoms, const float* __restrict__ pos, const float* __restrict__ pos_deriv,
                                                             double* __restrict__ x_partial) {
    __shared__ double red[kBlock / 64][9];
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom < num_atoms) {
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) acc[3 * a + b] = (double)pos[3 * atom + a] * (double)pos_deriv[3 * atom + b];
    }
#pragma unroll
    for (int q = 0; q < 9; q++)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
    if (lane_id() == 0) {
#pragma unroll
        for (int q = 0; q < 9; q++) red[threadIdx.x >> 6][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; w++) s += red[w][threadIdx.x];
        x_partial[(size_t)blockIdx.x * 9 + threadIdx.x] = s;
    }
}

// one workgroup: Pi (1/2 x the convolution's partials) and X (the atom partials), each added up in a fixed order, then
// dE/dB = - B^-T (Pi + X) with B^-1 the general 3 x 3 inverse of the box in double (for the reduced box the kernels take it equals
// the lower-triangular one of recip_box)
__global__ __launch_bounds__(kBlock) void pme_recip_box_finish(int pi_blocks, const double* __restrict__ pi_partial, int x_blocks,
                                                              const double* __restrict__ x_partial, const float* __restrict__ box,
                                                              float* __restrict__ grad_box) {
    __shared__ double red[kBlock / 64][15];
    double acc[15];
#pragma unroll
    for (int q = 0; q < 15; q++) acc[q] = 0.0;
    for (int b = threadIdx.x; b < pi_blocks; b += kBlock) {
#pragma unroll
        for (int q = 0; q < 6; q++) acc[q] += pi_partial[(size_t)b * 6 + q];
    }
    for (int b = threadIdx.x; b < x_blocks; b += kBlock) {
#pragma unroll
        for (int q = 0; q < 9; q++) acc[6 + q] += x_partial[(size_t)b * 9 + q];
    }
#pragma unroll
    for (int q = 0; q < 15; q++)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
    if (lane_id() == 0) {
#pragma unroll
        for (int q = 0; q < 15; q++) red[threadIdx.x >> 6][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[15];
        for (int q = 0; q < 15; q++) {
            s[q] = red[0][q];
            for (int w = 1; w < kBlock / 64; w++) s[q] += red[w][q];
        }
        const double pxx = 0.5 * s[0], pyy = 0.5 * s[1], pzz = 0.5 * s[2], pxy = 0.5 * s[3], pxz = 0.5 * s[4], pyz = 0.5 * s[5];
        const double M[9] = {pxx + s[6], pxy + s[7], pxz + s[8], pxy + s[9], pyy + s[10], pyz + s[11], pxz + s[12], pyz + s[13], pzz + s[14]};
        double B[9];
        for (int q = 0; q < 9; q++) B[q] = (double)box[q];
        // B^-1 = adj(B) / det(B)
        const double c00 = B[4] * B[8] - B[5] * B[7], c01 = B[5] * B[6] - B[3] * B[8], c02 = B[3] * B[7] - B[4] * B[6];
        const double det = B[0] * c00 + B[1] * c01 + B[2] * c02;
        const double inv[9] = {c00 / det, (B[2] * B[7] - B[1] * B[8]) / det, (B[1] * B[5] - B[2] * B[4]) / det,
                               c01 / det, (B[0] * B[8] - B[2] * B[6]) / det, (B[2] * B[3] - B[0] * B[5]) / det,
                               c02 / det, (B[1] * B[6] - B[0] * B[7]) / det, (B[0] * B[4] - B[1] * B[3]) / det};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++)       // (B^-T M)[a][b] = sum_c B^-1[c][a] M[c][b]
                grad_box[3 * a + b] = (float)-(inv[a] * M[b] + inv[3 + a] * M[3 + b] + inv[6 + a] * M[6 + b]);
    }
}

// workgroup partials -> 0.5 x their sum, always in the same order
__global__ __launch_bounds__(kConvBlocksMax) void pme_recip_energy(const double* __restrict__ partial, int count, float* __restrict__ energy) {
    __shared__ double red[kConvBlocksMax];
    red[threadIdx.x] = (int)threadIdx.x < count ? partial[threadIdx.x] : 0.0;
    __syncthreads();
    for (int off = kConvBlocksMax / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *energy = (float)(0.5 * red[0]);
}

// ---- interpolation: dE/dpositions, dE/dcharges from the irfftn of the scaled complex grid ----
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_interp(int num_atoms, Dims d, const float* __restrict__ box,
                                                           const float* __restrict__ charge, float sqrt_coulomb,
                                                           const int4* __restrict__ base, const float* __restrict__ theta,
                                                           const float* __restrict__ dtheta, const float* __restrict__ grid,
                                                           float* __restrict__ pos_deriv, float* __restrict__ charge_deriv) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= num_atoms) return;
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = box[i];
    const RecipBox r = recip_box(b);
    const int4 b0 = base[atom];
    const float* th = theta + (size_t)atom * 3 * ORDER;
    const float* dth = dtheta + (size_t)atom * 3 * ORDER;
    float tx[ORDER], ty[ORDER], tz[ORDER], dx[ORDER], dy[ORDER], dz[ORDER];
    int ix[ORDER], iy[ORDER], iz[ORDER];
#pragma unroll
    for (int i = 0; i < ORDER; i++) {
        tx[i] = th[i]; ty[i] = th[ORDER + i]; tz[i] = th[2 * ORDER + i];
        dx[i] = dth[i]; dy[i] = dth[ORDER + i]; dz[i] = dth[2 * ORDER + i];
        ix[i] = (b0.x + i) % d.kx; iy[i] = (b0.y + i) % d.ky; iz[i] = (b0.z + i) % d.kz;
    }
    float gx = 0.f, gy = 0.f, gz = 0.f, dq = 0.f;
#pragma unroll
    for (int a = 0; a < ORDER; a++) {
#pragma unroll
        for (int c = 0; c < ORDER; c++) {
            const float* row = grid + ((size_t)ix[a] * d.ky + iy[c]) * d.kz;
#pragma unroll
            for (int e = 0; e < ORDER; e++) {
                const float g = row[iz[e]];
                gx += dx[a] * ty[c] * tz[e] * g;
                gy += tx[a] * dy[c] * tz[e] * g;
                gz += tx[a] * ty[c] * dz[e] * g;
                dq += tx[a] * ty[c] * tz[e] * g;
            }
        }
    }
    const float s = charge[atom] * sqrt_coulomb;
    const float fx = gx * d.kx, fy = gy * d.ky, fz = gz * d.kz;
    pos_deriv[3 * atom] = s * (fx * r.r00);
    pos_deriv[3 * atom + 1] = s * (fx * r.r10 + fy * r.r11);
    pos_deriv[3 * atom + 2] = s * (fx * r.r20 + fy * r.r21 + fz * r.r22);
    charge_deriv[atom] = dq * sqrt_coulomb;
}

// =====================================================================================================================================
// Second order: the double backward with respect to positions and charges.  W_i(m) = atom i's separable weight at grid
// point m, Q = sum_i q_i W_i the charge grid, phi = G * Q the potential grid (the irfftn the interpolation reads).  With cotangents
// v [N][3] of the position gradient and w [N] of the charge gradient, L = sum_i v_i . dE/dx_i + sum_i w_i dE/dq_i = Q' . phi with
//     Q'  = sum_i [w_i W_i + q_i (v_i . grad) W_i]        pme_recip_gather_dir: the forward's bricks and sorted atoms, no second sort
//     phi' = G * Q'                                        the caller: rfftn -> nnpops_pme_reciprocal_convolve -> irfftn
//     dL/dq_j = W_j . phi' + ((v_j . grad) W_j) . phi
//     dL/dx_j = q_j grad W_j . phi' + q_j grad((v_j . grad) W_j) . phi + w_j grad W_j . phi      pme_recip_interp2
// (v . grad) W along axis a is s_a dtheta_a times the other two axes' theta, s_a = K_a (v . B^-1 column a); its gradient needs
// d2theta (the order-(n-2) weights differenced twice) and the mixed products dtheta_a dtheta_b theta_c.  pme_recip_spline2 recomputes
// the fractional offset from the positions exactly as pme_recip_spline does and stores theta, dtheta, d2theta (in double) and s in a
// workspace of its own.
// The first-order kernels above are not touched.
struct SecondWorkspace {
    double* wide;         // [N][3][3][order]  theta, dtheta, d2theta of the three axes, in double (see pme_recip_spline2)
    float* dir;           // [N][3]        s_a = K_a (v . B^-1 column a)
    size_t bytes;
};

SecondWorkspace second_carve(void* workspace, int num_atoms, int order) {
    SecondWorkspace w{};
    uintptr_t p = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    auto take = [&](size_t bytes) { const uintptr_t at = p; p += (bytes + 255) & ~(size_t)255; return at; };
    w.wide = (double*)take(sizeof(double) * 9 * (size_t)order * (size_t)num_atoms);
    w.dir = (float*)take(sizeof(float) * 3 * (size_t)num_atoms);
    w.bytes = (size_t)(p - (uintptr_t)workspace) + 256;
    return w;
}

template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_spline2(int num_atoms, const float* __restrict__ pos, const float* __restrict__ box,
                                                            Dims d, const int4* __restrict__ base, const float* __restrict__ v,
                                                            double* __restrict__ wide, float* __restrict__ dir) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= num_atoms) return;
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = box[i];
    const RecipBox r = recip_box(b);
    float p[3] = {pos[3 * atom], pos[3 * atom + 1], pos[3 * atom + 2]};
    const float rdiag[3] = {r.r00, r.r11, r.r22};
#pragma unroll
    for (int i = 2; i >= 0; i--) {                        // into the reduced box, c then b then a (as pme_recip_spline)
        const float s = floorf(p[i] * rdiag[i]);
#pragma unroll
        for (int j = 0; j < 3; j++) p[j] -= s * b[3 * i + j];
    }
    const float t3[3] = {p[0] * r.r00 + p[1] * r.r10 + p[2] * r.r20,
                         p[0] * 0.0f + p[1] * r.r11 + p[2] * r.r21,
                         p[0] * 0.0f + p[1] * 0.0f + p[2] * r.r22};
    const int K[3] = {d.kx, d.ky, d.kz};
    const int4 b0 = base[atom];
    const int g0[3] = {b0.x, b0.y, b0.z};
    double* wd = wide + (size_t)atom * 9 * ORDER;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float t = (t3[i] - floorf(t3[i])) * K[i];
        const int ti = (int)t;
        float dr = t - ti;
        // the base index is the forward pass's: should this pass round the offset to the other side of a grid line, take the end of
        // the forward's cell (the weights are continuous there)
        const int gi = min(max(ti % K[i], 0), K[i] - 1);
        if (gi != g0[i]) dr = ((gi - g0[i] + K[i]) % K[i] == 1) ? 1.0f : 0.0f;
        // The recursion of pme_recip_spline in double from the float offset, kept at orders ORDER - 2 (differenced twice: d2theta),
        // ORDER - 1 (differenced: dtheta) and ORDER (theta).  pme_recip_interp2 takes all three from here: d2theta sums to zero
        // over the stencil, and float weights, which do so only to rounding, left an error of that rounding times phi itself.
        const double x = dr;
        double w[ORDER];
#pragma unroll
        for (int j = 0; j < ORDER; j++) w[j] = 0.0;
        w[1] = x;
        w[0] = 1.0 - x;
        auto raise = [&](int j) {
            const double div = 1.0 / (j - 1);
            w[j - 1] = div * x * w[j - 2];
#pragma unroll
            for (int k = 1; k < j - 1; k++) w[j - k - 1] = div * ((x + k) * w[j - k - 2] + (j - k - x) * w[j - k - 1]);
            w[0] = div * (1.0 - x) * w[0];
        };
#pragma unroll
        for (int j = 3; j <= ORDER - 2; j++) raise(j);
#pragma unroll
        for (int j = 0; j < ORDER; j++) {
            const double lo = j >= 2 ? w[j - 2] : 0.0, mid = j >= 1 ? w[j - 1] : 0.0;      // (w[ORDER-2], w[ORDER-1] are zero)
            wd[(6 + i) * ORDER + j] = lo - 2.0 * mid + w[j];
        }
        raise(ORDER - 1);
        wd[(3 + i) * ORDER] = -w[0];
#pragma unroll
        for (int j = 1; j < ORDER; j++) wd[(3 + i) * ORDER + j] = w[j - 1] - w[j];
        raise(ORDER);
#pragma unroll
        for (int j = 0; j < ORDER; j++) wd[i * ORDER + j] = w[j];
    }
    const float vx = v[3 * atom], vy = v[3 * atom + 1], vz = v[3 * atom + 2];
    dir[3 * atom] = K[0] * (vx * r.r00 + vy * r.r10 + vz * r.r20);
    dir[3 * atom + 1] = K[1] * (vy * r.r11 + vz * r.r21);
    dir[3 * atom + 2] = K[2] * (vz * r.r22);
}

// the two weights of one axis of a staged atom at point `g` (row: ORDER values of the first array, then ORDER of the second): every
// stencil slot i with (g0 + i) mod K == g, as axis_weight
template <int ORDER>
__device__ __forceinline__ void axis_weights2(int g, int g0, int K, const float* row, float& a, float& b) {
    int dd = g - g0;
    dd += dd < 0 ? K : 0;
    a = 0.f;
    b = 0.f;
    for (int i = dd; i < ORDER; i += K) { a += row[i]; b += row[ORDER + i]; }
}

// the spread of Q' as a gather: pme_recip_gather's walk over the bricks and sorted atoms the forward pass left in the workspace; per
// staged atom six axis arrays -- x: A = w theta + q s_x dtheta and q theta; y: theta and s_y dtheta; z: theta and s_z dtheta -- and
//     Q'(m) += A_x ty tz + (q tx) (Dy tz + ty Dz)
// The staged weights lie atom-major in LDS with an odd stride: a lane reads the one slot its point needs per array (lanes of a wave
// ask for at most ORDER neighbouring words: no bank conflict) instead of all ORDER slots and a select.  A wave's 64 points share
// their x: an atom whose x stencil misses it is skipped by the whole wave.
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_gather_dir(Dims d, const int* __restrict__ start, const int* __restrict__ sorted,
                                                               const int4* __restrict__ base, const float* __restrict__ theta,
                                                               const float* __restrict__ dtheta, const float* __restrict__ dir,
                                                               const float* __restrict__ charge, const float* __restrict__ wq,
                                                               float sqrt_coulomb, float* __restrict__ grid) {
    __shared__ int s_bx[kMaxBinsPerAxis], s_by[kMaxBinsPerAxis], s_bz[kMaxBinsPerAxis];
    __shared__ int s_first[kMaxBinsPerAxis * kMaxBinsPerAxis * kMaxBinsPerAxis];
    __shared__ int s_prefix[kMaxBinsPerAxis * kMaxBinsPerAxis * kMaxBinsPerAxis + 1];
    __shared__ int s_ntrip;
    __shared__ int s_base[3][kBlock];
    __shared__ float s_w[kBlock][6 * ORDER + 1];           // [slot][array * ORDER + i]: Ax, Qx, Ty, Dy, Tz, Dz (odd stride)
    __shared__ int s_n[3], s_count[kMaxBinsPerAxis * kMaxBinsPerAxis * kMaxBinsPerAxis];

    const int brick = blockIdx.x;
    const int bz = brick % d.nbz, by = (brick / d.nbz) % d.nby, bx = brick / (d.nbz * d.nby);
    if (threadIdx.x == 0) s_n[0] = window_bins(bx, kBX, d.kx, d.nbx, ORDER, s_bx);
    if (threadIdx.x == 64) s_n[1] = window_bins(by, kBY, d.ky, d.nby, ORDER, s_by);
    if (threadIdx.x == 128) s_n[2] = window_bins(bz, kBZ, d.kz, d.nbz, ORDER, s_bz);
    __syncthreads();
    const int nx = s_n[0], ny = s_n[1], nz = s_n[2];
    if ((int)threadIdx.x < nx * ny * nz) {                // window order: x outermost, z innermost
        const int i = threadIdx.x / (ny * nz), j = (threadIdx.x / nz) % ny, k = threadIdx.x % nz;
        const long long bin = ((long long)s_bx[i] * d.nby + s_by[j]) * d.nbz + s_bz[k];
        const int first = start[bin];
        s_first[threadIdx.x] = first;
        s_count[threadIdx.x] = start[bin + 1] - first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        const int t = nx * ny * nz;
        for (int u = 0; u < t; u++) { s_prefix[u] = total; total += s_count[u]; }
        s_prefix[t] = total;
        s_ntrip = t;
    }
    __syncthreads();
    const int ntrip = s_ntrip, total = s_prefix[ntrip];
    const int gx = bx * kBX + (threadIdx.x / (kBY * kBZ)), gy = by * kBY + (threadIdx.x / kBZ) % kBY, gz = bz * kBZ + threadIdx.x % kBZ;
    const bool live = gx < d.kx && gy < d.ky && gz < d.kz;
    float acc = 0.f;
    for (int c0 = 0; c0 < total; c0 += kBlock) {
        const int f = c0 + threadIdx.x;
        if (f < total) {
            int t = 0;
            while (s_prefix[t + 1] <= f) t++;
            const int atom = sorted[s_first[t] + (f - s_prefix[t])];
            const int4 b0 = base[atom];
            s_base[0][threadIdx.x] = b0.x; s_base[1][threadIdx.x] = b0.y; s_base[2][threadIdx.x] = b0.z;
            const float qs = charge[atom] * sqrt_coulomb, ws = wq[atom] * sqrt_coulomb;
            const float sx = dir[3 * atom], sy = dir[3 * atom + 1], sz = dir[3 * atom + 2];
            const float* th = theta + (size_t)atom * 3 * ORDER;
            const float* dth = dtheta + (size_t)atom * 3 * ORDER;
#pragma unroll
            for (int i = 0; i < ORDER; i++) {
                s_w[threadIdx.x][i] = ws * th[i] + qs * sx * dth[i];
                s_w[threadIdx.x][ORDER + i] = qs * th[i];
                s_w[threadIdx.x][2 * ORDER + i] = th[ORDER + i];
                s_w[threadIdx.x][3 * ORDER + i] = sy * dth[ORDER + i];
                s_w[threadIdx.x][4 * ORDER + i] = th[2 * ORDER + i];
                s_w[threadIdx.x][5 * ORDER + i] = sz * dth[2 * ORDER + i];
            }
        }
        __syncthreads();
        const int m = min(kBlock, total - c0);
        if (live) {
            for (int k = 0; k < m; k++) {
                int ddx = gx - s_base[0][k];
                ddx += ddx < 0 ? d.kx : 0;
                if (ddx >= ORDER) continue;                // (the x stencil misses this wave's points: adds exactly nothing)
                float ax, qx, ty, dy, tz, dz;
                axis_weights2<ORDER>(gx, s_base[0][k], d.kx, &s_w[k][0], ax, qx);
                axis_weights2<ORDER>(gy, s_base[1][k], d.ky, &s_w[k][2 * ORDER], ty, dy);
                axis_weights2<ORDER>(gz, s_base[2][k], d.kz, &s_w[k][4 * ORDER], tz, dz);
                acc += ax * ty * tz + qx * (dy * tz + ty * dz);
            }
        }
        __syncthreads();
    }
    if (live) grid[((size_t)gx * d.ky + gy) * d.kz + gz] = acc;
}

// one lane per atom over its order^3 stencil, both grids: the sums along z first, then the x / y weights
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_interp2(int num_atoms, Dims d, const float* __restrict__ box,
                                                            const float* __restrict__ charge, const float* __restrict__ wq,
                                                            float sqrt_coulomb, const int4* __restrict__ base,
                                                            const double* __restrict__ wide, const float* __restrict__ dir,
                                                            const float* __restrict__ phi, const float* __restrict__ phi2,
                                                            float* __restrict__ grad_pos, float* __restrict__ grad_charge) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= num_atoms) return;
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = box[i];
    const RecipBox r = recip_box(b);
    const int4 b0 = base[atom];
    const double* th = wide + (size_t)atom * 9 * ORDER;
    const double* dth = th + 3 * ORDER;
    const double* d2 = th + 6 * ORDER;
    double tz[ORDER], dz[ORDER], cz[ORDER];
    int iz[ORDER];
#pragma unroll
    for (int i = 0; i < ORDER; i++) {
        tz[i] = th[2 * ORDER + i]; dz[i] = dth[2 * ORDER + i]; cz[i] = d2[2 * ORDER + i];
        iz[i] = (b0.z + i) % d.kz;
    }
    // The sums run in double: d_a d_b W . phi differences the potential grid twice, and on a fine grid neighbouring values of phi nearly
    // cancel -- float sums left an error that grew with the square of the grid size.
    double hx = 0.0, hy = 0.0, hz = 0.0;                                      // d_a W . phi
    double hxx = 0.0, hyy = 0.0, hzz = 0.0, hxy = 0.0, hxz = 0.0, hyz = 0.0;  // d_a d_b W . phi
    double a2 = 0.0, g2x = 0.0, g2y = 0.0, g2z = 0.0;                         // W . phi', d_a W . phi'
#pragma unroll
    for (int a = 0; a < ORDER; a++) {
        const int xi = (b0.x + a) % d.kx;
        const double tx = th[a], dx = dth[a], cx = d2[a];
#pragma unroll
        for (int c = 0; c < ORDER; c++) {
            const size_t row = ((size_t)xi * d.ky + (b0.y + c) % d.ky) * d.kz;
            const double ty = th[ORDER + c], dy = dth[ORDER + c], cy = d2[ORDER + c];
            double z0 = 0.0, z1 = 0.0, z2 = 0.0, p0 = 0.0, p1 = 0.0;
#pragma unroll
            for (int e = 0; e < ORDER; e++) {
                const double g = phi[row + iz[e]], g2 = phi2[row + iz[e]];
                z0 += tz[e] * g; z1 += dz[e] * g; z2 += cz[e] * g;
                p0 += tz[e] * g2; p1 += dz[e] * g2;
            }
            const double txy = tx * ty, dxy = dx * ty, xdy = tx * dy;
            hx += dxy * z0; hy += xdy * z0; hz += txy * z1;
            hxx += cx * ty * z0; hyy += tx * cy * z0; hzz += txy * z2;
            hxy += dx * dy * z0; hxz += dxy * z1; hyz += xdy * z1;
            a2 += txy * p0; g2x += dxy * p0; g2y += xdy * p0; g2z += txy * p1;
        }
    }
    const double sx = dir[3 * atom], sy = dir[3 * atom + 1], sz = dir[3 * atom + 2];
    const double qs = (double)charge[atom] * sqrt_coulomb, ws = (double)wq[atom] * sqrt_coulomb;
    grad_charge[atom] = (float)(sqrt_coulomb * (a2 + sx * hx + sy * hy + sz * hz));
    const double fx = (qs * (g2x + sx * hxx + sy * hxy + sz * hxz) + ws * hx) * d.kx;
    const double fy = (qs * (g2y + sx * hxy + sy * hyy + sz * hyz) + ws * hy) * d.ky;
    const double fz = (qs * (g2z + sx * hxz + sy * hyz + sz * hzz) + ws * hz) * d.kz;
    grad_pos[3 * atom] = (float)(fx * r.r00);
    grad_pos[3 * atom + 1] = (float)(fx * r.r10 + fy * r.r11);
    grad_pos[3 * atom + 2] = (float)(fx * r.r20 + fy * r.r21 + fz * r.r22);
}

int check_common(int num_atoms, int gx, int gy, int gz, int order) {
    NNPOPS_REQUIRE(num_atoms >= 0, "bad number of atoms %d", num_atoms);
    NNPOPS_REQUIRE(gx >= 1 && gy >= 1 && gz >= 1, "the grid dimensions must be positive (%d, %d, %d)", gx, gy, gz);
    NNPOPS_REQUIRE((long long)gx * gy * gz <= 0x7fffffffll, "grid of %lld points is too large", (long long)gx * gy * gz);
    NNPOPS_REQUIRE(order == 4 || order == 5, "Only pmeOrder 4 or 5 is supported (got %d)", order);
    return NNPOPS_OK;
}

}  // namespace

extern "C" {

int64_t nnpops_pme_reciprocal_workspace_bytes(int num_atoms, int gridx, int gridy, int gridz, int order) {
    if (check_common(num_atoms, gridx, gridy, gridz, order) != NNPOPS_OK) return 0;
    return (int64_t)carve(nullptr, num_atoms, gridx, gridy, gridz, order).bytes;
}

int nnpops_pme_reciprocal_spread(int num_atoms, int gridx, int gridy, int gridz, int order, const float* positions, const float* charges,
                                 const float* box_vectors, float coulomb, float* real_grid, void* workspace, void* stream) {
    if (int rc = check_common(num_atoms, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0, "coulomb must be positive");
    NNPOPS_REQUIRE(box_vectors && real_grid && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && charges), "NULL positions / charges pointer");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const RecipWorkspace w = carve(workspace, num_atoms, gridx, gridy, gridz, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    NNPOPS_HIP_TRY(hipMemsetAsync(w.bin_count, 0, sizeof(int) * (size_t)d.nbins, s));
    if (num_atoms > 0) {
        if (order == 4)
            hipLaunchKernelGGL(pme_recip_spline<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, positions, box_vectors, d, w.base, w.theta,
                               w.dtheta, w.bin_count);
        else
            hipLaunchKernelGGL(pme_recip_spline<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, positions, box_vectors, d, w.base, w.theta,
                               w.dtheta, w.bin_count);
    }
    hipLaunchKernelGGL(pme_recip_scan, dim3(1), dim3(1024), 0, s, d.nbins, (const int*)w.bin_count, w.bin_start, w.cursor);
    if (num_atoms > 0) {
        hipLaunchKernelGGL(pme_recip_scatter, dim3(ab), dim3(kBlock), 0, s, num_atoms, (const int4*)w.base, w.cursor, w.unsorted);
        const int ob = (int)std::min<long long>((d.nbins + kBlock / 64 - 1) / (kBlock / 64), 16384);
        hipLaunchKernelGGL(pme_recip_order, dim3(ob), dim3(kBlock), 0, s, d.nbins, (const int*)w.bin_start, (const int*)w.unsorted, w.sorted);
    }
    if (order == 4)
        hipLaunchKernelGGL(pme_recip_gather<4>, dim3((unsigned)d.nbins), dim3(kBlock), 0, s, d, (const int*)w.bin_start, (const int*)w.sorted,
                           (const int4*)w.base, (const float*)w.theta, charges, sqrt_coulomb, real_grid);
    else
        hipLaunchKernelGGL(pme_recip_gather<5>, dim3((unsigned)d.nbins), dim3(kBlock), 0, s, d, (const int*)w.bin_start, (const int*)w.sorted,
                           (const int4*)w.base, (const float*)w.theta, charges, sqrt_coulomb, real_grid);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_convolve(int num_atoms, int gridx, int gridy, int gridz, int order, const float* box_vectors, float alpha,
                                   const float* xmoduli, const float* ymoduli, const float* zmoduli, void* recip_grid, float* energy,
                                   void* workspace, void* stream) {
    if (int rc = check_common(num_atoms, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(alpha > 0, "alpha must be positive");
    NNPOPS_REQUIRE(box_vectors && xmoduli && ymoduli && zmoduli && recip_grid && energy && workspace, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const RecipWorkspace w = carve(workspace, num_atoms, gridx, gridy, gridz, order);
    const int cb = conv_blocks(gridx, gridy, gridz);
    const float recip_exp_factor = (float)(M_PI * M_PI / ((double)alpha * (double)alpha));
    hipLaunchKernelGGL(pme_recip_convolve, dim3(cb), dim3(kBlock), 0, s, gridx, gridy, gridz, box_vectors, recip_exp_factor, xmoduli,
                       ymoduli, zmoduli, (float2*)recip_grid, w.partial);
    hipLaunchKernelGGL(pme_recip_energy, dim3(1), dim3(kConvBlocksMax), 0, s, (const double*)w.partial, cb, energy);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int64_t nnpops_pme_reciprocal_box_workspace_bytes(int num_atoms, int gridx, int gridy, int gridz, int order) {
    if (check_common(num_atoms, gridx, gridy, gridz, order) != NNPOPS_OK) return 0;
    return (int64_t)box_carve(nullptr, num_atoms, gridx, gridy, gridz).bytes;
}

int nnpops_pme_reciprocal_convolve_box(int num_atoms, int gridx, int gridy, int gridz, int order, const float* box_vectors, float alpha,
                                       const float* xmoduli, const float* ymoduli, const float* zmoduli, void* recip_grid, float* energy,
                                       void* workspace, void* box_workspace, void* stream) {
    if (int rc = check_common(num_atoms, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(alpha > 0, "alpha must be positive");
    NNPOPS_REQUIRE(box_vectors && xmoduli && ymoduli && zmoduli && recip_grid && energy && workspace && box_workspace, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const RecipWorkspace w = carve(workspace, num_atoms, gridx, gridy, gridz, order);
    const BoxWorkspace bw = box_carve(box_workspace, num_atoms, gridx, gridy, gridz);
    const int cb = conv_blocks(gridx, gridy, gridz);
    const float recip_exp_factor = (float)(M_PI * M_PI / ((double)alpha * (double)alpha));
    hipLaunchKernelGGL(pme_recip_convolve, dim3(cb), dim3(kBlock), 0, s, gridx, gridy, gridz, box_vectors, recip_exp_factor, xmoduli,
                       ymoduli, zmoduli, (float2*)recip_grid, w.partial);
    hipLaunchKernelGGL(pme_recip_energy, dim3(1), dim3(kConvBlocksMax), 0, s, (const double*)w.partial, cb, energy);
    hipLaunchKernelGGL(pme_recip_box_pi, dim3(cb), dim3(kBlock), 0, s, gridx, gridy, gridz, box_vectors, recip_exp_factor, xmoduli, ymoduli,
                       zmoduli, (const float2*)recip_grid, bw.pi_partial);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_box_gradient(int num_atoms, int gridx, int gridy, int gridz, int order, const float* positions,
                                       const float* box_vectors, const float* position_deriv, float* grad_box, void* box_workspace,
                                       void* stream) {
    if (int rc = check_common(num_atoms, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(box_vectors && grad_box && box_workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && position_deriv), "NULL positions / derivative pointer");
    hipStream_t s = (hipStream_t)stream;
    const BoxWorkspace bw = box_carve(box_workspace, num_atoms, gridx, gridy, gridz);
    const int ab = div_up(num_atoms, kBlock);
    if (num_atoms > 0)
        hipLaunchKernelGGL(pme_recip_box_atoms, dim3(ab), dim3(kBlock), 0, s, num_atoms, positions, position_deriv, bw.x_partial);
    hipLaunchKernelGGL(pme_recip_box_finish, dim3(1), dim3(kBlock), 0, s, conv_blocks(gridx, gridy, gridz), (const double*)bw.pi_partial, ab,
                       (const double*)bw.x_partial, box_vectors, grad_box);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_interpolate(int num_atoms, int gridx, int gridy, int gridz, int order, const float* charges,
                                      const float* box_vectors, float coulomb, const float* real_grid, float* position_deriv,
                                      float* charge_deriv, void* workspace, void* stream) {
    if (int rc = check_common(num_atoms, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0, "coulomb must be positive");
    NNPOPS_REQUIRE(box_vectors && real_grid && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (charges && position_deriv && charge_deriv), "NULL charges / derivative pointer");
    if (num_atoms == 0) return NNPOPS_OK;
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const RecipWorkspace w = carve(workspace, num_atoms, gridx, gridy, gridz, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    if (order == 4)
        hipLaunchKernelGGL(pme_recip_interp<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, d, box_vectors, charges, sqrt_coulomb,
                           (const int4*)w.base, (const float*)w.theta, (const float*)w.dtheta, real_grid, position_deriv, charge_deriv);
    else
        hipLaunchKernelGGL(pme_recip_interp<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, d, box_vectors, charges, sqrt_coulomb,
                           (const int4*)w.base, (const float*)w.theta, (const float*)w.dtheta, real_grid, position_deriv, charge_deriv);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int64_t nnpops_pme_reciprocal_second_workspace_bytes(int num_atoms, int gridx, int gridy, int gridz, int order) {
    if (check_common(num_atoms, gridx, gridy, gridz, order) != NNPOPS_OK) return 0;
    return (int64_t)second_carve(nullptr, num_atoms, order).bytes;
}

int nnpops_pme_reciprocal_spread_directional(int num_atoms, int gridx, int gridy, int gridz, int order, const float* positions,
                                             const float* charges, const float* box_vectors, float coulomb, const float* v, const float* w,
                                             float* real_grid, void* workspace, void* second_workspace, void* stream) {
    if (int rc = check_common(num_atoms, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0, "coulomb must be positive");
    NNPOPS_REQUIRE(box_vectors && real_grid && workspace && second_workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && charges && v && w), "NULL positions / charges / cotangent pointer");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const RecipWorkspace ws = carve(workspace, num_atoms, gridx, gridy, gridz, order);
    const SecondWorkspace w2 = second_carve(second_workspace, num_atoms, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    if (order == 4) {
        if (num_atoms > 0)
            hipLaunchKernelGGL(pme_recip_spline2<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, positions, box_vectors, d, (const int4*)ws.base, v,
                               w2.wide, w2.dir);
        hipLaunchKernelGGL(pme_recip_gather_dir<4>, dim3((unsigned)d.nbins), dim3(kBlock), 0, s, d, (const int*)ws.bin_start,
                           (const int*)ws.sorted, (const int4*)ws.base, (const float*)ws.theta, (const float*)ws.dtheta,
                           (const float*)w2.dir, charges, w, sqrt_coulomb, real_grid);
    } else {
        if (num_atoms > 0)
            hipLaunchKernelGGL(pme_recip_spline2<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, positions, box_vectors, d, (const int4*)ws.base, v,
                               w2.wide, w2.dir);
        hipLaunchKernelGGL(pme_recip_gather_dir<5>, dim3((unsigned)d.nbins), dim3(kBlock), 0, s, d, (const int*)ws.bin_start,
                           (const int*)ws.sorted, (const int4*)ws.base, (const float*)ws.theta, (const float*)ws.dtheta,
                           (const float*)w2.dir, charges, w, sqrt_coulomb, real_grid);
    }
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_interpolate_second(int num_atoms, int gridx, int gridy, int gridz, int order, const float* charges,
                                             const float* box_vectors, float coulomb, const float* w, const float* potential_grid,
                                             const float* directional_grid, float* grad_positions, float* grad_charges, void* workspace,
                                             void* second_workspace, void* stream) {
    if (int rc = check_common(num_atoms, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0, "coulomb must be positive");
    NNPOPS_REQUIRE(box_vectors && potential_grid && directional_grid && workspace && second_workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (charges && w && grad_positions && grad_charges), "NULL charges / cotangent / gradient pointer");
    if (num_atoms == 0) return NNPOPS_OK;
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const RecipWorkspace ws = carve(workspace, num_atoms, gridx, gridy, gridz, order);
    const SecondWorkspace w2 = second_carve(second_workspace, num_atoms, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    if (order == 4)
        hipLaunchKernelGGL(pme_recip_interp2<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, d, box_vectors, charges, w, sqrt_coulomb,
                           (const int4*)ws.base, (const double*)w2.wide,
                           (const float*)w2.dir, potential_grid, directional_grid, grad_positions, grad_charges);
    else
        hipLaunchKernelGGL(pme_recip_interp2<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, d, box_vectors, charges, w, sqrt_coulomb,
                           (const int4*)ws.base, (const double*)w2.wide,
                           (const float*)w2.dir, potential_grid, directional_grid, grad_positions, grad_charges);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // extern "C"
