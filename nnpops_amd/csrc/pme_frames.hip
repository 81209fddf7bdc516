// pme_frames.hip -- both PME terms for a BATCH OF FRAMES, every frame in its own box: per-frame energies [B] and the derivatives with
// respect to positions and charges, in a handful of launches for the whole minibatch.  The single-system kernels
// (pme.hip, pme_recip.hip) are shaped for one large system -- a streamed pair list, a brick sort in front of the spread.  A frame of
// tens to a few hundred atoms fits in LDS whole, which allows a shorter design:
//
//   pme_direct_frames          the direct term WITHOUT a pair list.  The host table cuts every frame into tiles of 16 owner atoms; one
//                              workgroup takes a tile, 16 lanes per owner.  The frame's positions and charges are staged in LDS (up to
//                              kFrameLdsAtoms atoms, global reads beyond); owner i's lanes walk the frame's atoms j = sub, sub + 16, ...
//                              and form the displacement of the pair (max(i, j), min(i, j)) exactly as getNeighborPairsFrames does
//                              (pair_delta.h), keep it when !(d^2 > cutoff^2), skip it when j is in the owner's (descending) exclusion
//                              row, and add the terms of pme_direct_pairs; then the owner's lanes walk its exclusion row for the
//                              un-wrapped erf correction, as pme_direct_gather does.  Every pair is evaluated twice, once by each
//                              owner, from the same float values: no atomics, no incoming rows, no quantised sums, and Newton's third
//                              law holds to the bit.  float32 sums per lane in a fixed order, the 16 lanes combined in the fixed xor
//                              order; the energy (included pairs from the higher index, excluded pairs from the lower) in double per
//                              lane, then one double per tile.
//   pme_frames_energy          one wave per frame: the frame's partial sums (its tiles, or its convolution workgroups) in a fixed order.
//   pme_recip_spline_frames    one lane per atom: base index and B-spline weights in the atom's own frame's box (spline_atom).
//   pme_recip_spread_frames    the spread as a gather with NO SORT in front of it: one workgroup per (frame, brick of 4 x 4 x 16 grid
//                              points), one lane per point.  The workgroup walks the frame's atoms 256 at a time in ascending index; a
//                              lane keeps its atom when the atom's cyclic stencil meets the brick on all three axes; ballot ranks plus
//                              the four waves' counts give the kept atoms consecutive LDS slots in ascending atom order, and whenever
//                              the slots cannot take another round (or the frame is exhausted) every lane adds what reaches its point,
//                              in slot order.  The order of a point's sum is the atoms' order, whatever the timing; every point of
//                              every frame is written exactly once, so the grids need no clearing.
//   pme_recip_convolve_frames  one lane per complex point of a frame's grid, the frame's box in scalar registers; energy in double per
//                              (frame, workgroup).
//   pme_recip_interp_frames    one lane per atom: the order^3 gather from its own frame's slab of the potential grid.
// The box gradient dE_m/dB_m of both terms (DESIGN.md s8c for the formulae), in passes of their own so that the kernels above keep their bits:
//   pme_direct_frames_box      the tiles of pme_direct_frames, every pair once from its higher index: the shift n_k first (box_grad.h),
//                              pairs with n_k = 0 stop there; nine float64 sums per tile.  pme_frames_box_sum: one wave per frame.
//   pme_recip_box_pi_frames    after the convolution: Pi in float64 per (frame, workgroup) from the scaled grids.
//   pme_recip_box_finish_frames one workgroup per frame: the Pi partials, X = sum_j x_j (x) g_j over the frame's atoms, - B^-T (Pi / 2 + X).
//
// The table (nnpops_pme_frames_table, int32): {B, N, T, 0} | offsets [B + 1] | tile_start [B + 1] | tiles [T][4] = {frame, first atom of
// the frame, atoms of the frame, first owner} | atom_frame [N].  A frame's tiles are consecutive.  The kernels clamp whatever a table
// holds: nothing outside [0, N) atoms or [0, B) boxes is ever read or written.
// The boxes are read on the device by every pass: a captured graph follows new positions and boxes written in place.
// This unit is compiled without packed float32 arithmetic (build.py).
#include <cmath>
#include <limits>

#include "box_grad.h"
#include "device_common.h"
#include "host_common.h"
#include "pair_delta.h"
#include "pme_recip_common.h"

using namespace nnpops;

namespace {

constexpr int kBlock = 256;
constexpr int kTileOwners = NNPOPS_PME_FRAMES_TILE;    // owner atoms per workgroup, 16 lanes each
constexpr int kFrameLdsAtoms = 1024;                   // 16 KiB of LDS per workgroup: several workgroups still share a CU
constexpr int kBX = 4, kBY = 4, kBZ = 16;              // brick of grid points = one spread workgroup
constexpr int kConvBlocksMax = 1024;
constexpr float kTwoOverSqrtPi = 1.12837916709551257390f;
static_assert(kTileOwners * 16 == kBlock && kBX * kBY * kBZ == kBlock, "one lane per (owner, sub) and per grid point of a brick");
static_assert(kBoxThreads == kBlock, "box_block_sum9 adds up a workgroup of kBlock lanes");

struct TableView {
    const int32_t *offsets, *tile_start, *tiles, *atom_frame;
};
__host__ __device__ inline TableView view(const int32_t* table, int B, int T) {
    TableView v;
    v.offsets = table + 4;
    v.tile_start = v.offsets + (B + 1);
    v.tiles = v.tile_start + (B + 1);
    v.atom_frame = v.tiles + 4 * (size_t)T;
    return v;
}

struct Tile { int frame, first, n, owner0; };
__device__ __forceinline__ Tile load_tile(const int32_t* __restrict__ tiles, int tile, int N, int B) {
    const int32_t* r = tiles + 4 * (size_t)tile;                            // (uniform address: scalar loads)
    Tile t;
    t.frame = min(max(r[0], 0), max(B - 1, 0));
    t.first = min(max(r[1], 0), N);
    t.n = min(max(r[2], 0), N - t.first);
    t.owner0 = min(max(r[3], t.first), t.first + t.n);
    return t;
}

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the workgroup's energy: lanes of a wave in the xor order, then the four waves in wave order
__device__ __forceinline__ void block_energy(double energy, double* red, double* __restrict__ out) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) energy += __shfl_xor(energy, off, 64);
    if (lane_id() == 0) red[threadIdx.x >> 6] = energy;
    __syncthreads();
    if (threadIdx.x == 0) {
        double e = 0.0;
        for (int w = 0; w < kBlock / 64; w++) e += red[w];
        *out = e;
    }
}

__global__ __launch_bounds__(kBlock) void pme_direct_frames(int N, int B, int max_excl, const int32_t* __restrict__ tiles,
                                                             const float* __restrict__ pos, const float* __restrict__ charge,
                                                             const int* __restrict__ excl, const float* __restrict__ boxes, float cutoff2,
                                                             float alpha, float coulomb, float* __restrict__ pos_deriv,
                                                             float* __restrict__ charge_deriv, double* __restrict__ tile_energy) {
    __shared__ float spos[3 * kFrameLdsAtoms];
    __shared__ float sq[kFrameLdsAtoms];
    __shared__ double red[kBlock / 64];
    const Tile t = load_tile(tiles, blockIdx.x, N, B);
    const float* box = boxes + 9 * (size_t)t.frame;
    const float* fpos = pos + 3 * (size_t)t.first;
    const float* fq = charge + t.first;
    const bool staged = t.n <= kFrameLdsAtoms;
    if (staged) {
        for (int k = threadIdx.x; k < 3 * t.n; k += kBlock) spos[k] = fpos[k];
        for (int k = threadIdx.x; k < t.n; k += kBlock) sq[k] = fq[k];
    }
    __syncthreads();
    const int sub = threadIdx.x & 15;
    const int i = t.owner0 - t.first + (threadIdx.x >> 4);                  // the owner, counted inside its frame
    const bool live = i < t.n;
    const int gi = t.first + i;
    float ax = 0.f, ay = 0.f, az = 0.f, aq = 0.f;
    double energy = 0.0;
    auto walk = [&](const float* __restrict__ P, const float* __restrict__ Q) {
        const float qi = Q[i];
        const int* row = excl + (size_t)gi * max_excl;
        for (int j = sub; j < t.n; j += 16) {
            if (j == i) continue;
            const bool upper = i > j;                                        // the pair is (max, min), as the pair list has it
            const Vec3<float> d = wrapped_delta<float>(P, upper ? i : j, upper ? j : i, box, true);
            const float d2 = allpairs_norm2<float>(d);
            if (d2 > cutoff2) continue;                                      // kept when !(d2 > cutoff2), as getNeighborPairsFrames keeps it
            const int gj = t.first + j;
            bool include = true;
            for (int e = 0; e < max_excl; e++) {                             // rows are sorted in descending order (pme.py)
                const int x = row[e];
                if (x < gj) break;
                if (x == gj) { include = false; break; }
            }
            if (!include) continue;
            // the float expressions of pme_direct_pairs: c1 is the charge of the higher index for both owners
            const float r = sqrtf(d2);
            const float inv_r = 1.0f / r, ar = alpha * r;
            const float ex = expf(-ar * ar), erfc_ar = erfcf(ar);
            const float pre = coulomb * inv_r;
            const float qj = Q[j];
            const float c1 = upper ? qi : qj, c2 = upper ? qj : qi;
            if (upper) energy += (double)(pre * erfc_ar * c1 * c2);
            const float dedr = pre * c1 * c2 * (erfc_ar + ar * ex * kTwoOverSqrtPi) * inv_r * inv_r;
            const float fx = dedr * d.x, fy = dedr * d.y, fz = dedr * d.z;  // the force on the lower index; the higher takes its negative
            ax += upper ? -fx : fx; ay += upper ? -fy : fy; az += upper ? -fz : fz;
            aq += pre * erfc_ar * qj;
        }
        // excluded pairs of this owner: the erf() part reciprocal space cannot leave out, un-wrapped (as pme_direct_gather)
        const float px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
        for (int e = sub; e < max_excl; e += 16) {
            const int other = row[e];
            const int o = other - t.first;
            if (other == gi || (unsigned)o >= (unsigned)t.n) continue;      // (-1 padding; a partner outside the frame is never read)
            const float dx = px - P[3 * o], dy = py - P[3 * o + 1], dz = pz - P[3 * o + 2];
            const float r = sqrtf(dx * dx + dy * dy + dz * dz);
            const float inv_r = 1.0f / r, ar = alpha * r;
            const float ex = expf(-ar * ar), erf_ar = erff(ar);
            const float pre = coulomb * inv_r;
            const float c2 = Q[o];
            if (other > gi) energy -= (double)(pre * erf_ar * qi * c2);     // once per pair
            const float dedr = pre * qi * c2 * (erf_ar - ar * ex * kTwoOverSqrtPi) * inv_r * inv_r;
            ax += dedr * dx; ay += dedr * dy; az += dedr * dz;
            aq -= pre * erf_ar * c2;
        }
    };
    if (live) {
        if (staged) walk(spos, sq); else walk(fpos, fq);
    }
    ax = group16_sum(ax); ay = group16_sum(ay); az = group16_sum(az); aq = group16_sum(aq);
    if (live && sub == 0) {
        pos_deriv[3 * (size_t)gi] = ax; pos_deriv[3 * (size_t)gi + 1] = ay; pos_deriv[3 * (size_t)gi + 2] = az;
        charge_deriv[gi] = aq;
    }
    block_energy(energy, red, tile_energy + blockIdx.x);
}

// energy[m] = scale x the partial sums of frame m: [starts[m], starts[m + 1]) when `starts` is given, `per` consecutive ones otherwise.
// One wave per frame, lane l adds l, l + 64, ..., then the xor order: a frame's energy does not depend on the batch around it.
__global__ __launch_bounds__(64) void pme_frames_energy(const int32_t* __restrict__ starts, int per, int total, const double* __restrict__ partial,
                                                        double scale, float* __restrict__ energy) {
    const int m = blockIdx.x;
    const long long b0 = starts ? starts[m] : (long long)m * per, e0 = starts ? starts[m + 1] : b0 + per;
    const int begin = (int)min(max(b0, 0ll), (long long)total), end = (int)min(max(e0, (long long)begin), (long long)total);
    double e = 0.0;
    for (int q = begin + (int)threadIdx.x; q < end; q += 64) e += partial[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off, 64);
    if (threadIdx.x == 0) energy[m] = (float)(scale * e);
}

// ---- box gradient of the direct term: dE_m/dB_m = - sum_k n_k (x) G_k = sum_k n_k (x) (dedr_k delta_k) over frame m's included pairs ----
// A pass of its own (pme_direct_frames keeps its bits): the same tiles, staging, displacement, keep rule, exclusion test and float
// expressions for dedr, but owner i's lanes walk j = sub, sub + 16, ... < i only -- every pair ONCE, from its higher index, the side the
// forward counts the energy from.  The shift n_k is recovered (box_grad.h: image_shift) before anything else: a pair with n_k = 0 adds
// exactly nothing and skips the exclusion scan, the charges and the transcendentals.  Nine float64 sums per lane, box_block_sum9 per
// tile.  The excluded pairs' erf correction is un-wrapped: it does not depend on the box.
__global__ __launch_bounds__(kBlock) void pme_direct_frames_box(int N, int B, int max_excl, const int32_t* __restrict__ tiles,
                                                                 const float* __restrict__ pos, const float* __restrict__ charge,
                                                                 const int* __restrict__ excl, const float* __restrict__ boxes, float cutoff2,
                                                                 float alpha, float coulomb, double* __restrict__ tile_box) {
    __shared__ float spos[3 * kFrameLdsAtoms];
    __shared__ float sq[kFrameLdsAtoms];
    const Tile t = load_tile(tiles, blockIdx.x, N, B);
    const float* box = boxes + 9 * (size_t)t.frame;                         // (uniform address: scalar loads)
    const float* fpos = pos + 3 * (size_t)t.first;
    const float* fq = charge + t.first;
    const bool staged = t.n <= kFrameLdsAtoms;
    if (staged) {
        for (int k = threadIdx.x; k < 3 * t.n; k += kBlock) spos[k] = fpos[k];
        for (int k = threadIdx.x; k < t.n; k += kBlock) sq[k] = fq[k];
    }
    __syncthreads();
    const int sub = threadIdx.x & 15;
    const int i = t.owner0 - t.first + (threadIdx.x >> 4);                  // the owner, counted inside its frame
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    auto walk = [&](const float* __restrict__ P, const float* __restrict__ Q) {
        const int* row = excl + (size_t)(t.first + i) * max_excl;
        for (int j = sub; j < i; j += 16) {
            const Vec3<float> d = wrapped_delta<float>(P, i, j, box, true);
            const float d2 = allpairs_norm2<float>(d);
            if (d2 > cutoff2) continue;
            float n[3];
            image_shift(P, i, j, d.x, d.y, d.z, box, n);
            if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) continue;
            const int gj = t.first + j;
            bool include = true;
            for (int e = 0; e < max_excl; e++) {                             // rows are sorted in descending order (pme.py)
                const int x = row[e];
                if (x < gj) break;
                if (x == gj) { include = false; break; }
            }
            if (!include) continue;
            const float r = sqrtf(d2);
            const float inv_r = 1.0f / r, ar = alpha * r;
            const float ex = expf(-ar * ar), erfc_ar = erfcf(ar);
            const float pre = coulomb * inv_r;
            const float c1 = Q[i], c2 = Q[j];
            const float dedr = pre * c1 * c2 * (erfc_ar + ar * ex * kTwoOverSqrtPi) * inv_r * inv_r;
            const float f[3] = {dedr * d.x, dedr * d.y, dedr * d.z};         // -G_k
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int q = 0; q < 3; q++) acc[3 * a + q] += (double)n[a] * (double)f[q];
        }
    };
    if (i < t.n) {
        if (staged) walk(spos, sq); else walk(fpos, fq);
    }
    box_block_sum9(acc, tile_box + 9 * (size_t)blockIdx.x);
}

// box_deriv[m] = the nine sums of frame m's tiles [tile_start[m], tile_start[m + 1]): one wave per frame, lane l adds tiles l, l + 64, ...
// then the xor order.  A frame without tiles or without a shifted pair gets exact zeros; the order does not depend on the batch.
__global__ __launch_bounds__(64) void pme_frames_box_sum(const int32_t* __restrict__ tile_start, int T, const double* __restrict__ tile_box,
                                                         float* __restrict__ box_deriv) {
    const int m = blockIdx.x;
    const int begin = min(max(tile_start[m], 0), T), end = min(max(tile_start[m + 1], begin), T);
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    for (int k = begin + (int)threadIdx.x; k < end; k += 64) {
#pragma unroll
        for (int q = 0; q < 9; q++) acc[q] += tile_box[9 * (size_t)k + q];
    }
#pragma unroll
    for (int q = 0; q < 9; q++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
        if (threadIdx.x == q) box_deriv[9 * (size_t)m + q] = (float)acc[q];
    }
}

// ---- reciprocal space ----
struct Dims {
    int kx, ky, kz;          // grid
    int nbx, nby, nbz;       // bricks per axis
    int nbins;               // bricks per frame
};

Dims make_dims(int gx, int gy, int gz) {
    Dims d{gx, gy, gz, div_up(gx, kBX), div_up(gy, kBY), div_up(gz, kBZ), 0};
    d.nbins = d.nbx * d.nby * d.nbz;
    return d;
}

int conv_blocks(int gx, int gy, int gz) {
    const long long points = (long long)gx * gy * (gz / 2 + 1);
    return (int)std::min<long long>(std::max<long long>(1, (points + kBlock - 1) / kBlock), kConvBlocksMax);
}

struct RecipWorkspace {
    double* partial;      // [B][conv_blocks]
    int4* base;           // [N]            base grid index (x, y, z) and the atom's frame
    float* theta;         // [N][3][order]  B-spline weights
    float* dtheta;        // [N][3][order]  their derivatives
    size_t bytes;
};

RecipWorkspace carve(void* workspace, int num_atoms, int num_frames, int gx, int gy, int gz, int order) {
    RecipWorkspace w{};
    uintptr_t p = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    auto take = [&](size_t bytes) { const uintptr_t at = p; p += (bytes + 255) & ~(size_t)255; return at; };
    const size_t n = (size_t)num_atoms;
    w.partial = (double*)take(sizeof(double) * (size_t)num_frames * conv_blocks(gx, gy, gz));
    w.base = (int4*)take(sizeof(int4) * n);
    w.theta = (float*)take(sizeof(float) * 3 * (size_t)order * n);
    w.dtheta = (float*)take(sizeof(float) * 3 * (size_t)order * n);
    w.bytes = (size_t)(p - (uintptr_t)workspace) + 256;
    return w;
}

template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_spline_frames(int N, int B, const int32_t* __restrict__ atom_frame, const float* __restrict__ pos,
                                                                  const float* __restrict__ boxes, Dims d, int4* __restrict__ base,
                                                                  float* __restrict__ theta, float* __restrict__ dtheta) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= N) return;
    const int frame = min(max(atom_frame[atom], 0), B - 1);
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = boxes[9 * (size_t)frame + i];
    const RecipBox r = recip_box(b);
    const int K[3] = {d.kx, d.ky, d.kz};
    int gi[3];
    spline_atom<ORDER>(pos, atom, b, r, K, gi, theta + (size_t)atom * 3 * ORDER, dtheta + (size_t)atom * 3 * ORDER);
    base[atom] = make_int4(gi[0], gi[1], gi[2], frame);
}

// does the cyclic stencil [g0, g0 + ORDER - 1] mod K meet the points [lo, hi] of a brick?  Two cyclic intervals meet when the start of
// one lies in the other; a stencil as long as the axis (folded or not) meets everything, as window_bins / axis_weight treat it.
template <int ORDER>
__device__ __forceinline__ bool stencil_meets(int g0, int lo, int hi, int K) {
    if (ORDER >= K) return true;
    int ahead = lo - g0, behind = g0 - lo;
    ahead += ahead < 0 ? K : 0;
    behind += behind < 0 ? K : 0;
    return ahead < ORDER || behind <= hi - lo;
}

template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_spread_frames(int N, int B, const int32_t* __restrict__ offsets, Dims d,
                                                                  const int4* __restrict__ base, const float* __restrict__ theta,
                                                                  const float* __restrict__ charge, float sqrt_coulomb,
                                                                  float* __restrict__ grids) {
    __shared__ int s_base[3][kBlock];
    __shared__ float s_th[3 * ORDER][kBlock];              // [axis * ORDER + i][slot]: x weights carry q sqrt(coulomb)
    __shared__ int s_kept[kBlock / 64];
    const int frame = blockIdx.x / d.nbins, brick = blockIdx.x % d.nbins;   // (the host launches exactly B * nbins workgroups)
    const int bz = brick % d.nbz, by = (brick / d.nbz) % d.nby, bx = brick / (d.nbz * d.nby);
    const int a0 = min(max(offsets[frame], 0), N), a1 = min(max(offsets[frame + 1], a0), N);
    const int x_lo = bx * kBX, x_hi = min(x_lo + kBX, d.kx) - 1, y_lo = by * kBY, y_hi = min(y_lo + kBY, d.ky) - 1,
              z_lo = bz * kBZ, z_hi = min(z_lo + kBZ, d.kz) - 1;
    const int gx = x_lo + (threadIdx.x / (kBY * kBZ)), gy = y_lo + (threadIdx.x / kBZ) % kBY, gz = z_lo + threadIdx.x % kBZ;
    const bool live = gx < d.kx && gy < d.ky && gz < d.kz;
    const int wave = threadIdx.x >> 6;
    float acc = 0.f;
    int filled = 0;
    auto add_slots = [&](int m) {                          // every lane adds what reaches its point, in slot order
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
    };
    for (int c0 = a0; c0 < a1; c0 += kBlock) {
        const int atom = c0 + threadIdx.x;
        int4 b0 = make_int4(0, 0, 0, 0);
        bool keep = false;
        if (atom < a1) {
            b0 = base[atom];
            keep = stencil_meets<ORDER>(b0.x, x_lo, x_hi, d.kx) && stencil_meets<ORDER>(b0.y, y_lo, y_hi, d.ky) &&
                   stencil_meets<ORDER>(b0.z, z_lo, z_hi, d.kz);
        }
        const unsigned long long mask = __ballot(keep);
        if (lane_id() == 0) s_kept[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, round = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) {
            const int c = s_kept[w];
            before += w < wave ? c : 0;
            round += c;
        }
        if (filled + round > kBlock) {                     // (uniform) the slots cannot take this round: add what they hold first
            add_slots(filled);
            filled = 0;
            __syncthreads();
        }
        if (keep) {
            const int slot = filled + before + prefix_popc(mask);
            s_base[0][slot] = b0.x; s_base[1][slot] = b0.y; s_base[2][slot] = b0.z;
            const float qs = charge[atom] * sqrt_coulomb;
            const float* th = theta + (size_t)atom * 3 * ORDER;
#pragma unroll
            for (int i = 0; i < ORDER; i++) s_th[i][slot] = qs * th[i];
#pragma unroll
            for (int i = ORDER; i < 3 * ORDER; i++) s_th[i][slot] = th[i];
        }
        filled += round;
        __syncthreads();                                   // (the slots are complete; s_kept may be rewritten)
    }
    add_slots(filled);
    if (live) grids[(((size_t)frame * d.kx + gx) * d.ky + gy) * d.kz + gz] = acc;
}

// the float expressions of pme_recip_convolve with the frame's own box
__global__ __launch_bounds__(kBlock) void pme_recip_convolve_frames(int gx, int gy, int gz, int cb, const float* __restrict__ boxes,
                                                                   float recip_exp_factor, const float* __restrict__ xmod,
                                                                   const float* __restrict__ ymod, const float* __restrict__ zmod,
                                                                   float2* __restrict__ cgrids, double* __restrict__ partial) {
    __shared__ double red[kBlock / 64];
    const int frame = blockIdx.x / cb, blk = blockIdx.x % cb;               // (the host launches exactly B * cb workgroups)
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = boxes[9 * (size_t)frame + i];        // (uniform: scalar loads)
    const RecipBox r = recip_box(b);
    const float scale_factor = (float)M_PI * b[0] * b[4] * b[8];
    const int zsize = gz / 2 + 1;
    const long long points = (long long)gx * gy * zsize;
    float2* cgrid = cgrids + (size_t)frame * points;
    double energy = 0.0;
    for (long long idx = (long long)blk * kBlock + threadIdx.x; idx < points; idx += (long long)cb * kBlock) {
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
    block_energy(energy, red, partial + blockIdx.x);
}

// the expressions of pme_recip_interp, from the atom's own frame's slab of the potential grids
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_interp_frames(int N, int B, Dims d, const float* __restrict__ boxes,
                                                                  const float* __restrict__ charge, float sqrt_coulomb,
                                                                  const int4* __restrict__ base, const float* __restrict__ theta,
                                                                  const float* __restrict__ dtheta, const float* __restrict__ grids,
                                                                  float* __restrict__ pos_deriv, float* __restrict__ charge_deriv) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= N) return;
    const int4 b0 = base[atom];
    const int frame = min(max(b0.w, 0), B - 1);
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = boxes[9 * (size_t)frame + i];
    const RecipBox r = recip_box(b);
    const float* grid = grids + (size_t)frame * d.kx * d.ky * d.kz;
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
    pos_deriv[3 * (size_t)atom] = s * (fx * r.r00);
    pos_deriv[3 * (size_t)atom + 1] = s * (fx * r.r10 + fy * r.r11);
    pos_deriv[3 * (size_t)atom + 2] = s * (fx * r.r20 + fy * r.r21 + fz * r.r22);
    charge_deriv[atom] = dq * sqrt_coulomb;
}

// ---- box gradient of the reciprocal term: dE_m/dB_m = - B_m^-T (Pi_m + X_m) ----
// Pi: a pass of its own over the grids pme_recip_convolve_frames has scaled (that kernel keeps its bits), frame and workgroup from
// blockIdx.x as there, the convolution's float expressions for eterm, the six float64 sums of pme_recip_box_pi (without the 1/2) per
// (frame, workgroup) into pi_partial [B][cb][6].  Points whose eterm underflows add nothing.
__global__ __launch_bounds__(kBlock) void pme_recip_box_pi_frames(int gx, int gy, int gz, int cb, const float* __restrict__ boxes,
                                                                 float recip_exp_factor, const float* __restrict__ xmod,
                                                                 const float* __restrict__ ymod, const float* __restrict__ zmod,
                                                                 const float2* __restrict__ cgrids, double* __restrict__ pi_partial) {
    __shared__ double red[kBlock / 64][6];
    const int frame = blockIdx.x / cb, blk = blockIdx.x % cb;               // (the host launches exactly B * cb workgroups)
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = boxes[9 * (size_t)frame + i];        // (uniform: scalar loads)
    const RecipBox r = recip_box(b);
    const float scale_factor = (float)M_PI * b[0] * b[4] * b[8];
    const int zsize = gz / 2 + 1;
    const long long points = (long long)gx * gy * zsize;
    const float2* cgrid = cgrids + (size_t)frame * points;
    double pi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long idx = (long long)blk * kBlock + threadIdx.x; idx < points; idx += (long long)cb * kBlock) {
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

// One workgroup per frame: lane t adds the frame's Pi partials t, t + 256, ... and, for X = sum_j x_j (x) g_j, its atoms
// offsets[m] + t, + 256, ... from the positions as passed and the unscaled interpolated dE/dpositions (float64 products); the fifteen
// sums go through the xor tree, then the four waves in order; one lane forms the general 3 x 3 inverse of B_m in float64 and stores
// - B_m^-T (Pi / 2 + X).  A frame's atoms are few enough for one workgroup: no separate atoms launch, and nothing here depends on the
// batch around the frame.  An empty frame has zero grids and no atoms: zeros.
__global__ __launch_bounds__(kBlock) void pme_recip_box_finish_frames(int N, int cb, const int32_t* __restrict__ offsets,
                                                                     const double* __restrict__ pi_partial, const float* __restrict__ pos,
                                                                     const float* __restrict__ pos_deriv, const float* __restrict__ boxes,
                                                                     float* __restrict__ box_deriv) {
    __shared__ double red[kBlock / 64][15];
    const int frame = blockIdx.x;
    const int a0 = min(max(offsets[frame], 0), N), a1 = min(max(offsets[frame + 1], a0), N);
    double acc[15];
#pragma unroll
    for (int q = 0; q < 15; q++) acc[q] = 0.0;
    for (int k = threadIdx.x; k < cb; k += kBlock) {
#pragma unroll
        for (int q = 0; q < 6; q++) acc[q] += pi_partial[((size_t)frame * cb + k) * 6 + q];
    }
    for (int atom = a0 + (int)threadIdx.x; atom < a1; atom += kBlock) {
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int c = 0; c < 3; c++) acc[6 + 3 * a + c] += (double)pos[3 * (size_t)atom + a] * (double)pos_deriv[3 * (size_t)atom + c];
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
        double Bm[9];
        for (int q = 0; q < 9; q++) Bm[q] = (double)boxes[9 * (size_t)frame + q];
        // B^-1 = adj(B) / det(B)
        const double c00 = Bm[4] * Bm[8] - Bm[5] * Bm[7], c01 = Bm[5] * Bm[6] - Bm[3] * Bm[8], c02 = Bm[3] * Bm[7] - Bm[4] * Bm[6];
        const double det = Bm[0] * c00 + Bm[1] * c01 + Bm[2] * c02;
        const double inv[9] = {c00 / det, (Bm[2] * Bm[7] - Bm[1] * Bm[8]) / det, (Bm[1] * Bm[5] - Bm[2] * Bm[4]) / det,
                               c01 / det, (Bm[0] * Bm[8] - Bm[2] * Bm[6]) / det, (Bm[2] * Bm[3] - Bm[0] * Bm[5]) / det,
                               c02 / det, (Bm[1] * Bm[6] - Bm[0] * Bm[7]) / det, (Bm[0] * Bm[4] - Bm[1] * Bm[3]) / det};
        for (int a = 0; a < 3; a++)
            for (int c = 0; c < 3; c++)       // (B^-T M)[a][c] = sum_k B^-1[k][a] M[k][c]
                box_deriv[9 * (size_t)frame + 3 * a + c] = (float)(0.0 - (inv[a] * M[c] + inv[3 + a] * M[3 + c] + inv[6 + a] * M[6 + c]));
    }
}

int check_recip(int num_atoms, int num_frames, int gx, int gy, int gz, int order) {
    NNPOPS_REQUIRE(num_atoms >= 0 && num_frames >= 1, "bad sizes (atoms %d, frames %d)", num_atoms, num_frames);
    NNPOPS_REQUIRE(gx >= 1 && gy >= 1 && gz >= 1, "the grid dimensions must be positive (%d, %d, %d)", gx, gy, gz);
    const long long points = (long long)gx * gy * gz;
    NNPOPS_REQUIRE(points <= 0x7fffffffll, "grid of %lld points is too large", points);
    NNPOPS_REQUIRE((long long)num_frames * std::max<long long>(make_dims(gx, gy, gz).nbins, conv_blocks(gx, gy, gz)) <= 0x7fffffffll,
                   "%d frames of a %d x %d x %d grid are too many workgroups for one launch", num_frames, gx, gy, gz);
    NNPOPS_REQUIRE(order == 4 || order == 5, "Only pmeOrder 4 or 5 is supported (got %d)", order);
    return NNPOPS_OK;
}

int64_t count_tiles(int num_frames, const int64_t* offsets) {
    int64_t T = 0;
    for (int m = 0; m < num_frames; m++) T += (offsets[m + 1] - offsets[m] + kTileOwners - 1) / kTileOwners;
    return T;
}

}  // namespace

extern "C" {

int64_t nnpops_pme_frames_table_ints(int num_frames, const int64_t* offsets) {
    NNPOPS_REQUIRE(num_frames >= 0 && offsets != nullptr, "Expected \"offsets\" to hold at least one entry");
    NNPOPS_REQUIRE(offsets[0] == 0, "Expected \"offsets\" to start at 0");
    for (int m = 0; m < num_frames; m++) NNPOPS_REQUIRE(offsets[m + 1] >= offsets[m], "Expected \"offsets\" to be ascending");
    NNPOPS_REQUIRE(offsets[num_frames] <= std::numeric_limits<int32_t>::max() / 8, "Too many atoms for the PME frames table");
    return 4 + 2 * ((int64_t)num_frames + 1) + 4 * count_tiles(num_frames, offsets) + offsets[num_frames];
}

int nnpops_pme_frames_table(int num_frames, const int64_t* offsets, int32_t* table) {
    NNPOPS_REQUIRE(table != nullptr, "NULL table pointer");
    if (nnpops_pme_frames_table_ints(num_frames, offsets) < 0) return NNPOPS_ERR_INVALID_ARGUMENT;
    const int64_t T = count_tiles(num_frames, offsets);
    table[0] = num_frames; table[1] = (int32_t)offsets[num_frames]; table[2] = (int32_t)T; table[3] = 0;
    int32_t* off = table + 4;
    int32_t* tile_start = off + (num_frames + 1);
    int32_t* tiles = tile_start + (num_frames + 1);
    int32_t* atom_frame = tiles + 4 * T;
    int32_t t = 0;
    for (int m = 0; m < num_frames; m++) {
        const int32_t first = (int32_t)offsets[m], n = (int32_t)(offsets[m + 1] - offsets[m]);
        off[m] = first;
        tile_start[m] = t;
        for (int32_t o = 0; o < n; o += kTileOwners, t++) {
            int32_t* r = tiles + 4 * (size_t)t;
            r[0] = m; r[1] = first; r[2] = n; r[3] = first + o;
        }
        for (int32_t a = 0; a < n; a++) atom_frame[first + a] = m;
    }
    off[num_frames] = (int32_t)offsets[num_frames];
    tile_start[num_frames] = t;
    return NNPOPS_OK;
}

int64_t nnpops_pme_direct_frames_workspace_bytes(int num_tiles) {
    return num_tiles < 0 ? 0 : (int64_t)sizeof(double) * std::max(num_tiles, 1) + 256;
}

int nnpops_pme_direct_frames(int num_atoms, int num_frames, int num_tiles, int max_exclusions, const int32_t* table, const float* positions,
                             const float* charges, const int32_t* exclusions, const float* box_vectors, float cutoff, float alpha,
                             float coulomb, float* energies, float* position_deriv, float* charge_deriv, void* workspace, void* stream) {
    NNPOPS_REQUIRE(num_atoms >= 0 && num_frames >= 1 && num_tiles >= 0 && max_exclusions >= 0, "bad sizes (atoms %d, frames %d, tiles %d, exclusions %d)",
                   num_atoms, num_frames, num_tiles, max_exclusions);
    NNPOPS_REQUIRE(cutoff > 0 && alpha > 0 && coulomb > 0, "cutoff, alpha and coulomb must be positive");
    NNPOPS_REQUIRE(table && box_vectors && energies && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && charges && position_deriv && charge_deriv), "NULL device pointer");
    NNPOPS_REQUIRE(max_exclusions == 0 || num_atoms == 0 || exclusions, "NULL exclusions pointer");
    hipStream_t s = (hipStream_t)stream;
    const TableView v = view(table, num_frames, num_tiles);
    double* tile_energy = (double*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (num_tiles > 0)
        hipLaunchKernelGGL(pme_direct_frames, dim3(num_tiles), dim3(kBlock), 0, s, num_atoms, num_frames, max_exclusions, v.tiles, positions,
                           charges, exclusions, box_vectors, cutoff * cutoff, alpha, coulomb, position_deriv, charge_deriv, tile_energy);
    hipLaunchKernelGGL(pme_frames_energy, dim3(num_frames), dim3(64), 0, s, v.tile_start, 0, num_tiles, (const double*)tile_energy, 1.0, energies);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int64_t nnpops_pme_reciprocal_frames_workspace_bytes(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order) {
    if (check_recip(num_atoms, num_frames, gridx, gridy, gridz, order) != NNPOPS_OK) return 0;
    return (int64_t)carve(nullptr, num_atoms, num_frames, gridx, gridy, gridz, order).bytes;
}

int nnpops_pme_reciprocal_frames_spread(int num_atoms, int num_frames, int num_tiles, int gridx, int gridy, int gridz, int order,
                                        const int32_t* table, const float* positions, const float* charges, const float* box_vectors,
                                        float coulomb, float* real_grids, void* workspace, void* stream) {
    if (int rc = check_recip(num_atoms, num_frames, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0 && num_tiles >= 0, "coulomb must be positive");
    NNPOPS_REQUIRE(table && box_vectors && real_grids && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && charges), "NULL positions / charges pointer");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const TableView v = view(table, num_frames, num_tiles);
    const RecipWorkspace w = carve(workspace, num_atoms, num_frames, gridx, gridy, gridz, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    const unsigned blocks = (unsigned)num_frames * (unsigned)d.nbins;
    if (order == 4) {
        if (num_atoms > 0)
            hipLaunchKernelGGL(pme_recip_spline_frames<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, v.atom_frame, positions, box_vectors,
                               d, w.base, w.theta, w.dtheta);
        hipLaunchKernelGGL(pme_recip_spread_frames<4>, dim3(blocks), dim3(kBlock), 0, s, num_atoms, num_frames, v.offsets, d, (const int4*)w.base,
                           (const float*)w.theta, charges, sqrt_coulomb, real_grids);
    } else {
        if (num_atoms > 0)
            hipLaunchKernelGGL(pme_recip_spline_frames<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, v.atom_frame, positions, box_vectors,
                               d, w.base, w.theta, w.dtheta);
        hipLaunchKernelGGL(pme_recip_spread_frames<5>, dim3(blocks), dim3(kBlock), 0, s, num_atoms, num_frames, v.offsets, d, (const int4*)w.base,
                           (const float*)w.theta, charges, sqrt_coulomb, real_grids);
    }
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_frames_convolve(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order, const float* box_vectors,
                                          float alpha, const float* xmoduli, const float* ymoduli, const float* zmoduli, void* recip_grids,
                                          float* energies, void* workspace, void* stream) {
    if (int rc = check_recip(num_atoms, num_frames, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(alpha > 0, "alpha must be positive");
    NNPOPS_REQUIRE(box_vectors && xmoduli && ymoduli && zmoduli && recip_grids && energies && workspace, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const RecipWorkspace w = carve(workspace, num_atoms, num_frames, gridx, gridy, gridz, order);
    const int cb = conv_blocks(gridx, gridy, gridz);
    const float recip_exp_factor = (float)(M_PI * M_PI / ((double)alpha * (double)alpha));
    hipLaunchKernelGGL(pme_recip_convolve_frames, dim3((unsigned)num_frames * (unsigned)cb), dim3(kBlock), 0, s, gridx, gridy, gridz, cb, box_vectors,
                       recip_exp_factor, xmoduli, ymoduli, zmoduli, (float2*)recip_grids, w.partial);
    hipLaunchKernelGGL(pme_frames_energy, dim3(num_frames), dim3(64), 0, s, (const int32_t*)nullptr, cb, num_frames * cb, (const double*)w.partial,
                       0.5, energies);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_frames_interpolate(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order, const float* charges,
                                             const float* box_vectors, float coulomb, const float* real_grids, float* position_deriv,
                                             float* charge_deriv, void* workspace, void* stream) {
    if (int rc = check_recip(num_atoms, num_frames, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0, "coulomb must be positive");
    NNPOPS_REQUIRE(box_vectors && real_grids && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (charges && position_deriv && charge_deriv), "NULL charges / derivative pointer");
    if (num_atoms == 0) return NNPOPS_OK;
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const RecipWorkspace w = carve(workspace, num_atoms, num_frames, gridx, gridy, gridz, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    if (order == 4)
        hipLaunchKernelGGL(pme_recip_interp_frames<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, d, box_vectors, charges, sqrt_coulomb,
                           (const int4*)w.base, (const float*)w.theta, (const float*)w.dtheta, real_grids, position_deriv, charge_deriv);
    else
        hipLaunchKernelGGL(pme_recip_interp_frames<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, d, box_vectors, charges, sqrt_coulomb,
                           (const int4*)w.base, (const float*)w.theta, (const float*)w.dtheta, real_grids, position_deriv, charge_deriv);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

// ---- box gradients: box_deriv [num_frames][3][3] = dE_m/dB_m, fully written ----
int64_t nnpops_pme_direct_frames_box_workspace_bytes(int num_tiles) {
    return num_tiles < 0 ? 0 : (int64_t)sizeof(double) * 9 * std::max(num_tiles, 1) + 256;
}

int nnpops_pme_direct_frames_box(int num_atoms, int num_frames, int num_tiles, int max_exclusions, const int32_t* table, const float* positions,
                                 const float* charges, const int32_t* exclusions, const float* box_vectors, float cutoff, float alpha,
                                 float coulomb, float* box_deriv, void* workspace, void* stream) {
    NNPOPS_REQUIRE(num_atoms >= 0 && num_frames >= 1 && num_tiles >= 0 && max_exclusions >= 0, "bad sizes (atoms %d, frames %d, tiles %d, exclusions %d)",
                   num_atoms, num_frames, num_tiles, max_exclusions);
    NNPOPS_REQUIRE(cutoff > 0 && alpha > 0 && coulomb > 0, "cutoff, alpha and coulomb must be positive");
    NNPOPS_REQUIRE(table && box_vectors && box_deriv && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && charges), "NULL device pointer");
    NNPOPS_REQUIRE(max_exclusions == 0 || num_atoms == 0 || exclusions, "NULL exclusions pointer");
    hipStream_t s = (hipStream_t)stream;
    const TableView v = view(table, num_frames, num_tiles);
    double* tile_box = (double*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (num_tiles > 0)
        hipLaunchKernelGGL(pme_direct_frames_box, dim3(num_tiles), dim3(kBlock), 0, s, num_atoms, num_frames, max_exclusions, v.tiles, positions,
                           charges, exclusions, box_vectors, cutoff * cutoff, alpha, coulomb, tile_box);
    hipLaunchKernelGGL(pme_frames_box_sum, dim3(num_frames), dim3(64), 0, s, v.tile_start, num_tiles, (const double*)tile_box, box_deriv);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int64_t nnpops_pme_reciprocal_frames_box_workspace_bytes(int num_frames, int gridx, int gridy, int gridz) {
    if (check_recip(0, num_frames, gridx, gridy, gridz, 4) != NNPOPS_OK) return 0;
    return (int64_t)sizeof(double) * 6 * (int64_t)num_frames * conv_blocks(gridx, gridy, gridz) + 256;
}

int nnpops_pme_reciprocal_frames_box_pi(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order, const float* box_vectors,
                                        float alpha, const float* xmoduli, const float* ymoduli, const float* zmoduli, const void* recip_grids,
                                        void* box_workspace, void* stream) {
    if (int rc = check_recip(num_atoms, num_frames, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(alpha > 0, "alpha must be positive");
    NNPOPS_REQUIRE(box_vectors && xmoduli && ymoduli && zmoduli && recip_grids && box_workspace, "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    const int cb = conv_blocks(gridx, gridy, gridz);
    const float recip_exp_factor = (float)(M_PI * M_PI / ((double)alpha * (double)alpha));
    double* pi_partial = (double*)(((uintptr_t)box_workspace + 255) & ~(uintptr_t)255);
    hipLaunchKernelGGL(pme_recip_box_pi_frames, dim3((unsigned)num_frames * (unsigned)cb), dim3(kBlock), 0, s, gridx, gridy, gridz, cb, box_vectors,
                       recip_exp_factor, xmoduli, ymoduli, zmoduli, (const float2*)recip_grids, pi_partial);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_frames_box_gradient(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order,
                                              const int32_t* table, const float* positions, const float* position_deriv,
                                              const float* box_vectors, float* box_deriv, void* box_workspace, void* stream) {
    if (int rc = check_recip(num_atoms, num_frames, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(table && box_vectors && box_deriv && box_workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && position_deriv), "NULL positions / derivative pointer");
    hipStream_t s = (hipStream_t)stream;
    const TableView v = view(table, num_frames, 0);                         // (the offsets come before the tiles)
    const double* pi_partial = (const double*)(((uintptr_t)box_workspace + 255) & ~(uintptr_t)255);
    hipLaunchKernelGGL(pme_recip_box_finish_frames, dim3(num_frames), dim3(kBlock), 0, s, num_atoms, conv_blocks(gridx, gridy, gridz), v.offsets,
                       pi_partial, positions, position_deriv, box_vectors, box_deriv);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // extern "C"
