// pme_frames_second_order.hip -- the double backward of both PME terms over a BATCH OF FRAMES with respect to positions and charges
// (the formulae are s8d's, the batch shape is s8e's).  The first backward of the per-frame energies returns g_m P and
// g_m C (P = dE/dpositions, C = dE/dcharges of frame m, g_m its upstream gradient).  With cotangents v [N][3] and w [N] of those two
// outputs this unit computes the gradients of
//     L = sum_m g_m sum_{i in m} (v_i . P_i + w_i C_i)
// with respect to positions, charges and g.  The single-system kernels (pme_second_order.hip, pme_recip.hip) cannot be re-indexed: the
// direct one streams a pair list through a transposed index and the frames path has no pair list; the reciprocal one walks the sorted
// bricks the single-system spread leaves behind and the frames spread has no sort.
//
//   pme_direct_frames_double     the work split of pme_direct_frames: one workgroup per tile of 16 owner atoms, 16 lanes per owner, the
//                                frame's positions, charges, v and w staged in LDS (eight floats per atom, up to kFrameLdsAtoms atoms:
//                                32 KiB; global reads beyond).  Owner i's lanes walk j = sub, sub + 16, ...; the displacement of the pair
//                                (max(i, j), min(i, j)), the keep rule and the exclusion test are the forward's; s, c and T of s8d are
//                                evaluated with the higher index first by BOTH owners, so both ends see the same float values, and the
//                                owner's sign is applied last.  Then the owner walks its own exclusion row for the un-wrapped erf terms.
//                                float64 sums per lane in j order, the 16 lanes in the fixed xor order, times g_m, one store per owner.
//                                No atomics, no workspace.
//   pme_recip_spline2_frames     one lane per atom: theta, dtheta, d2theta in double from the float offset, recomputed in the atom's own
//                                frame's box with the forward's wrapping and base index; s_a = K_a (v . B_m^-1 column a).
//   pme_recip_spread_dir_frames  Q' = sum_i [w_i W_i + q_i (v_i . grad) W_i] with the structure of pme_recip_spread_frames (one workgroup
//                                per frame and brick, ballot ranks into consecutive LDS slots, flushes in slot order); the six axis
//                                arrays of pme_recip_gather_dir staged per kept atom, atom-major with an odd stride.
//   pme_recip_interp2_frames     one lane per atom over the order^3 stencil of phi and phi' in its own frame's slab, the sums along z
//                                first, double weights and double sums; writes dL/dx and dL/dq times g_m.
//   pme_frames_upstream_grad     one wave per frame: dL/dg_m = sum_{i in m} (v_i . P_i + w_i C_i) on the saved first-order outputs.
//
// The table, the forward's reciprocal workspace (partial sums | base | theta | dtheta) and the brick shape are pme_frames.hip's; that
// unit is not edited (its kernels keep their assembly), so the few lines that describe them are repeated here and must follow it.
// Every table entry is clamped to the arrays; the boxes and g are read on the device, so a captured graph follows them.
// Compiled without packed float32 arithmetic, as pme_frames.hip (build.py): the keep rule must round as the forward's does.
#include <cmath>
#include <limits>

#include "device_common.h"
#include "host_common.h"
#include "pair_delta.h"
#include "pme_recip_common.h"

using namespace nnpops;

namespace {

constexpr int kBlock = 256;
constexpr int kTileOwners = NNPOPS_PME_FRAMES_TILE;
constexpr int kFrameLdsAtoms = 1024;                   // eight floats per atom: 32 KiB of LDS per workgroup
constexpr int kBX = 4, kBY = 4, kBZ = 16;              // brick of grid points = one spread workgroup
constexpr int kConvBlocksMax = 1024;
constexpr float kTwoOverSqrtPi = 1.12837916709551257390f;
static_assert(kTileOwners * 16 == kBlock && kBX * kBY * kBZ == kBlock, "one lane per (owner, sub) and per grid point of a brick");

// ---- the table and the forward's workspace, as pme_frames.hip lays them out ----
struct TableView {
    const int32_t *offsets, *tile_start, *tiles, *atom_frame;
};
TableView view(const int32_t* table, int B, int T) {
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

struct ForwardWorkspace {     // what nnpops_pme_reciprocal_frames_spread left behind
    const int4* base;         // [N]            base grid index (x, y, z) and the atom's frame
    const float* theta;       // [N][3][order]
    const float* dtheta;      // [N][3][order]
};
ForwardWorkspace forward_carve(const void* workspace, int num_atoms, int num_frames, int gx, int gy, int gz, int order) {
    uintptr_t p = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    auto take = [&](size_t bytes) { const uintptr_t at = p; p += (bytes + 255) & ~(size_t)255; return at; };
    const size_t n = (size_t)num_atoms;
    take(sizeof(double) * (size_t)num_frames * conv_blocks(gx, gy, gz));
    ForwardWorkspace w;
    w.base = (const int4*)take(sizeof(int4) * n);
    w.theta = (const float*)take(sizeof(float) * 3 * (size_t)order * n);
    w.dtheta = (const float*)take(sizeof(float) * 3 * (size_t)order * n);
    return w;
}

struct SecondWorkspace {
    double* wide;             // [N][3][3][order]  theta, dtheta, d2theta of the three axes, in double
    float* dir;               // [N][3]            s_a = K_a (v . B^-1 column a)
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

// ---- direct term ----
// f, f', f'' (times k) -> T and the two charge terms of the pair (a, b); u = delta / r, dv = v_a - v_b (pme_second_order.hip)
__device__ __forceinline__ void pair_second(float qa, float qb, float wa, float wb, float ux, float uy, float uz, float dvx, float dvy,
                                            float dvz, float inv_r, float f, float fp, float fpp, float (&T)[3], float& dq_a, float& dq_b) {
    const float s = ux * dvx + uy * dvy + uz * dvz;
    const float qq = qa * qb, c = wa * qb + wb * qa;
    const float a = qq * (fpp - fp * inv_r) * s + c * fp, b = qq * fp * inv_r;
    T[0] = a * ux + b * dvx; T[1] = a * uy + b * dvy; T[2] = a * uz + b * dvz;
    dq_a = qb * fp * s + wb * f;
    dq_b = qa * fp * s + wa * f;
}

__device__ __forceinline__ double group16_sum(double x) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__global__ __launch_bounds__(kBlock) void pme_direct_frames_double(int N, int B, int max_excl, const int32_t* __restrict__ tiles,
                                                                    const float* __restrict__ pos, const float* __restrict__ charge,
                                                                    const int* __restrict__ excl, const float* __restrict__ boxes,
                                                                    const float* __restrict__ v, const float* __restrict__ w,
                                                                    const float* __restrict__ upstream, float cutoff2, float alpha,
                                                                    float coulomb, float* __restrict__ grad_pos,
                                                                    float* __restrict__ grad_charge) {
    __shared__ float spos[3 * kFrameLdsAtoms];
    __shared__ float sv[3 * kFrameLdsAtoms];
    __shared__ float sq[kFrameLdsAtoms];
    __shared__ float sw[kFrameLdsAtoms];
    const Tile t = load_tile(tiles, blockIdx.x, N, B);
    const float* box = boxes + 9 * (size_t)t.frame;                         // (uniform address: scalar loads)
    const float g = upstream[t.frame];
    const float* fpos = pos + 3 * (size_t)t.first;
    const float* fv = v + 3 * (size_t)t.first;
    const float* fq = charge + t.first;
    const float* fw = w + t.first;
    const bool staged = t.n <= kFrameLdsAtoms;
    if (staged) {
        for (int k = threadIdx.x; k < 3 * t.n; k += kBlock) { spos[k] = fpos[k]; sv[k] = fv[k]; }
        for (int k = threadIdx.x; k < t.n; k += kBlock) { sq[k] = fq[k]; sw[k] = fw[k]; }
    }
    __syncthreads();
    const int sub = threadIdx.x & 15;
    const int i = t.owner0 - t.first + (threadIdx.x >> 4);                  // the owner, counted inside its frame
    const bool live = i < t.n;
    const int gi = t.first + i;
    double sx = 0.0, sy = 0.0, sz = 0.0, sc = 0.0;
    auto walk = [&](const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ V, const float* __restrict__ W) {
        const float qi = Q[i], wi = W[i], vix = V[3 * i], viy = V[3 * i + 1], viz = V[3 * i + 2];
        const int* row = excl + (size_t)gi * max_excl;
        for (int j = sub; j < t.n; j += 16) {
            if (j == i) continue;
            const bool upper = i > j;                                        // the pair is (max, min), as the forward has it
            const Vec3<float> d = wrapped_delta<float>(P, upper ? i : j, upper ? j : i, box, true);
            const float d2 = allpairs_norm2<float>(d);
            if (d2 > cutoff2) continue;
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
            const float ex = expf(-ar * ar) * kTwoOverSqrtPi, erfc_ar = erfcf(ar);
            const float pre = coulomb * inv_r;
            const float f = pre * erfc_ar;
            const float fp = -pre * (erfc_ar + ar * ex) * inv_r;
            const float fpp = 2.0f * pre * (erfc_ar + ar * ex + ar * ar * ar * ex) * inv_r * inv_r;
            // the higher index first for both owners: the same float values at both ends of the pair
            const float qj = Q[j], wj = W[j], vjx = V[3 * j], vjy = V[3 * j + 1], vjz = V[3 * j + 2];
            const float dvx = upper ? vix - vjx : vjx - vix, dvy = upper ? viy - vjy : vjy - viy, dvz = upper ? viz - vjz : vjz - viz;
            float T[3], dq_hi, dq_lo;
            pair_second(upper ? qi : qj, upper ? qj : qi, upper ? wi : wj, upper ? wj : wi, d.x * inv_r, d.y * inv_r, d.z * inv_r, dvx, dvy,
                        dvz, inv_r, f, fp, fpp, T, dq_hi, dq_lo);
            sx += (double)(upper ? T[0] : -T[0]); sy += (double)(upper ? T[1] : -T[1]); sz += (double)(upper ? T[2] : -T[2]);
            sc += (double)(upper ? dq_hi : dq_lo);
        }
        // excluded pairs of this owner (its own row; the table is symmetric): f = -k erf(alpha r) / r on the un-wrapped difference
        const float px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
        for (int e = sub; e < max_excl; e += 16) {
            const int other = row[e];
            const int o = other - t.first;
            if (other == gi || (unsigned)o >= (unsigned)t.n) continue;      // (-1 padding; a partner outside the frame is never read)
            const float dx = px - P[3 * o], dy = py - P[3 * o + 1], dz = pz - P[3 * o + 2];
            const float r = sqrtf(dx * dx + dy * dy + dz * dz);
            const float inv_r = 1.0f / r, ar = alpha * r;
            const float ex = expf(-ar * ar) * kTwoOverSqrtPi, erf_ar = erff(ar);
            const float pre = coulomb * inv_r;
            const float f = -pre * erf_ar;
            const float fp = pre * (erf_ar - ar * ex) * inv_r;
            const float fpp = 2.0f * pre * (ar * ex + ar * ar * ar * ex - erf_ar) * inv_r * inv_r;
            float T[3], dq_i, dq_o;
            pair_second(qi, Q[o], wi, W[o], dx * inv_r, dy * inv_r, dz * inv_r, vix - V[3 * o], viy - V[3 * o + 1], viz - V[3 * o + 2], inv_r,
                        f, fp, fpp, T, dq_i, dq_o);
            sx += (double)T[0]; sy += (double)T[1]; sz += (double)T[2]; sc += (double)dq_i;
        }
    };
    if (live) {
        if (staged) walk(spos, sq, sv, sw); else walk(fpos, fq, fv, fw);
    }
    sx = group16_sum(sx); sy = group16_sum(sy); sz = group16_sum(sz); sc = group16_sum(sc);
    if (live && sub == 0) {
        const double gd = (double)g;
        grad_pos[3 * (size_t)gi] = (float)(gd * sx); grad_pos[3 * (size_t)gi + 1] = (float)(gd * sy); grad_pos[3 * (size_t)gi + 2] = (float)(gd * sz);
        grad_charge[gi] = (float)(gd * sc);
    }
}

// dL/dg_m = sum over frame m's atoms of v . P + w C, float64, lane l adds atoms l, l + 64, ..., then the xor order: one wave per frame,
// a frame's value does not depend on the batch around it; a frame without atoms gets 0.
__global__ __launch_bounds__(64) void pme_frames_upstream_grad(int N, const int32_t* __restrict__ offsets, const float* __restrict__ v,
                                                               const float* __restrict__ w, const float* __restrict__ pos_deriv,
                                                               const float* __restrict__ charge_deriv, float* __restrict__ grad_upstream) {
    const int m = blockIdx.x;
    const int a0 = min(max(offsets[m], 0), N), a1 = min(max(offsets[m + 1], a0), N);
    double s = 0.0;
    for (int atom = a0 + (int)threadIdx.x; atom < a1; atom += 64) {
        const size_t k = 3 * (size_t)atom;
        s += (double)v[k] * (double)pos_deriv[k] + (double)v[k + 1] * (double)pos_deriv[k + 1] + (double)v[k + 2] * (double)pos_deriv[k + 2] +
             (double)w[atom] * (double)charge_deriv[atom];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (threadIdx.x == 0) grad_upstream[m] = (float)s;
}

// ---- reciprocal term ----
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_spline2_frames(int N, int B, const int32_t* __restrict__ atom_frame,
                                                                   const float* __restrict__ pos, const float* __restrict__ boxes, Dims d,
                                                                   const int4* __restrict__ base, const float* __restrict__ v,
                                                                   double* __restrict__ wide, float* __restrict__ dir) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= N) return;
    const int frame = min(max(atom_frame[atom], 0), B - 1);
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = boxes[9 * (size_t)frame + i];
    const RecipBox r = recip_box(b);
    float p[3] = {pos[3 * atom], pos[3 * atom + 1], pos[3 * atom + 2]};
    const float rdiag[3] = {r.r00, r.r11, r.r22};
#pragma unroll
    for (int i = 2; i >= 0; i--) {                        // into the reduced box, c then b then a (as spline_atom)
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
        // spline_atom's recursion in double from the float offset, kept at orders ORDER - 2 (differenced twice: d2theta), ORDER - 1
        // (differenced: dtheta) and ORDER (theta): d2theta must sum to zero over the stencil beyond float rounding
        const double x = dr;
        double wt[ORDER];
#pragma unroll
        for (int j = 0; j < ORDER; j++) wt[j] = 0.0;
        wt[1] = x;
        wt[0] = 1.0 - x;
        auto raise = [&](int j) {
            const double div = 1.0 / (j - 1);
            wt[j - 1] = div * x * wt[j - 2];
#pragma unroll
            for (int k = 1; k < j - 1; k++) wt[j - k - 1] = div * ((x + k) * wt[j - k - 2] + (j - k - x) * wt[j - k - 1]);
            wt[0] = div * (1.0 - x) * wt[0];
        };
#pragma unroll
        for (int j = 3; j <= ORDER - 2; j++) raise(j);
#pragma unroll
        for (int j = 0; j < ORDER; j++) {
            const double lo = j >= 2 ? wt[j - 2] : 0.0, mid = j >= 1 ? wt[j - 1] : 0.0;    // (wt[ORDER-2], wt[ORDER-1] are zero)
            wd[(6 + i) * ORDER + j] = lo - 2.0 * mid + wt[j];
        }
        raise(ORDER - 1);
        wd[(3 + i) * ORDER] = -wt[0];
#pragma unroll
        for (int j = 1; j < ORDER; j++) wd[(3 + i) * ORDER + j] = wt[j - 1] - wt[j];
        raise(ORDER);
#pragma unroll
        for (int j = 0; j < ORDER; j++) wd[i * ORDER + j] = wt[j];
    }
    const float vx = v[3 * atom], vy = v[3 * atom + 1], vz = v[3 * atom + 2];
    dir[3 * atom] = K[0] * (vx * r.r00 + vy * r.r10 + vz * r.r20);
    dir[3 * atom + 1] = K[1] * (vy * r.r11 + vz * r.r21);
    dir[3 * atom + 2] = K[2] * (vz * r.r22);
}

// does the cyclic stencil [g0, g0 + ORDER - 1] mod K meet the points [lo, hi] of a brick?  (pme_frames.hip)
template <int ORDER>
__device__ __forceinline__ bool stencil_meets(int g0, int lo, int hi, int K) {
    if (ORDER >= K) return true;
    int ahead = lo - g0, behind = g0 - lo;
    ahead += ahead < 0 ? K : 0;
    behind += behind < 0 ? K : 0;
    return ahead < ORDER || behind <= hi - lo;
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

// Q'(m) += A_x ty tz + (q tx) (Dy tz + ty Dz) over the frame's atoms in ascending order, A_x = w theta_x + q s_x dtheta_x, D_a = s_a
// dtheta_a: pme_recip_spread_frames' walk (256 atoms a round, kept atoms ranked by ballot and prefix popcount into consecutive slots, a
// flush when the slots cannot take the next round and at the end) with pme_recip_gather_dir's staging: the six axis arrays of a kept
// atom lie atom-major with an odd stride, so a lane reads only the slot its point needs (lanes of a wave ask for at most ORDER
// neighbouring words per array: no bank conflict).  Every point of every frame is written exactly once; a frame without atoms gets zeros.
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_spread_dir_frames(int N, int B, const int32_t* __restrict__ offsets, Dims d,
                                                                      const int4* __restrict__ base, const float* __restrict__ theta,
                                                                      const float* __restrict__ dtheta, const float* __restrict__ dir,
                                                                      const float* __restrict__ charge, const float* __restrict__ wq,
                                                                      float sqrt_coulomb, float* __restrict__ grids) {
    __shared__ int s_base[3][kBlock];
    __shared__ float s_w[kBlock][6 * ORDER + 1];           // [slot][array * ORDER + i]: Ax, Qx, Ty, Dy, Tz, Dz (odd stride)
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
                float ax, qx, ty, dy, tz, dz;
                axis_weights2<ORDER>(gx, s_base[0][k], d.kx, &s_w[k][0], ax, qx);
                axis_weights2<ORDER>(gy, s_base[1][k], d.ky, &s_w[k][2 * ORDER], ty, dy);
                axis_weights2<ORDER>(gz, s_base[2][k], d.kz, &s_w[k][4 * ORDER], tz, dz);
                acc += ax * ty * tz + qx * (dy * tz + ty * dz);
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
        for (int wv = 0; wv < kBlock / 64; wv++) {
            const int c = s_kept[wv];
            before += wv < wave ? c : 0;
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
            const float qs = charge[atom] * sqrt_coulomb, ws = wq[atom] * sqrt_coulomb;
            const float sx = dir[3 * atom], sy = dir[3 * atom + 1], sz = dir[3 * atom + 2];
            const float* th = theta + (size_t)atom * 3 * ORDER;
            const float* dth = dtheta + (size_t)atom * 3 * ORDER;
#pragma unroll
            for (int i = 0; i < ORDER; i++) {
                s_w[slot][i] = ws * th[i] + qs * sx * dth[i];
                s_w[slot][ORDER + i] = qs * th[i];
                s_w[slot][2 * ORDER + i] = th[ORDER + i];
                s_w[slot][3 * ORDER + i] = sy * dth[ORDER + i];
                s_w[slot][4 * ORDER + i] = th[2 * ORDER + i];
                s_w[slot][5 * ORDER + i] = sz * dth[2 * ORDER + i];
            }
        }
        filled += round;
        __syncthreads();                                   // (the slots are complete; s_kept may be rewritten)
    }
    add_slots(filled);
    if (live) grids[(((size_t)frame * d.kx + gx) * d.ky + gy) * d.kz + gz] = acc;
}

// one lane per atom over its order^3 stencil of both grids in its own frame's slab: the sums along z first, then the x / y weights.
// Double weights and double sums (d_a d_b W . phi differences the potential grid twice), the result times g_m.
template <int ORDER>
__global__ __launch_bounds__(kBlock) void pme_recip_interp2_frames(int N, int B, Dims d, const float* __restrict__ boxes,
                                                                   const float* __restrict__ charge, const float* __restrict__ wq,
                                                                   const float* __restrict__ upstream, float sqrt_coulomb,
                                                                   const int4* __restrict__ base, const double* __restrict__ wide,
                                                                   const float* __restrict__ dir, const float* __restrict__ phis,
                                                                   const float* __restrict__ phis2, float* __restrict__ grad_pos,
                                                                   float* __restrict__ grad_charge) {
    const int atom = blockIdx.x * kBlock + threadIdx.x;
    if (atom >= N) return;
    const int4 b0 = base[atom];
    const int frame = min(max(b0.w, 0), B - 1);
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = boxes[9 * (size_t)frame + i];
    const RecipBox r = recip_box(b);
    const float* phi = phis + (size_t)frame * d.kx * d.ky * d.kz;
    const float* phi2 = phis2 + (size_t)frame * d.kx * d.ky * d.kz;
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
                const double gv = phi[row + iz[e]], gv2 = phi2[row + iz[e]];
                z0 += tz[e] * gv; z1 += dz[e] * gv; z2 += cz[e] * gv;
                p0 += tz[e] * gv2; p1 += dz[e] * gv2;
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
    const double g = (double)upstream[frame];
    grad_charge[atom] = (float)(g * (sqrt_coulomb * (a2 + sx * hx + sy * hy + sz * hz)));
    const double fx = (qs * (g2x + sx * hxx + sy * hxy + sz * hxz) + ws * hx) * d.kx;
    const double fy = (qs * (g2y + sx * hxy + sy * hyy + sz * hyz) + ws * hy) * d.ky;
    const double fz = (qs * (g2z + sx * hxz + sy * hyz + sz * hzz) + ws * hz) * d.kz;
    grad_pos[3 * (size_t)atom] = (float)(g * (fx * r.r00));
    grad_pos[3 * (size_t)atom + 1] = (float)(g * (fx * r.r10 + fy * r.r11));
    grad_pos[3 * (size_t)atom + 2] = (float)(g * (fx * r.r20 + fy * r.r21 + fz * r.r22));
}

int check_recip(int num_atoms, int num_frames, int gx, int gy, int gz, int order) {
    NNPOPS_REQUIRE(num_atoms >= 0 && num_frames >= 1, "bad sizes (atoms %d, frames %d)", num_atoms, num_frames);
    NNPOPS_REQUIRE(gx >= 1 && gy >= 1 && gz >= 1, "the grid dimensions must be positive (%d, %d, %d)", gx, gy, gz);
    const long long points = (long long)gx * gy * gz;
    NNPOPS_REQUIRE(points <= 0x7fffffffll, "grid of %lld points is too large", points);
    NNPOPS_REQUIRE((long long)num_frames * make_dims(gx, gy, gz).nbins <= 0x7fffffffll,
                   "%d frames of a %d x %d x %d grid are too many workgroups for one launch", num_frames, gx, gy, gz);
    NNPOPS_REQUIRE(order == 4 || order == 5, "Only pmeOrder 4 or 5 is supported (got %d)", order);
    return NNPOPS_OK;
}

}  // namespace

extern "C" {

int64_t nnpops_pme_direct_frames_double_backward_workspace_bytes(int num_tiles) {
    return num_tiles < 0 ? 0 : 256;                       // the pass keeps its sums in registers: nothing beyond the alignment slack
}

int nnpops_pme_direct_frames_double_backward(int num_atoms, int num_frames, int num_tiles, int max_exclusions, const int32_t* table,
                                             const float* positions, const float* charges, const int32_t* exclusions, const float* box_vectors,
                                             const float* v, const float* w, const float* upstream, float cutoff, float alpha, float coulomb,
                                             float* grad_positions, float* grad_charges, void* workspace, void* stream) {
    NNPOPS_REQUIRE(num_atoms >= 0 && num_frames >= 1 && num_tiles >= 0 && max_exclusions >= 0, "bad sizes (atoms %d, frames %d, tiles %d, exclusions %d)",
                   num_atoms, num_frames, num_tiles, max_exclusions);
    NNPOPS_REQUIRE(cutoff > 0 && alpha > 0 && coulomb > 0, "cutoff, alpha and coulomb must be positive");
    NNPOPS_REQUIRE(table && box_vectors && upstream && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && charges && v && w && grad_positions && grad_charges), "NULL device pointer");
    NNPOPS_REQUIRE(max_exclusions == 0 || num_atoms == 0 || exclusions, "NULL exclusions pointer");
    if (num_tiles == 0) return NNPOPS_OK;
    const TableView tv = view(table, num_frames, num_tiles);
    hipLaunchKernelGGL(pme_direct_frames_double, dim3(num_tiles), dim3(kBlock), 0, (hipStream_t)stream, num_atoms, num_frames, max_exclusions,
                       tv.tiles, positions, charges, exclusions, box_vectors, v, w, upstream, cutoff * cutoff, alpha, coulomb, grad_positions,
                       grad_charges);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_frames_upstream_grad(int num_atoms, int num_frames, const int32_t* table, const float* v, const float* w,
                                    const float* position_deriv, const float* charge_deriv, float* grad_upstream, void* stream) {
    NNPOPS_REQUIRE(num_atoms >= 0 && num_frames >= 1, "bad sizes (atoms %d, frames %d)", num_atoms, num_frames);
    NNPOPS_REQUIRE(table && grad_upstream, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (v && w && position_deriv && charge_deriv), "NULL cotangent / derivative pointer");
    const TableView tv = view(table, num_frames, 0);                        // (the offsets come before the tiles)
    hipLaunchKernelGGL(pme_frames_upstream_grad, dim3(num_frames), dim3(64), 0, (hipStream_t)stream, num_atoms, tv.offsets, v, w, position_deriv,
                       charge_deriv, grad_upstream);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int64_t nnpops_pme_reciprocal_frames_second_workspace_bytes(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order) {
    if (check_recip(num_atoms, num_frames, gridx, gridy, gridz, order) != NNPOPS_OK) return 0;
    return (int64_t)second_carve(nullptr, num_atoms, order).bytes;
}

int nnpops_pme_reciprocal_frames_spread_directional(int num_atoms, int num_frames, int num_tiles, int gridx, int gridy, int gridz, int order,
                                                    const int32_t* table, const float* positions, const float* charges,
                                                    const float* box_vectors, float coulomb, const float* v, const float* w,
                                                    float* real_grids, const void* workspace, void* second_workspace, void* stream) {
    if (int rc = check_recip(num_atoms, num_frames, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0 && num_tiles >= 0, "coulomb must be positive");
    NNPOPS_REQUIRE(table && box_vectors && real_grids && workspace && second_workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (positions && charges && v && w), "NULL positions / charges / cotangent pointer");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const TableView tv = view(table, num_frames, num_tiles);
    const ForwardWorkspace fw = forward_carve(workspace, num_atoms, num_frames, gridx, gridy, gridz, order);
    const SecondWorkspace w2 = second_carve(second_workspace, num_atoms, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    const unsigned blocks = (unsigned)num_frames * (unsigned)d.nbins;
    if (order == 4) {
        if (num_atoms > 0)
            hipLaunchKernelGGL(pme_recip_spline2_frames<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, tv.atom_frame, positions, box_vectors,
                               d, fw.base, v, w2.wide, w2.dir);
        hipLaunchKernelGGL(pme_recip_spread_dir_frames<4>, dim3(blocks), dim3(kBlock), 0, s, num_atoms, num_frames, tv.offsets, d, fw.base, fw.theta,
                           fw.dtheta, (const float*)w2.dir, charges, w, sqrt_coulomb, real_grids);
    } else {
        if (num_atoms > 0)
            hipLaunchKernelGGL(pme_recip_spline2_frames<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, tv.atom_frame, positions, box_vectors,
                               d, fw.base, v, w2.wide, w2.dir);
        hipLaunchKernelGGL(pme_recip_spread_dir_frames<5>, dim3(blocks), dim3(kBlock), 0, s, num_atoms, num_frames, tv.offsets, d, fw.base, fw.theta,
                           fw.dtheta, (const float*)w2.dir, charges, w, sqrt_coulomb, real_grids);
    }
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

int nnpops_pme_reciprocal_frames_interpolate_second(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order,
                                                    const float* charges, const float* box_vectors, float coulomb, const float* w,
                                                    const float* upstream, const float* potential_grids, const float* directional_grids,
                                                    float* grad_positions, float* grad_charges, const void* workspace,
                                                    void* second_workspace, void* stream) {
    if (int rc = check_recip(num_atoms, num_frames, gridx, gridy, gridz, order)) return rc;
    NNPOPS_REQUIRE(coulomb > 0, "coulomb must be positive");
    NNPOPS_REQUIRE(box_vectors && upstream && potential_grids && directional_grids && workspace && second_workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_atoms == 0 || (charges && w && grad_positions && grad_charges), "NULL charges / cotangent / gradient pointer");
    if (num_atoms == 0) return NNPOPS_OK;
    hipStream_t s = (hipStream_t)stream;
    const Dims d = make_dims(gridx, gridy, gridz);
    const ForwardWorkspace fw = forward_carve(workspace, num_atoms, num_frames, gridx, gridy, gridz, order);
    const SecondWorkspace w2 = second_carve(second_workspace, num_atoms, order);
    const float sqrt_coulomb = (float)std::sqrt((double)coulomb);
    const int ab = div_up(num_atoms, kBlock);
    if (order == 4)
        hipLaunchKernelGGL(pme_recip_interp2_frames<4>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, d, box_vectors, charges, w, upstream,
                           sqrt_coulomb, fw.base, (const double*)w2.wide, (const float*)w2.dir, potential_grids, directional_grids,
                           grad_positions, grad_charges);
    else
        hipLaunchKernelGGL(pme_recip_interp2_frames<5>, dim3(ab), dim3(kBlock), 0, s, num_atoms, num_frames, d, box_vectors, charges, w, upstream,
                           sqrt_coulomb, fw.base, (const double*)w2.wide, (const float*)w2.dir, potential_grids, directional_grids,
                           grad_positions, grad_charges);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // extern "C"
