// pme_second_order.hip -- the double backward of direct-space PME (pme.hip) with respect to positions and charges.
//
// The first backward of the energy returns g P (positions) and g C (charges), P = dE/dpositions, C = dE/dcharges.  With cotangents
// v [N][3] of the position gradient and w [N] of the charge gradient this file computes the gradients of
//     L = sum_i v_i . P_i + sum_i w_i C_i
// with respect to positions and charges (the caller scales them by g).  Per included pair (i = neighbors[0], j = neighbors[1],
// delta = x_i - x_j - const, r = |delta|, u = delta / r), f(r) = k erfc(alpha r) / r, ex = (2 / sqrt(pi)) exp(-(alpha r)^2):
//     f'  = -k (erfc(alpha r) + alpha r ex) / r^2
//     f'' =  k (2 erfc(alpha r) + 2 alpha r ex + 2 (alpha r)^3 ex) / r^3
//     s = u . (v_i - v_j),  c = w_i q_j + w_j q_i
//     T = [q_i q_j (f'' - f'/r) s + c f'] u + q_i q_j (f'/r) (v_i - v_j)
//     dL/dx_i += T,  dL/dx_j -= T,  dL/dq_i += q_j f' s + w_j f,  dL/dq_j += q_i f' s + w_i f
// deltas / distances enter as data, as in the first-order op: the image shifts are held fixed.  An excluded pair takes the same
// expressions with f(r) = -k erf(alpha r) / r on the un-wrapped difference, each atom reading its own (symmetric) exclusion row.
//
// Layout: OWNER COMPUTES over the pair list's transposed index (pairs_index.hip), as pme_direct_terms / pme_direct_gather_indexed:
//   pme_direct_double_terms    one lane per slot, streaming the list arrays; the inclusion test and the float expressions for erfc / exp
//                              of pme_direct_terms; writes {T, dL/dq_i} and {T, dL/dq_j} as two 16-byte records;
//   pme_direct_double_gather   16 lanes per atom: the slots it is first in, the slots it is second in, its excluded pairs, added up in
//                              double in a fixed order; every output written once.
// No atomics of any kind: bitwise reproducible.  A list grouped by neighbors[0] (what getNeighborPairs emits) is read contiguously on
// its first side through the index's row segments; any other list brings a second index, built from the list with its two rows
// swapped, whose column segments then serve the first side.
#include <cmath>

#include "device_common.h"
#include "host_common.h"

using namespace nnpops;

namespace {

constexpr int kBlock = 256;
constexpr float kTwoOverSqrtPi = 1.12837916709551257390f;

// f, f', f'' (times k) -> T and the two charge terms of one pair; u = delta / r, dv = v_i - v_j
__device__ __forceinline__ void pair_second(float qi, float qj, float wi, float wj, float ux, float uy, float uz, float dvx, float dvy,
                                            float dvz, float inv_r, float f, float fp, float fpp, float4& to_i, float& dq_j) {
    const float s = ux * dvx + uy * dvy + uz * dvz;
    const float qq = qi * qj, c = wi * qj + wj * qi;
    const float a = qq * (fpp - fp * inv_r) * s + c * fp, b = qq * fp * inv_r;
    to_i = make_float4(a * ux + b * dvx, a * uy + b * dvy, a * uz + b * dvz, qj * fp * s + wj * f);
    dq_j = qi * fp * s + wi * f;
}

__global__ __launch_bounds__(kBlock) void pme_direct_double_terms(long long num_pairs, int num_atoms, int max_excl, const int* __restrict__ nb0,
                                                                 const int* __restrict__ nb1, const float* __restrict__ deltas,
                                                                 const float* __restrict__ distances, const float* __restrict__ charge,
                                                                 const int* __restrict__ excl, const float* __restrict__ v,
                                                                 const float* __restrict__ w, float alpha, float coulomb,
                                                                 float4* __restrict__ first, float4* __restrict__ second) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < num_pairs; i += stride) {
        const int atom1 = nb0[i], atom2 = nb1[i];
        bool include = (unsigned)atom1 < (unsigned)num_atoms && (unsigned)atom2 < (unsigned)num_atoms;
        for (int j = 0; include && j < max_excl; j++) {       // exclusion rows are sorted in descending order (as pme_direct_terms)
            const int e = excl[(long long)atom1 * max_excl + j];
            if (e < atom2) break;
            if (e == atom2) include = false;
        }
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        float dq2 = 0.f;
        if (include) {
            const float r = distances[i];
            const float inv_r = 1.0f / r, ar = alpha * r;
            const float ex = expf(-ar * ar) * kTwoOverSqrtPi, erfc_ar = erfcf(ar);
            const float pre = coulomb * inv_r;
            const float f = pre * erfc_ar;
            const float fp = -pre * (erfc_ar + ar * ex) * inv_r;
            const float fpp = 2.0f * pre * (erfc_ar + ar * ex + ar * ar * ar * ex) * inv_r * inv_r;
            pair_second(charge[atom1], charge[atom2], w[atom1], w[atom2], deltas[3 * i] * inv_r, deltas[3 * i + 1] * inv_r,
                        deltas[3 * i + 2] * inv_r, v[3 * atom1] - v[3 * atom2], v[3 * atom1 + 1] - v[3 * atom2 + 1],
                        v[3 * atom1 + 2] - v[3 * atom2 + 2], inv_r, f, fp, fpp, t, dq2);
        }
        first[i] = t;                                          // what the FIRST atom of the pair adds: +T, its dL/dq
        second[i] = make_float4(t.x, t.y, t.z, dq2);           // what the SECOND atom adds: -T, its dL/dq
    }
}

__device__ __forceinline__ double group16_sum(double x) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// first_order == nullptr: the list is grouped by neighbors[0] and first_seg holds the atoms' contiguous runs of slots; otherwise
// first_seg are segments of first_order (the slots sorted by neighbors[0]).  second_seg / second_order: the slots sorted by neighbors[1].
__global__ __launch_bounds__(kBlock) void pme_direct_double_gather(int num_atoms, int max_excl, const float* __restrict__ pos,
                                                                  const float* __restrict__ charge, const int* __restrict__ excl,
                                                                  const float* __restrict__ v, const float* __restrict__ w, float alpha,
                                                                  float coulomb, const int2* __restrict__ first_seg,
                                                                  const int* __restrict__ first_order, const int2* __restrict__ second_seg,
                                                                  const int* __restrict__ second_order, const float4* __restrict__ first,
                                                                  const float4* __restrict__ second, float* __restrict__ grad_pos,
                                                                  float* __restrict__ grad_charge) {
    const int sub = threadIdx.x & 15;
    const int atom = blockIdx.x * (kBlock / 16) + (threadIdx.x >> 4);      // (whole waves reach the group shuffles: no early return)
    const bool live = atom < num_atoms;
    double sx = 0.0, sy = 0.0, sz = 0.0, sq = 0.0;
    if (live) {
        const int2 fs = first_seg[atom], ss = second_seg[atom];
        for (int k = fs.x + sub; k < fs.y; k += 16) {
            const float4 t = first[first_order ? first_order[k] : k];
            sx += (double)t.x; sy += (double)t.y; sz += (double)t.z; sq += (double)t.w;
        }
        for (int p = ss.x + sub; p < ss.y; p += 16) {
            const float4 t = second[second_order[p]];
            sx -= (double)t.x; sy -= (double)t.y; sz -= (double)t.z; sq += (double)t.w;
        }
        // excluded pairs of this atom (its own row; the table is symmetric): f = -k erf(alpha r) / r, un-wrapped
        const float px = pos[3 * atom], py = pos[3 * atom + 1], pz = pos[3 * atom + 2], c1 = charge[atom], w1 = w[atom];
        const float vx = v[3 * atom], vy = v[3 * atom + 1], vz = v[3 * atom + 2];
        for (int j = sub; j < max_excl; j += 16) {
            const int other = excl[(long long)atom * max_excl + j];
            if ((unsigned)other >= (unsigned)num_atoms || other == atom) continue;
            const float dx = px - pos[3 * other], dy = py - pos[3 * other + 1], dz = pz - pos[3 * other + 2];
            const float r = sqrtf(dx * dx + dy * dy + dz * dz);
            const float inv_r = 1.0f / r, ar = alpha * r;
            const float ex = expf(-ar * ar) * kTwoOverSqrtPi, erf_ar = erff(ar);
            const float pre = coulomb * inv_r;
            const float f = -pre * erf_ar;
            const float fp = pre * (erf_ar - ar * ex) * inv_r;
            const float fpp = 2.0f * pre * (ar * ex + ar * ar * ar * ex - erf_ar) * inv_r * inv_r;
            float4 t;
            float unused;
            pair_second(c1, charge[other], w1, w[other], dx * inv_r, dy * inv_r, dz * inv_r, vx - v[3 * other], vy - v[3 * other + 1],
                        vz - v[3 * other + 2], inv_r, f, fp, fpp, t, unused);
            sx += (double)t.x; sy += (double)t.y; sz += (double)t.z; sq += (double)t.w;
        }
    }
    sx = group16_sum(sx); sy = group16_sum(sy); sz = group16_sum(sz); sq = group16_sum(sq);
    if (live && sub == 0) {
        grad_pos[3 * atom] = (float)sx; grad_pos[3 * atom + 1] = (float)sy; grad_pos[3 * atom + 2] = (float)sz;
        grad_charge[atom] = (float)sq;
    }
}

int pair_blocks(long long num_pairs) { return (int)std::min<long long>(std::max<long long>(1, (num_pairs + kBlock - 1) / kBlock), 256 * 16); }

}  // namespace

extern "C" {

int64_t nnpops_pme_direct_double_backward_workspace_bytes(int64_t num_pairs, int num_atoms) {
    if (num_pairs < 0 || num_atoms < 0) return 0;
    return (int64_t)(2 * (((size_t)num_pairs * 16 + 255) & ~(size_t)255) + 512);
}

int nnpops_pme_direct_double_backward(int num_atoms, int64_t num_pairs, int max_exclusions, const float* positions, const float* charges,
                                      const int32_t* neighbors, const float* deltas, const float* distances, const int32_t* exclusions,
                                      const int32_t* index, const int32_t* first_index, const float* v, const float* w, float alpha,
                                      float coulomb, float* grad_positions, float* grad_charges, void* workspace, void* stream) {
    NNPOPS_REQUIRE(num_atoms > 0 && num_pairs >= 0 && max_exclusions >= 0, "bad sizes (atoms %d, pairs %lld, exclusions %d)", num_atoms,
                   (long long)num_pairs, max_exclusions);
    NNPOPS_REQUIRE(alpha > 0 && coulomb > 0, "alpha and coulomb must be positive");
    NNPOPS_REQUIRE(positions && charges && v && w && grad_positions && grad_charges && workspace && index, "NULL device pointer");
    NNPOPS_REQUIRE(num_pairs == 0 || (neighbors && deltas && distances), "NULL pair-list pointer");
    NNPOPS_REQUIRE(max_exclusions == 0 || exclusions, "NULL exclusions pointer");
    hipStream_t s = (hipStream_t)stream;
    uintptr_t p = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    auto take = [&](size_t bytes) { const uintptr_t at = p; p += (bytes + 255) & ~(size_t)255; return at; };
    float4* first = (float4*)take((size_t)num_pairs * 16);
    float4* second = (float4*)take((size_t)num_pairs * 16);
    // (the layout nnpops_neighbor_pairs_build_index writes: slots by column | row segments | column segments)
    const int2* row_seg = (const int2*)(index + ((num_pairs + 1) & ~1ll));
    const int2* col_seg = row_seg + num_atoms;
    const int2* first_seg = first_index ? (const int2*)(first_index + ((num_pairs + 1) & ~1ll)) + num_atoms : row_seg;
    hipLaunchKernelGGL(pme_direct_double_terms, dim3(pair_blocks(num_pairs)), dim3(kBlock), 0, s, (long long)num_pairs, num_atoms,
                       max_exclusions, neighbors, neighbors + num_pairs, deltas, distances, charges, exclusions, v, w, alpha, coulomb, first,
                       second);
    hipLaunchKernelGGL(pme_direct_double_gather, dim3(div_up((long long)num_atoms * 16, kBlock)), dim3(kBlock), 0, s, num_atoms,
                       max_exclusions, positions, charges, exclusions, v, w, alpha, coulomb, first_seg, first_index, col_seg, index,
                       (const float4*)first, (const float4*)second, grad_positions, grad_charges);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // extern "C"
