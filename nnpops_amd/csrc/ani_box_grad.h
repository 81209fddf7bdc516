// ani_box_grad.h -- box-vector gradient (virial) of the AEV: one pass over what backprop() leaves behind.
//
// Every displacement the AEV uses is d = x_j - x_i + n B (B: rows = box vectors, n in Z^3 the minimum-image shift the builder chose,
// held fixed), so with L = sum g_radial radial + sum g_angular angular
//     dL/dB[k][c] = sum over every use of a displacement of  n_k (dL/dd)_c
// -- the radial pairs and the angular legs of every centre.  One wave per atom, walking the atom's row as the radial backward does
// (rows and counts by POSITION of that walk, `order` gives the atom), a lane per neighbour:
//   * radial: a pair {i, j} is used twice, as d_ij by the radial AEV of i and as d_ji = -d_ij (shift -n) by that of j.  The wave of
//     i adds the FIRST use only: (dL/dd_ij)_own = sum_k g[i][species j][k] dR_k/dr d / r, its own gradient row, no gather; the wave
//     of j adds the other from its side.  Every directed use exactly once, as the forward counted it.
//   * angular: leg s of centre a has displacement recA[a][s], partner ids[a][s] and force leg_force[a][s] = dL_a/dd (the reaction on
//     the centre is minus the sum of its legs and moves no displacement of its own).  When the last backprop() stored the leg forces
//     in the RECEIVING atoms' rows (scatter, ani_angular_bwd.h), leg_force[a][s] is the force on a from the triples centred on
//     ids[a][s]: it belongs to the displacement -recA[a][s] of that centre, whose shift is -n.  Same walk, opposite sign.
// n is RECOVERED (box_grad.h: image_shift) from the positions, the stored displacement and the box -- exact whatever rounding the
// builder's minimum image took, whether or not the cell grid wrapped the atoms -- and a pair with n = 0, which is most of them,
// costs nothing more.  Products and sums in float64; the 9 sums of a workgroup by box_block_sum9, the workgroups by pairs_box_finish:
// the number of partial sums is a function of the number of atoms alone, no atomics, two calls agree bit for bit.
#pragma once

#include "ani_kernels.h"
#include "box_grad.h"

namespace nnpops {

constexpr int kAniBoxWaves = kBoxThreads / 64;      // atoms in flight per workgroup

inline int ani_box_blocks(int num_atoms) { return std::max(1, std::min(div_up(num_atoms, kAniBoxWaves), kBoxMaxBlocks)); }

// What one wave adds for the atom at position w of the walk (atom i): the radial uses of its row, then its angular legs.
__device__ __forceinline__ void ani_box_atom(const AniParams* __restrict__ P, const float* __restrict__ pos, const float* __restrict__ box,
                                             const float4* __restrict__ nbr, int cap, int capA, const int* __restrict__ cnt_pos,
                                             const float* __restrict__ radial_grad, int ld_radial, const float4* __restrict__ recA,
                                             const int* __restrict__ ids, const float4* __restrict__ leg_force, int scattered, int w, int i,
                                             double (&acc)[9]) {
    const int lane = lane_id();
    const int N = P->N, S = P->S, nR = P->nR;
    const float inv_rcr = P->inv_rcr, scale = P->radial_scale;
    const double leg_sign = scattered ? -1.0 : 1.0;
    int raw_a, raw_ro, my_species, na, nro;
    unpack_cnt_pos(cnt_pos[w], raw_a, raw_ro, my_species);
    clamp_counts(raw_a, raw_ro, cap, capA, na, nro);   // (an overflowed frame stays in bounds and is incomplete, as its forces are)
    const int total = na + nro;
    const float4* row = nbr + (size_t)w * cap;
    const float* gi = radial_grad + (size_t)i * ld_radial;
    for (int e = lane; e < total; e += 64) {            // radial: this atom's use of every pair of its row
        const float4 rec = row[e];
        const int word = __float_as_int(rec.w), j = word & kIdMask, sp = word >> kTagShift;
        if (j >= N || (unsigned)sp >= (unsigned)S) continue;
        float n[3];
        image_shift(pos, i, j, -rec.x, -rec.y, -rec.z, box, n);
        if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) continue;
        const float r = fast_sqrt(rec.x * rec.x + rec.y * rec.y + rec.z * rec.z);
        float sn, cs;
        sincospi_unit(r * inv_rcr, sn, cs);
        const float fc2 = -cs - 1.0f, dfc = -(0.5f * kPi * inv_rcr) * sn;       // fc2 = -2 fc
        const float* g = gi + sp * nR;
        float s = 0.f;
        for (int k = 0; k < nR; k++) {
            const float sh = r - P->rad_rs[k];
            const float ex = fast_exp2(P->rad_c[k] * sh * sh);
            s = fmaf(g[k], fmaf(fc2 * sh, P->rad_eta[k], dfc) * ex, s);
        }
        s *= scale * fast_rcp(r);
        const double G[3] = {(double)(s * rec.x), (double)(s * rec.y), (double)(s * rec.z)};
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int q = 0; q < 3; q++) acc[3 * a + q] += (double)n[a] * G[q];
    }
    if (scattered || na >= 2) {                         // angular legs (parked: a centre with a lone leg has no triples and no forces)
        const float4* ra = recA + (size_t)i * capA;
        const int* id = ids + (size_t)i * capA;
        const float4* lf = leg_force + (size_t)i * capA;
        for (int e = lane; e < na; e += 64) {
            const int j = id[e];
            if ((unsigned)j >= (unsigned)N) continue;
            const float4 rec = ra[e];
            float n[3];
            image_shift(pos, i, j, -rec.x, -rec.y, -rec.z, box, n);
            if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) continue;
            const float4 f = lf[e];
            const double F[3] = {leg_sign * (double)f.x, leg_sign * (double)f.y, leg_sign * (double)f.z};
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int q = 0; q < 3; q++) acc[3 * a + q] += (double)n[a] * F[q];
        }
    }
}

__global__ __launch_bounds__(kBoxThreads) void ani_box_partials(
    const AniParams* __restrict__ P, const float* __restrict__ pos, const float* __restrict__ box, const float4* __restrict__ nbr, int cap,
    int capA, const int* __restrict__ cnt_pos, const float* __restrict__ radial_grad, int ld_radial, const float4* __restrict__ recA,
    const int* __restrict__ ids, const float4* __restrict__ leg_force,
    const int* __restrict__ order,     // atoms in cell order, or NULL
    int scattered,                     // the leg forces sit in the receivers' rows
    double* __restrict__ partials) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    const int N = P->N;
    for (int w = blockIdx.x * kAniBoxWaves + wave_in_group(); w < N; w += gridDim.x * kAniBoxWaves) {
        int i = order ? order[w] : w;
        if ((unsigned)i >= (unsigned)N) i = w;              // (a void grid build leaves no valid order: stay in bounds)
        ani_box_atom(P, pos, box, nbr, cap, capA, cnt_pos, radial_grad, ld_radial, recA, ids, leg_force, scattered, w, i, acc);
    }
    box_block_sum9(acc, partials + (size_t)blockIdx.x * 9);
}

// Periodic batches (nnpops_ani_set_molecules on a periodic handle): the same pass with one box and one sum per molecule.  A molecule
// of n atoms is dealt to ani_box_molecule_blocks(n) workgroups -- a function of n alone -- whose waves stride over its atoms
// [offsets[m], offsets[m + 1]) in index order (batches never use the cell order), every shift recovered against box m; workgroup k of
// the molecule leaves its nine float64 sums at partials[first_block[m] + k], and ani_box_finish_molecules, one workgroup per molecule,
// adds them in the order of pairs_box_finish and writes box_deriv[m].  No atomics; the order of every sum depends on the molecule's
// atom count alone, so two calls agree bit for bit and a molecule's nine entries do not depend on its companions.  `blocks` (one
// {molecule, k} per workgroup), `first_block` and the partial sums belong to the handle (sized by nnpops_ani_set_molecules).
// (One workgroup per molecule, which needs neither table nor second launch, was measured first: its four waves walk a 192-atom frame
//  in 48 rounds, ~185 us whatever the batch -- 8 frames 212 us for compute + backprop_box against 29 us without the box gradient.)
constexpr int kAniBoxMoleculeBlocks = 64;

__host__ __device__ inline int ani_box_molecule_blocks(int num_atoms) {
    const int want = (num_atoms + kAniBoxWaves - 1) / kAniBoxWaves;
    return want < 1 ? 1 : want > kAniBoxMoleculeBlocks ? kAniBoxMoleculeBlocks : want;
}

__global__ __launch_bounds__(kBoxThreads) void ani_box_partials_molecules(
    const AniParams* __restrict__ P, const float* __restrict__ pos, const float* __restrict__ boxes, const int* __restrict__ offsets,
    const int2* __restrict__ blocks, const float4* __restrict__ nbr, int cap, int capA, const int* __restrict__ cnt_pos,
    const float* __restrict__ radial_grad, int ld_radial, const float4* __restrict__ recA, const int* __restrict__ ids,
    const float4* __restrict__ leg_force, int scattered, double* __restrict__ partials) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    const int2 mine = blocks[blockIdx.x];
    const int m = mine.x;
    const int lo = max(offsets[m], 0), hi = min(offsets[m + 1], P->N);
    const int stride = ani_box_molecule_blocks(hi - lo) * kAniBoxWaves;
    const float* box = boxes + 9 * (size_t)m;
    for (int i = lo + mine.y * kAniBoxWaves + wave_in_group(); i < hi; i += stride)
        ani_box_atom(P, pos, box, nbr, cap, capA, cnt_pos, radial_grad, ld_radial, recA, ids, leg_force, scattered, i, i, acc);
    box_block_sum9(acc, partials + (size_t)blockIdx.x * 9);
}

// one workgroup per molecule: lane t adds up the molecule's partial sums t, t + 256, ..., then box_block_sum9 (cf. pairs_box_finish)
__global__ __launch_bounds__(kBoxThreads) void ani_box_finish_molecules(const int* __restrict__ first_block, const double* __restrict__ partials,
                                                                       float* __restrict__ box_deriv) {
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    const int m = blockIdx.x;
    for (int b = first_block[m] + threadIdx.x; b < first_block[m + 1]; b += kBoxThreads) {
#pragma unroll
        for (int q = 0; q < 9; q++) acc[q] += partials[(size_t)b * 9 + q];
    }
    box_block_sum9(acc, box_deriv + 9 * (size_t)m);
}

}  // namespace nnpops
