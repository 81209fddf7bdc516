// mlp_weight_grad.h -- gradients of the fused atomic networks with respect to their eight parameter arrays (C ABI:
// nnpops_mlp_weight_grad, nnpops_mlp_weight_grad_workspace_bytes).  Included by mlp_fused.hip in front of its forward kernel: it uses that file's
// MlpArgs, KindDesc and tile constants.
//
// For species k and member m, with c the upstream weight of (the atom's molecule, m) (nnpops_hip.h: member_weights; 1 without it):
//   d3 = c w6 CELU'(z3)            dW6 = sum c y3        db6 = sum c
//                                  dW4 = sum d3 (x) y2   db4 = sum d3
//   d2 = (W4^T d3) CELU'(z2)       dW2 = sum d2 (x) y1   db2 = sum d2
//   d1 = (W2^T d2) CELU'(z1)       dW0 = sum d1 (x) x    db0 = sum d1          (sums over the atoms of the species)
//
// Two stages, no partial sums anywhere:
//   1. the tile pass (mlp_fused.hip: mlp_forward<true, true>, the gradient pass with WG set) carries a 64-atom tile through the four layers and
//      back, as the gradient pass does, and writes what that pass throws away into the workspace, FEATURE-MAJOR in fp32: per
//      (kind, member) the rows  c d1 [h1] | c d2 [h2] | c d3 [h3] | c y3 [h3] | c [1] | y1 [h1] | y2 [h2],  each `npad` floats long
//      (the atoms of the kind rounded up to whole tiles; the columns past the kind hold c = 0).  O(atoms M widths).
//   2. the contraction index is the atom, and in that layout BOTH operands of  dW[i][j] = sum_a d[i][a] y[j][a]  are read along
//      it: mlp_weight_contract gives a wave a 16 x 64 block of one dW and walks ALL atoms of the kind in order with
//      v_mfma_f32_16x16x4_f32; the AEV rows of dW0 are gathered through rows[] / x_groups where they lie.  The bias gradients and
//      dW6, db6 are the row sums of the first five regions (mlp_weight_rowsums: one wave per row, float64, fixed butterfly).
// Every output element is the sum of one wave over the atoms in their grouped order: no atomics, no slots, the same bits every call.
//
// Why fp32 matrix instructions here and not the split-fp16 planes of the forward pass: the operand d carries the upstream weight c
// of its atom, which is the caller's and of any magnitude, and it changes from atom to atom inside the contraction, so it cannot be
// folded in behind the product the way mlp_input_grad<true> folds a member's weight.  hi + 2^-11 lo is an exact split only inside
// fp16's range; fp32 operands need no range at all, their products are exact in the instruction and the accumulation is fp32 as
// everywhere else.  The instruction has an eighth of the f16 rate; the work is (widths^2 + h1 F) per atom and member, a third more
// than the forward pass.
//
// A member whose weight is zero for every molecule (mlp_weight_live) is skipped by both stages; its gradients are written as zeros.
#pragma once
// (included inside the anonymous namespace of mlp_fused.hip)

struct WgKind {
    int n, first, npad;                     // atoms of the kind, position of the first one in `rows`, atoms rounded up to whole tiles
    int h1, h2, h3;
    long base;                              // floats from the start of the workspace to the kind's rows
    float *dw0, *db0, *dw2, *db2, *dw4, *db4, *dw6, *db6;
};

struct WgTile {                             // what the tile pass takes behind MlpArgs (MlpWgArgs in mlp_fused.hip: MlpArgs keeps its size)
    float* ws;
    const int* live;
    long base[NNPOPS_MLP_MAX_KINDS];        // floats from the start of the workspace to every kind's rows
};

struct WgArgs {
    int num_kinds, F, M, ldx;
    const float* x;
    const int* rows;
    const int* x_groups;
    const float* ws;
    const int* live;                        // [M]: 0 for a member whose weight is zero in every molecule
    WgKind kinds[NNPOPS_MLP_MAX_KINDS];
};

// rows of a (kind, member) in the workspace
__host__ __device__ __forceinline__ int wg_rows(int h1, int h2, int h3) { return 2 * (h1 + h2 + h3) + 1; }
__host__ __device__ __forceinline__ int wg_row_d1() { return 0; }
__host__ __device__ __forceinline__ int wg_row_d2(int h1) { return h1; }
__host__ __device__ __forceinline__ int wg_row_d3(int h1, int h2) { return h1 + h2; }
__host__ __device__ __forceinline__ int wg_row_cy3(int h1, int h2, int h3) { return h1 + h2 + h3; }
__host__ __device__ __forceinline__ int wg_row_c(int h1, int h2, int h3) { return h1 + h2 + 2 * h3; }
__host__ __device__ __forceinline__ int wg_row_y1(int h1, int h2, int h3) { return h1 + h2 + 2 * h3 + 1; }
__host__ __device__ __forceinline__ int wg_row_y2(int h1, int h2, int h3) { return 2 * h1 + h2 + 2 * h3 + 1; }

__global__ __launch_bounds__(256) void mlp_weight_live(const float* __restrict__ weights, int ldw, int molecules, int M, int* __restrict__ live) {
    for (int m = threadIdx.x; m < M; m += 256) {
        int any = weights ? 0 : 1;
        if (weights)
            for (int b = 0; b < molecules; b++) any |= weights[(size_t)b * ldw + m] != 0.0f ? 1 : 0;
        live[m] = any;
    }
}

// P = 0: dW0 [h1][F] = (c d1) x^T,  1: dW2 [h2][h1] = (c d2) y1^T,  2: dW4 [h3][h2] = (c d3) y2^T.
// grid (64 x 64 blocks of the widest kind's matrix, member, kind); wave w owns rows 16 w .. 16 w + 15 of the block, four column blocks.
// Lane (i = lane % 16, kg = lane / 16) holds atoms 16 s + 4 kg .. + 3 of row i of either operand (one 16-byte load along the atoms) and
// feeds them to four instructions in turn: which atom meets which K slot does not matter as long as both operands agree.
template <int P>
__global__ __launch_bounds__(256) void mlp_weight_contract(const WgArgs g) {
    const WgKind& kd = g.kinds[blockIdx.z];
    const int m = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int h1 = kd.h1, h2 = kd.h2, h3 = kd.h3;
    const int rows_a = P == 0 ? h1 : P == 1 ? h2 : h3, cols_b = P == 0 ? g.F : P == 1 ? h1 : h2;
    const int tj = (cols_b + 63) >> 6, ti = (rows_a + 63) >> 6;
    if ((int)blockIdx.x >= ti * tj) return;
    const int i0 = ((int)blockIdx.x / tj) * 64 + w * 16, j0 = ((int)blockIdx.x % tj) * 64;
    if (i0 >= rows_a) return;                               // (widths are multiples of 32: a wave has all of its 16 rows or none)
    const int idx = lane & 15, kg = lane >> 4;
    const size_t npad = (size_t)kd.npad;
    const float* base = g.ws + kd.base + (size_t)m * wg_rows(h1, h2, h3) * npad;
    const int row_a = P == 0 ? wg_row_d1() : P == 1 ? wg_row_d2(h1) : wg_row_d3(h1, h2);
    const int row_b = P == 2 ? wg_row_y2(h1, h2, h3) : wg_row_y1(h1, h2, h3);
    const float* pa = base + (size_t)(row_a + i0 + idx) * npad + 4 * kg;
    const float* pb[4];
    int xcol[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++) {
        const int j = min(j0 + cb * 16 + idx, cols_b - 1);   // (columns past the matrix re-read its last one and are not stored)
        pb[cb] = base + (size_t)(row_b + j) * npad + 4 * kg;
        xcol[cb] = g.x_groups ? 16 * g.x_groups[j >> 4] + (j & 15) : j;
    }
    f32x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = g.live[m] ? kd.npad >> 4 : 0;          // (a skipped member's rows were never written)
    for (int s = 0; s < steps; s++) {
        const float4 a4 = *reinterpret_cast<const float4*>(pa + 16 * s);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        float b[4][4];
        if constexpr (P == 0) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int atom = 16 * s + 4 * kg + t;
                const bool in = atom < kd.n;
                const float* xr = g.x + (size_t)g.rows[kd.first + min(atom, kd.n - 1)] * g.ldx;
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    const float v = xr[xcol[cb]];
                    b[cb][t] = in ? v : 0.0f;
                }
            }
        } else {
#pragma unroll
            for (int cb = 0; cb < 4; cb++) {
                const float4 v = *reinterpret_cast<const float4*>(pb[cb] + 16 * s);
                b[cb][0] = v.x; b[cb][1] = v.y; b[cb][2] = v.z; b[cb][3] = v.w;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int cb = 0; cb < 4; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[cb][t], acc[cb], 0, 0, 0);
    }
    float* out = P == 0 ? kd.dw0 + (size_t)m * h1 * g.F : P == 1 ? kd.dw2 + (size_t)m * h2 * h1 : kd.dw4 + (size_t)m * h3 * h2;
#pragma unroll
    for (int cb = 0; cb < 4; cb++) {
        const int col = j0 + cb * 16 + idx;
        if (col >= cols_b) continue;
#pragma unroll
        for (int q = 0; q < 4; q++) out[(size_t)(i0 + 4 * kg + q) * cols_b + col] = acc[cb][q];
    }
}

// db0, db2, db4, dW6, db6: the sums over the atoms of the first h1 + h2 + 2 h3 + 1 rows of a (kind, member).  One wave per row: lane l adds
// the atoms l, l + 64, ... in float64 and the lane sums meet in a fixed butterfly.  grid (rows / 4 of the widest kind, member, kind).
__global__ __launch_bounds__(256) void mlp_weight_rowsums(const WgArgs g) {
    const WgKind& kd = g.kinds[blockIdx.z];
    const int m = blockIdx.y, lane = threadIdx.x & 63;
    const int h1 = kd.h1, h2 = kd.h2, h3 = kd.h3;
    const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row > wg_row_c(h1, h2, h3)) return;
    const float* p = g.ws + kd.base + ((size_t)m * wg_rows(h1, h2, h3) + row) * (size_t)kd.npad;
    double acc = 0.0;
    if (g.live[m])
        for (int a = lane; a < kd.n; a += 64) acc += (double)p[a];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane != 0) return;
    const float v = (float)acc;
    if (row < wg_row_d2(h1)) kd.db0[(size_t)m * h1 + row] = v;
    else if (row < wg_row_d3(h1, h2)) kd.db2[(size_t)m * h2 + row - wg_row_d2(h1)] = v;
    else if (row < wg_row_cy3(h1, h2, h3)) kd.db4[(size_t)m * h3 + row - wg_row_d3(h1, h2)] = v;
    else if (row < wg_row_c(h1, h2, h3)) kd.dw6[(size_t)m * h3 + row - wg_row_cy3(h1, h2, h3)] = v;
    else kd.db6[m] = v;
}

constexpr int kWgLiveFloats = 64;           // the head of the workspace: the members' live flags, in blocks of 64

int64_t wg_workspace_floats(const nnpops_mlp_frame* fr) {
    int64_t total = (int64_t)((fr->num_members + kWgLiveFloats - 1) / kWgLiveFloats) * kWgLiveFloats;
    for (int k = 0; k < fr->num_kinds; k++) {
        const nnpops_mlp_kind& s = fr->kinds[k];
        const int64_t npad = (int64_t)((s.num_atoms + kTile - 1) / kTile) * kTile;
        total += (int64_t)fr->num_members * wg_rows(s.h1, s.h2, s.h3) * npad;
    }
    return total;
}
