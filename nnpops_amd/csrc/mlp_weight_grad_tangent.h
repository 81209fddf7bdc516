// mlp_weight_grad_tangent.h -- the gradient, in the eight parameter arrays, of a DIRECTIONAL DERIVATIVE of the fused atomic networks
// (C ABI: nnpops_mlp_weight_grad_tangent, nnpops_mlp_weight_grad_tangent_workspace_bytes): what a loss on forces asks of the networks.
// Included by mlp_fused.hip behind check_and_fill: it uses that file's MlpArgs, KindDesc, tile helpers and descriptor check.
//
// For species k and member m, an atom with input x, tangent t (the cotangent of dE/dx: J.v of the AEV) and upstream weight c:
//   forward        z1 = W0 x + b0, y1 = s(z1), ...          tangent   z'1 = W0 t, y'1 = s'(z1) z'1, z'2 = W2 y'1, ...   E' = w6 . y'3
//   first backward d3 = w6 s'(z3), d2 = (W4^T d3) s'(z2), d1 = (W2^T d2) s'(z1)
//   second         e3 = w6 s''(z3) z'3
//                  e2 = s'(z2) W4^T e3 + s''(z2) z'2 W4^T d3
//                  e1 = s'(z1) W2^T e2 + s''(z1) z'1 W2^T d2
//   dW6 = sum c y'3                                 db6 = 0
//   dW4 = sum c (d3 (x) y'2 + e3 (x) y2)            db4 = sum c e3
//   dW2 = sum c (d2 (x) y'1 + e2 (x) y1)            db2 = sum c e2
//   dW0 = sum c (d1 (x) t   + e1 (x) x )            db0 = sum c e1           (s = CELU; s'' = s' / alpha for z <= 0, 0 above)
//
// Two stages, as in mlp_weight_grad.h, no partial sums anywhere:
//   1. mlp_tangent_tile carries 32 atoms of one species and one member through the four layers and back.  The forward kernel's tile is four
//      16-column blocks: blocks 0-1 hold the VALUES of the 32 atoms (x -> y1 -> y2 -> y3), blocks 2-3 the TANGENTS of the same atoms
//      (t -> y'1 -> y'2 -> y'3), so the products W0, W2, W4 act on both at once.  In the accumulator layout an atom's value and its
//      tangent sit in the same lane in different accumulators: y' = s'(z) z' and the s'' terms are lane-local.  On the way back the 64
//      columns are [d | e] and W4^T, W2^T act on both halves in one product.  Everything is linear in c and in t, so d and e travel
//      unweighted and the weights are applied where the rows are stored.
//   2. the workspace holds, per (kind, member) and FEATURE-MAJOR in fp32, rows 2 npad long (npad: the atoms of the kind rounded up to whole
//      tiles of 32):   c d_l || c e_l  (l = 1, 2, 3)   and   y'_l || y_l  (l = 1, 2),   and behind them rows npad long with c y'3.
//      Every matrix gradient is ONE contraction over the doubled row (mlp_tangent_contract: v_mfma_f32_16x16x4_f32, the body of
//      mlp_weight_contract; dW0 streams t against c d1, then x against c e1, both gathered through rows[] / x_groups); the bias
//      gradients are the row sums of the e halves, dW6 those of c y'3 (mlp_tangent_rowsums: float64, fixed butterfly).
//
// The range of t.  The tangent is the caller's and of any magnitude; the split-fp16 planes of the tile pass are exact only inside fp16's
// range.  Every tangent quantity is linear in t, so the tile pass multiplies an atom's row of t by a power of two that brings its largest
// entry into [1/2, 1) -- exact -- and the inverse power multiplies the atom's y' and e columns (and E') back where they are stored.  The
// alternative, W0 t on fp32 matrix instructions, would put a second kind of product and a second operand path for the weights into the
// kernel's longest loop; the normalisation costs one extra read of the row of t and two multiplications per stored value.
//
// A member whose weight is zero for every molecule is skipped by both stages and its gradients are zeros (the tile pass still visits it
// when tangent_energies is asked for: E' is unweighted).
#pragma once
// (included inside the anonymous namespace of mlp_fused.hip)

constexpr int kTgAtoms = 32;                // atoms per workgroup of the tile pass: column blocks 0-1 values, 2-3 tangents

struct TgKind {
    int n, first, npad;                     // atoms of the kind, position of the first one in `rows`, atoms rounded up to whole tiles of 32
    int h1, h2, h3;
    long base;                              // floats from the start of the workspace to the kind's rows
    float *dw0, *db0, *dw2, *db2, *dw4, *db4, *dw6, *db6;
};

struct TgTile {                             // what the tile pass takes behind MlpArgs
    float* ws;
    const int* live;
    const float* t; int ldt;
    float* tangent_energies;                // optional [grouped atoms][M]
    long base[NNPOPS_MLP_MAX_KINDS];
};
struct MlpTgArgs : MlpArgs { TgTile tt; };

struct TgArgs {
    int num_kinds, F, M, ldx, ldt;
    const float *x, *t;
    const int* rows;
    const int* x_groups;
    const float* ws;
    const int* live;
    TgKind kinds[NNPOPS_MLP_MAX_KINDS];
};

// rows of a (kind, member) in the workspace, in units of DOUBLED rows (2 npad floats); c y'3 lies behind them in rows of npad floats
__host__ __device__ __forceinline__ int tg_row_a1() { return 0; }
__host__ __device__ __forceinline__ int tg_row_a2(int h1) { return h1; }
__host__ __device__ __forceinline__ int tg_row_a3(int h1, int h2) { return h1 + h2; }
__host__ __device__ __forceinline__ int tg_row_b1(int h1, int h2, int h3) { return h1 + h2 + h3; }
__host__ __device__ __forceinline__ int tg_row_b2(int h1, int h2, int h3) { return 2 * h1 + h2 + h3; }
__host__ __device__ __forceinline__ int tg_double_rows(int h1, int h2, int h3) { return 2 * h1 + 2 * h2 + h3; }
__host__ __device__ __forceinline__ int tg_floats_per_atom(int h1, int h2, int h3) { return 2 * tg_double_rows(h1, h2, h3) + h3; }

// the power of two that brings v > 0 into [1/2, 1), and its inverse (1 and 1 for v = 0, infinities and NaN)
__device__ __forceinline__ void tg_normaliser(float v, float& scale, float& inverse) {
    const int field = (int)((__float_as_uint(v) >> 23) & 0xffu);
    scale = 1.0f; inverse = 1.0f;
    if (v > 0.0f && field != 0xff) {
        const int e = min(max(field - 127, -125), 125);     // 2^e <= v < 2^(e + 1) (denormals: below 2^-125, brought as far as the format goes)
        scale = __uint_as_float((unsigned)(127 - e - 1) << 23);
        inverse = __uint_as_float((unsigned)(127 + e + 1) << 23);
    }
}

// =============================================================================================
// the tile pass: 32 atoms and their tangents through the four layers and back
// =============================================================================================
__global__ __launch_bounds__(kThreads, 2) void mlp_tangent_tile(const MlpTgArgs g) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* xstage = lds;                                     // 2 x 8 KiB: a K step of [x | t], split, fragment layout
    char* actA = lds + 2 * kStageBytes;                     // 64 KiB
    char* actB = actA + kActBytes;                          // 64 KiB
    int* xgroup = reinterpret_cast<int*>(actB + kActBytes); // 64 ints: column block of x / t behind every 16-feature block
    float* ctile = reinterpret_cast<float*>(xgroup + 64);   // 32: the upstream weight of (the molecule of the atom, m); 0 past the kind
    float* tinv = ctile + kTgAtoms;                         // 32: what brings the atom's normalised tangent back
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const KindDesc& kd = kind_of_block(g, blockIdx.x);
    const int local = blockIdx.x - kd.block0;
    const int m = local % g.M, tile = local / g.M;
    if (!g.tt.live[m] && !g.tt.tangent_energies) return;    // (a member nobody weighs: uniform over the workgroup)
    const int r0 = tile * kTgAtoms;                         // first atom of the tile inside the kind
    if (tid >= 128 && tid < 128 + kTgAtoms) {
        const int r = r0 + tid - 128;
        float c = 0.0f;
        if (r < kd.n) {
            c = 1.0f;
            if (g.member_weights)
                c = g.member_weights[(size_t)(g.w_offsets ? molecule_of_row(g.w_offsets, g.w_segments, g.rows[kd.first + r]) : 0) * g.ldw + m];
        }
        ctile[tid - 128] = c;
    }
    if (tid < 64) xgroup[tid] = 16 * tid < g.F ? (g.x_groups ? g.x_groups[tid] : tid) : 0;
    __syncthreads();
    const int kgD = lane >> 4, a16 = lane & 15;
    const float inv_alpha = 1.0f / g.alpha;

    const int nb1 = kd.h1 >> 4, nb2 = kd.h2 >> 4, nb3 = kd.h3 >> 4;
    const int s0 = (g.F + 31) >> 5, s1 = kd.h1 >> 5, s2 = kd.h2 >> 5, s3 = kd.h3 >> 5;
    const int n1 = blocks_of_wave(nb1, w), n2 = blocks_of_wave(nb2, w), n3 = blocks_of_wave(nb3, w);

    f32x4 acc1[kRB][kCB], acc2[kRB][kCB];
    f32x4 c1[kRB][kCB], c2[kRB][kCB];                      // per hidden layer: blocks 0-1 CELU'(z), blocks 2-3 CELU''(z) z' (scaled as z')
    int kidx = 0;
#pragma unroll
    for (int i = 1; i < NNPOPS_MLP_MAX_KINDS; i++)
        if (i < g.num_kinds && (int)blockIdx.x >= g.kinds[i].block0) kidx = i;
    const size_t npad = (size_t)kd.tiles * kTgAtoms;
    float* wtile = g.tt.ws + g.tt.base[kidx] + (size_t)m * tg_floats_per_atom(kd.h1, kd.h2, kd.h3) * npad + r0;
    // a pair of blocks in D layout -> the two halves of the doubled rows row0 + 16 rb + 4 g + q, columns of the atoms cb * 16 + a16
    auto emit = [&](int row0, int rb, int cb, const f32x4& first, const f32x4& second, float f_first, float f_second) {
        float* p = wtile + (size_t)(row0 + rb * 16 + kgD * 4) * (2 * npad) + cb * 16 + a16;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            p[q * 2 * npad] = first[q] * f_first;
            p[q * 2 * npad + npad] = second[q] * f_second;
        }
    };

    // ---------------- layer 0: the rows of x (threads 0..255) and of t (256..511) stream through LDS, 32 columns per step ----------------
    {
        const _Float16* wp = kd.w0 + (size_t)m * nb1 * s0 * 2 * kFrag;
        const int sa = tid >> 3, piece = tid & 7;            // column of the tile (0..31 values, 32..63 tangents), four consecutive features
        const bool tangent = sa >= kTgAtoms;
        const int srow = g.rows[kd.first + min(r0 + (sa & (kTgAtoms - 1)), kd.n - 1)];
        const float* xsrc = (tangent ? g.tt.t + (size_t)srow * g.tt.ldt : g.x + (size_t)srow * g.ldx) + min((piece & 3) * 4, g.F - 4);
        char* xdst = xstage + ((sa >> 4) * 2) * 1024 + ((sa & 15) + 16 * (piece >> 1)) * 16 + 8 * (piece & 1);
        float in_scale = g.scale;
        if (tangent) {                                       // the largest entry of the row over the live columns: eight threads per atom
            float mx = 0.0f;
            for (int s = 0; s < s0; s++) {
                if (32 * s + piece * 4 < g.F) {
                    const float4 v = *reinterpret_cast<const float4*>(xsrc + 16 * xgroup[2 * s + (piece >> 2)]);
                    mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
            float ts, ti;
            tg_normaliser(mx, ts, ti);
            in_scale *= ts;
            if (piece == 0) tinv[sa - kTgAtoms] = ti;
        }
        float4 xraw;
        float xscale;
        auto fetch_x = [&](int s) {
            const int k = 32 * s + piece * 4;
            const bool in = k < g.F;                         // (F is a multiple of 8: all four or none)
            xraw = *reinterpret_cast<const float4*>(xsrc + 16 * xgroup[in ? 2 * s + (piece >> 2) : 0]);
            xscale = in ? in_scale : 0.0f;
        };
        auto stage_x = [&](int stage) {
            // (a column past F re-reads live data times 0: 0 x finite only -- select, so that nothing behind the row can leak in)
            const f32x4 xv = {xscale != 0.0f ? xraw.x * xscale : 0.0f, xscale != 0.0f ? xraw.y * xscale : 0.0f,
                              xscale != 0.0f ? xraw.z * xscale : 0.0f, xscale != 0.0f ? xraw.w * xscale : 0.0f};
            f16x4 h, l;
            split4(xv, h, l);
            *reinterpret_cast<f16x4*>(xdst + stage * kStageBytes) = h;
            *reinterpret_cast<f16x4*>(xdst + stage * kStageBytes + 1024) = l;
        };
        zero_acc(acc1, acc2);
        AFrag a0, a1, a2, a3;
        fetch_x(0);
        load_a(a0, wp, s0, nb1, 0, w, lane);
        load_a(a1, wp, s0, nb1, min(1, s0 - 1), w, lane);
        load_a(a2, wp, s0, nb1, min(2, s0 - 1), w, lane);
        stage_x(0);
        fetch_x(min(1, s0 - 1));
        __syncthreads();
        auto step = [&](int s, const AFrag& cur, AFrag& refill) {
            load_a(refill, wp, s0, nb1, min(s + 3, s0 - 1), w, lane);
            mma_step(cur, xstage + (s & 1) * kStageBytes, n1, lane, acc1, acc2);
            stage_x((s + 1) & 1);
            fetch_x(min(s + 2, s0 - 1));
            __syncthreads();
        };
        for (int s = 0; s < s0; s += 4) {
            step(s, a0, a3);
            if (s + 1 < s0) step(s + 1, a1, a0);
            if (s + 2 < s0) step(s + 2, a2, a1);
            if (s + 3 < s0) step(s + 3, a3, a2);
        }
    }
    // Everything is kept divided by the operand scale (mlp_forward); a tangent also times its atom's normaliser.
    const float kScale = g.scale, kUnscale = g.unscale;
    const float exp_scale = kUnscale * inv_alpha * 1.44269504089f, alpha_s = g.alpha * kScale;
    float cw[2], ti[2];                                     // of this lane's two atoms (column blocks 0 and 1)
#pragma unroll
    for (int cb = 0; cb < 2; cb++) { cw[cb] = ctile[cb * 16 + a16]; ti[cb] = tinv[cb * 16 + a16]; }
    // bias + CELU on the values, CELU' on the tangents; both to the next layer's region and to the rows y' || y
    auto activate = [&](const float* __restrict__ bias, int nmine, f32x4 (&c)[kRB][kCB], char* act, int row_b) {
        for_blocks(nmine, w, [&](int j, int rb) {
            const float4 b = *reinterpret_cast<const float4*>(bias + rb * 16 + kgD * 4);
            const float bq[4] = {b.x * kScale, b.y * kScale, b.z * kScale, b.w * kScale};
#pragma unroll
            for (int cb = 0; cb < 2; cb++) {
                f32x4 y, yd;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float vs = fmaf(kLoInv, acc2[j][cb][q], acc1[j][cb][q]) + bq[q];
                    const float zd = fmaf(kLoInv, acc2[j][cb + 2][q], acc1[j][cb + 2][q]);
                    const float e = __builtin_amdgcn_exp2f(fminf(vs, 0.f) * exp_scale);       // CELU'(v) for v <= 0
                    y[q] = vs > 0.f ? vs : fmaf(alpha_s, e, -alpha_s);
                    const float sp = vs > 0.f ? 1.0f : e;
                    yd[q] = sp * zd;
                    c[j][cb][q] = sp;
                    c[j][cb + 2][q] = vs > 0.f ? 0.0f : yd[q] * inv_alpha;                    // CELU''(v) z'
                }
                put_fragment(act, rb, cb, lane, y);
                put_fragment(act, rb, cb + 2, lane, yd);
                emit(row_b, rb, cb, yd, y, kUnscale * ti[cb], kUnscale);
            }
        });
    };
    activate(kd.b0 + (size_t)m * kd.h1, n1, c1, actA, tg_row_b1(kd.h1, kd.h2, kd.h3));
    __syncthreads();
    // ---------------- layer 2 ----------------
    layer_resident(kd.w2 + (size_t)m * nb2 * s1 * 2 * kFrag, s1, nb2, n2, w, lane, actA, acc1, acc2);
    activate(kd.b2 + (size_t)m * kd.h2, n2, c2, actB, tg_row_b2(kd.h1, kd.h2, kd.h3));
    __syncthreads();
    // ---------------- layer 4, and layer 6 on the spot: E' = w6 . y'3, d3 = w6 CELU'(z3), e3 = w6 CELU''(z3) z'3 ----------------
    layer_resident(kd.w4 + (size_t)m * nb3 * s2 * 2 * kFrag, s2, nb3, n3, w, lane, actB, acc1, acc2);
    float part[2] = {0.f, 0.f};
    {
        const float* bias = kd.b4 + (size_t)m * kd.h3;
        const float* w6 = kd.w6 + (size_t)m * kd.h3;
        float* cyd = wtile + (size_t)tg_double_rows(kd.h1, kd.h2, kd.h3) * (2 * npad);
        for_blocks(n3, w, [&](int j, int rb) {
            const float4 b = *reinterpret_cast<const float4*>(bias + rb * 16 + kgD * 4);
            const float4 wl = *reinterpret_cast<const float4*>(w6 + rb * 16 + kgD * 4);
            const float bq[4] = {b.x * kScale, b.y * kScale, b.z * kScale, b.w * kScale};
            const float wr[4] = {wl.x, wl.y, wl.z, wl.w};
#pragma unroll
            for (int cb = 0; cb < 2; cb++) {
                f32x4 d, ep, yd;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float vs = fmaf(kLoInv, acc2[j][cb][q], acc1[j][cb][q]) + bq[q];
                    const float zd = fmaf(kLoInv, acc2[j][cb + 2][q], acc1[j][cb + 2][q]);
                    const float e = __builtin_amdgcn_exp2f(fminf(vs, 0.f) * exp_scale);
                    const float sp = vs > 0.f ? 1.0f : e;
                    yd[q] = sp * zd;
                    part[cb] = fmaf(wr[q] * kUnscale, yd[q], part[cb]);
                    d[q] = wr[q] * kScale * sp;                                 // d3 / scale
                    ep[q] = vs > 0.f ? 0.0f : wr[q] * (e * inv_alpha) * zd;     // e3 / scale (times the normaliser)
                }
                put_fragment(actA, rb, cb, lane, d);                            // (region A: layer 2 is done with it)
                put_fragment(actA, rb, cb + 2, lane, ep);
                emit(tg_row_a3(kd.h1, kd.h2), rb, cb, d, ep, kUnscale * cw[cb], kUnscale * cw[cb] * ti[cb]);
                float* p = cyd + (size_t)(rb * 16 + kgD * 4) * npad + cb * 16 + a16;
#pragma unroll
                for (int q = 0; q < 4; q++) p[q * npad] = yd[q] * (kUnscale * cw[cb]) * ti[cb];
            }
        });
    }
    // E' of the tile's atoms: sum over the K groups of a wave (lanes 16 apart), then over the waves
    float* red = reinterpret_cast<float*>(xstage);          // kWaves x 32 atoms (the stages are idle now)
#pragma unroll
    for (int cb = 0; cb < 2; cb++) {
        float p = part[cb];
        p += __shfl_xor(p, 16, 64);
        p += __shfl_xor(p, 32, 64);
        if (kgD == 0) red[w * kTgAtoms + cb * 16 + a16] = p;
    }
    __syncthreads();
    if (g.tt.tangent_energies && tid < kTgAtoms && r0 + tid < kd.n) {
        float e = 0.0f;
#pragma unroll
        for (int v = 0; v < kWaves; v++) e += red[v * kTgAtoms + tid];
        g.tt.tangent_energies[(size_t)(kd.first + r0 + tid) * g.M + m] = e * tinv[tid];
    }
    if (!g.tt.live[m]) return;                              // (visited for E' alone)
    // ---------------- backward: [d2 | e2] from W4^T [d3 | e3], [d1 | e1] from W2^T [d2 | e2] ----------------
    auto back = [&](int nmine, const f32x4 (&c)[kRB][kCB], char* act, int row_a) {
        for_blocks(nmine, w, [&](int j, int rb) {
#pragma unroll
            for (int cb = 0; cb < 2; cb++) {
                f32x4 d, ep;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float pd = fmaf(kLoInv, acc2[j][cb][q], acc1[j][cb][q]);            // W^T d / scale
                    const float pe = fmaf(kLoInv, acc2[j][cb + 2][q], acc1[j][cb + 2][q]);    // W^T e / scale
                    d[q] = pd * c[j][cb][q];
                    ep[q] = fmaf(c[j][cb][q], pe, c[j][cb + 2][q] * kUnscale * pd);
                }
                if (act) {
                    put_fragment(act, rb, cb, lane, d);
                    put_fragment(act, rb, cb + 2, lane, ep);
                }
                emit(row_a, rb, cb, d, ep, kUnscale * cw[cb], kUnscale * cw[cb] * ti[cb]);
            }
        });
    };
    layer_resident(kd.w4t + (size_t)m * nb2 * s3 * 2 * kFrag, s3, nb2, n2, w, lane, actA, acc1, acc2);
    back(n2, c2, actB, tg_row_a2(kd.h1));
    __syncthreads();
    layer_resident(kd.w2t + (size_t)m * nb1 * s2 * 2 * kFrag, s2, nb1, n1, w, lane, actB, acc1, acc2);
    back(n1, c1, nullptr, tg_row_a1());
}

// =============================================================================================
// the contractions over the doubled rows
// =============================================================================================
// P = 0: dW0 [h1][F] = [c d1 | c e1] [t | x]^T,  1: dW2 [h2][h1] = [c d2 | c e2] [y'1 | y1]^T,  2: dW4 [h3][h2] = [c d3 | c e3] [y'2 | y2]^T.
// Grid, wave and lane roles are mlp_weight_contract's; the walk is over 2 npad columns, first half then second, in one wave and a fixed order.
template <int P>
__global__ __launch_bounds__(256) void mlp_tangent_contract(const TgArgs g) {
    const TgKind& kd = g.kinds[blockIdx.z];
    const int m = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int h1 = kd.h1, h2 = kd.h2, h3 = kd.h3;
    const int rows_a = P == 0 ? h1 : P == 1 ? h2 : h3, cols_b = P == 0 ? g.F : P == 1 ? h1 : h2;
    const int tj = (cols_b + 63) >> 6, ti = (rows_a + 63) >> 6;
    if ((int)blockIdx.x >= ti * tj) return;
    const int i0 = ((int)blockIdx.x / tj) * 64 + w * 16, j0 = ((int)blockIdx.x % tj) * 64;
    if (i0 >= rows_a) return;                               // (widths are multiples of 32: a wave has all of its 16 rows or none)
    const int idx = lane & 15, kg = lane >> 4;
    const size_t npad = (size_t)kd.npad, ld = 2 * npad;
    const float* base = g.ws + kd.base + (size_t)m * tg_floats_per_atom(h1, h2, h3) * npad;
    const int row_a = P == 0 ? tg_row_a1() : P == 1 ? tg_row_a2(h1) : tg_row_a3(h1, h2);
    const int row_b = P == 2 ? tg_row_b2(h1, h2, h3) : tg_row_b1(h1, h2, h3);
    const float* pa = base + (size_t)(row_a + i0 + idx) * ld + 4 * kg;
    const float* pb[4];
    int xcol[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++) {
        const int j = min(j0 + cb * 16 + idx, cols_b - 1);   // (columns past the matrix re-read its last one and are not stored)
        pb[cb] = base + (size_t)(row_b + j) * ld + 4 * kg;
        xcol[cb] = g.x_groups ? 16 * g.x_groups[j >> 4] + (j & 15) : j;
    }
    f32x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; cb++) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int half = kd.npad >> 4;
    const int steps = g.live[m] ? 2 * half : 0;              // (a skipped member's rows were never written)
    for (int s = 0; s < steps; s++) {
        const float4 a4 = *reinterpret_cast<const float4*>(pa + 16 * s);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        float b[4][4];
        if constexpr (P == 0) {
            const bool second = s >= half;                   // t against c d1, then x against c e1
            const float* src = second ? g.x : g.t;
            const size_t ldsrc = second ? g.ldx : g.ldt;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int atom = 16 * (second ? s - half : s) + 4 * kg + t;
                const bool in = atom < kd.n;
                const float* xr = src + (size_t)g.rows[kd.first + min(atom, kd.n - 1)] * ldsrc;
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

// db0, db2, db4: the sums over the atoms of the e halves of the first h1 + h2 + h3 doubled rows; dW6: those of the rows c y'3; db6 = 0 (E' does
// not depend on b6).  One wave per row: lane l adds the atoms l, l + 64, ... in float64 and the lane sums meet in a fixed butterfly.
__global__ __launch_bounds__(256) void mlp_tangent_rowsums(const TgArgs g) {
    const TgKind& kd = g.kinds[blockIdx.z];
    const int m = blockIdx.y, lane = threadIdx.x & 63;
    const int h1 = kd.h1, h2 = kd.h2, h3 = kd.h3;
    const int row = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ne = h1 + h2 + h3;
    if (row > ne + h3) return;
    const size_t npad = (size_t)kd.npad;
    const float* base = g.ws + kd.base + (size_t)m * tg_floats_per_atom(h1, h2, h3) * npad;
    const float* p = row < ne ? base + (size_t)row * 2 * npad + npad : base + (size_t)tg_double_rows(h1, h2, h3) * 2 * npad + (size_t)(row - ne) * npad;
    double acc = 0.0;
    if (g.live[m] && row < ne + h3)
        for (int a = lane; a < kd.n; a += 64) acc += (double)p[a];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane != 0) return;
    const float v = (float)acc;
    if (row < h1) kd.db0[(size_t)m * h1 + row] = v;
    else if (row < h1 + h2) kd.db2[(size_t)m * h2 + row - h1] = v;
    else if (row < ne) kd.db4[(size_t)m * h3 + row - h1 - h2] = v;
    else if (row < ne + h3) kd.dw6[(size_t)m * h3 + row - ne] = v;
    else kd.db6[m] = 0.0f;
}

int64_t tg_workspace_floats(const nnpops_mlp_frame* fr) {
    int64_t total = (int64_t)((fr->num_members + kWgLiveFloats - 1) / kWgLiveFloats) * kWgLiveFloats;
    for (int k = 0; k < fr->num_kinds; k++) {
        const nnpops_mlp_kind& s = fr->kinds[k];
        const int64_t npad = (int64_t)((s.num_atoms + kTgAtoms - 1) / kTgAtoms) * kTgAtoms;
        total += (int64_t)fr->num_members * tg_floats_per_atom(s.h1, s.h2, s.h3) * npad;
    }
    return total;
}

int tg_launch(void* stream, const nnpops_mlp_frame* frame, const nnpops_mlp_weight_grad_tangent_out* out) {
    MlpTgArgs g{};
    int blocks = 0;
    int rc = check_and_fill(frame, g, true, frame ? frame->num_members : 1, &blocks);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(out != nullptr && out->workspace != nullptr && ((uintptr_t)out->workspace % 16) == 0, "the workspace must be a 16-byte aligned device pointer");
    const int64_t need = tg_workspace_floats(frame) * (int64_t)sizeof(float);
    NNPOPS_REQUIRE(out->workspace_bytes >= need, "the workspace holds %lld bytes, %lld are needed", (long long)out->workspace_bytes, (long long)need);
    NNPOPS_REQUIRE(out->t != nullptr && out->ldt >= frame->num_features && out->ldt % 4 == 0 && ((uintptr_t)out->t % 16) == 0,
                   "t rows must be 16-byte aligned and at least as wide as the features (ldt %d)", out->ldt);
    NNPOPS_REQUIRE(frame->num_members <= 65535, "at most 65535 members (got %d)", frame->num_members);
    g.dx_partial = nullptr; g.publish_to = nullptr;
    TgArgs a{};
    a.num_kinds = g.num_kinds; a.F = g.F; a.M = g.M; a.ldx = g.ldx; a.ldt = out->ldt; a.x = g.x; a.t = out->t; a.rows = g.rows; a.x_groups = g.x_groups;
    float* ws = (float*)out->workspace;
    int* live = (int*)out->workspace;
    a.ws = ws; a.live = live;
    TgTile& tt = g.tt;
    tt.ws = ws; tt.live = live; tt.t = out->t; tt.ldt = out->ldt; tt.tangent_energies = out->tangent_energies;
    long base = (long)((g.M + kWgLiveFloats - 1) / kWgLiveFloats) * kWgLiveFloats;
    int max_sum_rows = 1, max_blocks[3] = {1, 1, 1};
    blocks = 0;
    for (int k = 0; k < g.num_kinds; k++) {
        KindDesc& d = g.kinds[k];
        const nnpops_mlp_weight_grad_kind& o = out->kinds[k];
        NNPOPS_REQUIRE(o.dw0 && o.db0 && o.dw2 && o.db2 && o.dw4 && o.db4 && o.dw6 && o.db6, "NULL gradient pointer (kind %d)", k);
        d.tiles = (d.n + kTgAtoms - 1) / kTgAtoms;          // (tiles of 32 atoms here, not the forward pass's 64)
        d.block0 = blocks;
        blocks += d.tiles * g.M;
        TgKind& tk = a.kinds[k];
        tk.n = d.n; tk.first = d.first; tk.npad = d.tiles * kTgAtoms; tk.h1 = d.h1; tk.h2 = d.h2; tk.h3 = d.h3; tk.base = base;
        tk.dw0 = o.dw0; tk.db0 = o.db0; tk.dw2 = o.dw2; tk.db2 = o.db2; tk.dw4 = o.dw4; tk.db4 = o.db4; tk.dw6 = o.dw6; tk.db6 = o.db6;
        tt.base[k] = base;
        base += (long)g.M * tg_floats_per_atom(d.h1, d.h2, d.h3) * tk.npad;
        max_sum_rows = std::max(max_sum_rows, d.h1 + d.h2 + 2 * d.h3 + 1);
        max_blocks[0] = std::max(max_blocks[0], ((d.h1 + 63) / 64) * ((g.F + 63) / 64));
        max_blocks[1] = std::max(max_blocks[1], ((d.h2 + 63) / 64) * ((d.h1 + 63) / 64));
        max_blocks[2] = std::max(max_blocks[2], ((d.h3 + 63) / 64) * ((d.h2 + 63) / 64));
    }
    for (int k = g.num_kinds; k < NNPOPS_MLP_MAX_KINDS; k++) { g.kinds[k] = g.kinds[0]; a.kinds[k] = a.kinds[0]; tt.base[k] = tt.base[0]; }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mlp_weight_live, dim3(1), dim3(256), 0, s, g.member_weights, g.ldw, std::max(g.w_segments, 1), g.M, live);
    NNPOPS_HIP_TRY(hipGetLastError());
    if (blocks > 0) {
        const size_t lds = 2 * kStageBytes + 2 * kActBytes + 256 + 2 * kTgAtoms * sizeof(float);
        static bool raised[64] = {};
        int dev = 0;
        NNPOPS_HIP_TRY(hipGetDevice(&dev));
        if (dev >= 64 || !raised[dev & 63]) {
            NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)mlp_tangent_tile, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            raised[dev & 63] = true;
        }
        hipLaunchKernelGGL(mlp_tangent_tile, dim3(blocks), dim3(kThreads), lds, s, g);
        NNPOPS_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(mlp_tangent_rowsums, dim3((max_sum_rows + 3) / 4, g.M, g.num_kinds), dim3(256), 0, s, a);
    NNPOPS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mlp_tangent_contract<0>, dim3(max_blocks[0], g.M, g.num_kinds), dim3(256), 0, s, a);
    NNPOPS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mlp_tangent_contract<1>, dim3(max_blocks[1], g.M, g.num_kinds), dim3(256), 0, s, a);
    NNPOPS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mlp_tangent_contract<2>, dim3(max_blocks[2], g.M, g.num_kinds), dim3(256), 0, s, a);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}
