// mlp_pack_networks.h -- the packed planes of a whole ensemble from its eight parameter arrays, on the device (C ABI:
// nnpops_mlp_pack_networks, nnpops_mlp_networks_plane_halves, nnpops_mlp_networks_floats).  Included by mlp_fused.hip behind mlp_pack: it
// uses that file's fragment constants and writes the bits mlp_pack writes, matrix by matrix.
//
// What it serves: the rebuild of a trainable module's planes after an optimizer step (nnpops_amd/BatchedNN.py: _TrainableFusedNN).  The
// parameters live in the module's layout, layer{0,2,4,6}_{weights,biases} [kinds][M][out][in] zero padded to the widest species; the kernels
// of this file read them where they lie and write, in TWO launches whatever the number of kinds, members and matrices:
//   1. mlp_pack_networks -- every fragment of every plane (a wave per fragment: 64 lanes x 8 halves x 2 planes = 2 KiB, each lane two
//      16-byte stores), both sets (all columns | the live column blocks), and the fp32 side arrays b0 | b2 | b4 | w6 | b6.  The same launch
//      clears the status block.
//   2. mlp_networks_status -- what the host decides from (nnpops_hip.h: the status block): per (kind, layer) the last row that is used, the
//      nine scalars of the activation bound and a flag for values that are not finite.
// The job table is small enough to travel in the kernel arguments: per (set, kind, group of matrices) the first fragment and the place in
// the output; a wave finds its group by bisection, the matrix, row block and K step by division.
//
// Reads: a lane of a natural-order fragment reads 8 consecutive floats of its row, of a permuted one two runs of 4 (float4 where the rows
// are 16-byte aligned), so the 4 lanes that share a row cover 128 consecutive bytes; a lane of a TRANSPOSED fragment reads down a column,
// the 16 lanes that share a K index cover 64 consecutive bytes, and the four waves of a workgroup take neighbouring row blocks of the
// same K step -- the other halves of the same lines.
//
// Determinism: the planes are a function of single elements.  The abs-sums of the status block are formed in float64 in a fixed order
// (lane l adds the elements l, l + 64, ... and the lanes meet in a butterfly) and meet the block through integer maxima -- nonnegative
// doubles order as their bits do --, so the block does not depend on the launch either.
#pragma once
// (included inside the anonymous namespace of mlp_fused.hip)

constexpr int kPkGroups = 7;                // w0 | w2 | w4 | w4t | w2t | w0t | w0tm (the last one only over at most 256 live columns)
constexpr int kPkSlots = 2 * NNPOPS_MLP_MAX_KINDS * kPkGroups;       // (set, kind, group)
constexpr int kPkStatusWords = NNPOPS_MLP_PACK_STATUS_BYTES / 4;
constexpr int kPkNonFinite = 3 * NNPOPS_MLP_MAX_KINDS;              // word of the flag; the scalars follow from byte 104
constexpr int kPkScalars = 26;                                       // first word of the nine doubles

struct PkArgs {
    int kinds, M, F, Fl;                    // Fl: live columns, 0 without live blocks
    int o0, o2, i2, o4, i4, o6, i6;         // w0 [kinds][M][o0][F]  w2 [..][o2][i2]  w4 [..][o4][i4]  w6 [..][o6][i6]
    int vec;                                // bit 0 / 1 / 2: the rows of w0 / w2 / w4 are 16-byte aligned
    const float *w0, *b0, *w2, *b2, *w4, *b4, *w6, *b6;
    const int* blocks;                      // the live 16-column blocks (device)
    _Float16 *planes, *live;
    float* floats;
    int* status;
    int frag_blocks;                        // workgroups of fragment work; the ones behind them write the floats
    int h[NNPOPS_MLP_MAX_KINDS][3];
    int float0[NNPOPS_MLP_MAX_KINDS + 1];   // first float of every kind
    int frag0[kPkSlots + 1];                // first fragment of every slot
    long out[kPkSlots];                     // halves in front of the slot in its set's buffer
};

// the shape of a descriptor: checked, and laid out -- fragments, places, floats.  No pointer is read here (the size queries take it too).
int pk_plan(const nnpops_mlp_networks* n, PkArgs& g, int64_t halves[2]) {
    NNPOPS_REQUIRE(n != nullptr, "NULL network descriptor");
    NNPOPS_REQUIRE(n->num_kinds >= 1 && n->num_kinds <= NNPOPS_MLP_MAX_KINDS, "1..%d kinds (got %d)", NNPOPS_MLP_MAX_KINDS, n->num_kinds);
    NNPOPS_REQUIRE(n->num_members >= 1 && n->num_members <= 128, "1..128 ensemble members (got %d)", n->num_members);
    NNPOPS_REQUIRE(n->num_features > 0 && n->num_features % 8 == 0 && n->num_features <= 1024,
                   "the input width must be a positive multiple of 8, at most 1024 (got %d)", n->num_features);
    NNPOPS_REQUIRE(n->out0 >= 1 && n->out2 >= 1 && n->in2 >= 1 && n->out4 >= 1 && n->in4 >= 1 && n->out6 >= 1 && n->in6 >= 1,
                   "empty parameter array");
    NNPOPS_REQUIRE(n->num_live_blocks >= 0 && (n->num_live_blocks == 0 || n->num_features % 16 == 0) && n->num_live_blocks <= n->num_features / 16,
                   "live blocks are 16-column blocks of the input: at most %d of them (got %d)", n->num_features / 16, n->num_live_blocks);
    g.kinds = n->num_kinds; g.M = n->num_members; g.F = n->num_features; g.Fl = 16 * n->num_live_blocks;
    g.o0 = n->out0; g.o2 = n->out2; g.i2 = n->in2; g.o4 = n->out4; g.i4 = n->in4; g.o6 = n->out6; g.i6 = n->in6;
    for (int k = 0; k < g.kinds; k++)
        for (int l = 0; l < 3; l++) {
            const int h = n->widths[3 * k + l];
            NNPOPS_REQUIRE(h >= 32 && h <= 256 && h % 32 == 0, "packed layer widths must be multiples of 32 in 32..256 (got %d)", h);
            g.h[k][l] = h;
        }
    int frag = 0, fl = 0;
    for (int set = 0; set < 2; set++) {
        const int Fx = set ? g.Fl : g.F;
        int64_t place = 0;
        for (int k = 0; k < NNPOPS_MLP_MAX_KINDS; k++) {
            for (int grp = 0; grp < kPkGroups; grp++) {
                const int slot = (set * NNPOPS_MLP_MAX_KINDS + k) * kPkGroups + grp;
                g.frag0[slot] = frag; g.out[slot] = (long)place;
                if (k >= g.kinds || Fx == 0 || (grp == 6 && (set == 0 || Fx > 256))) continue;
                const int h1 = g.h[k][0], h2 = g.h[k][1], h3 = g.h[k][2];
                const int R = grp == 0 ? h1 : grp == 1 ? h2 : grp == 2 ? h3 : grp == 3 ? h2 : grp == 4 ? h1 : Fx;
                const int C = grp == 0 ? Fx : grp == 1 ? h1 : grp == 2 ? h2 : grp == 3 ? h3 : grp == 4 ? h2 : grp == 5 ? g.M * h1 : h1;
                const int count = ((R + 15) / 16) * ((C + 31) / 32) * (grp == 5 ? 1 : g.M);
                frag += count; place += (int64_t)count * 2 * kFrag;
            }
        }
        halves[set] = place;
    }
    g.frag0[kPkSlots] = frag;
    g.frag_blocks = (frag + 3) / 4;
    for (int k = 0; k <= NNPOPS_MLP_MAX_KINDS; k++) {
        g.float0[k] = fl;
        if (k < g.kinds) fl += g.M * (g.h[k][0] + g.h[k][1] + 2 * g.h[k][2] + 1);
    }
    return NNPOPS_OK;
}

__device__ __forceinline__ void pk_split8(const float (&v)[8], f16x8& h, f16x8& l) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const _Float16 hh = (_Float16)v[i];
        h[i] = hh;
        l[i] = (_Float16)((v[i] - (float)hh) * kLoScale);
    }
}

__global__ __launch_bounds__(256) void mlp_pack_networks(const PkArgs g) {
    if (blockIdx.x == 0 && threadIdx.x < kPkStatusWords) g.status[threadIdx.x] = 0;
    if ((int)blockIdx.x >= g.frag_blocks) {                  // ---- the floats: b0 | b2 | b4 | w6 | b6 of every kind at its widths
        const int e = ((int)blockIdx.x - g.frag_blocks) * 256 + (int)threadIdx.x;
        if (e >= g.float0[g.kinds]) return;
        int kind = 0;
#pragma unroll
        for (int i = 1; i < NNPOPS_MLP_MAX_KINDS; i++)
            if (i < g.kinds && e >= g.float0[i]) kind = i;
        const int h1 = g.h[kind][0], h2 = g.h[kind][1], h3 = g.h[kind][2], M = g.M;
        int j = e - g.float0[kind];
        const size_t km = (size_t)kind * M;
        float v = 0.f;
        if (j < M * h1) { const int m = j / h1, r = j % h1; if (r < g.o0) v = g.b0[(km + m) * g.o0 + r]; }
        else if ((j -= M * h1) < M * h2) { const int m = j / h2, r = j % h2; if (r < g.o2) v = g.b2[(km + m) * g.o2 + r]; }
        else if ((j -= M * h2) < M * h3) { const int m = j / h3, r = j % h3; if (r < g.o4) v = g.b4[(km + m) * g.o4 + r]; }
        else if ((j -= M * h3) < M * h3) { const int m = j / h3, c = j % h3; if (c < g.i6) v = g.w6[(km + m) * g.o6 * g.i6 + c]; }
        else { j -= M * h3; v = g.b6[(km + j) * g.o6]; }
        g.floats[e] = v;
        return;
    }
    // ---- one fragment per wave
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (t >= g.frag0[kPkSlots]) return;
    int lo = 0, hi = kPkSlots;
    while (hi - lo > 1) {                                    // the last slot that starts at or before t (empty slots start where the next one does)
        const int mid = (lo + hi) >> 1;
        if (g.frag0[mid] <= t) lo = mid; else hi = mid;
    }
    const int slot = lo, set = slot / (NNPOPS_MLP_MAX_KINDS * kPkGroups), kind = (slot / kPkGroups) % NNPOPS_MLP_MAX_KINDS, grp = slot % kPkGroups;
    const int h1 = g.h[kind][0], h2 = g.h[kind][1], h3 = g.h[kind][2];
    const int Fx = set ? g.Fl : g.F;
    const bool transposed = grp >= 3, permute = grp != 0;
    const int R = grp == 0 ? h1 : grp == 1 ? h2 : grp == 2 ? h3 : grp == 3 ? h2 : grp == 4 ? h1 : Fx;
    const int Cm = grp == 0 ? Fx : grp == 1 ? h1 : grp == 2 ? h2 : grp == 3 ? h3 : grp == 4 ? h2 : h1;       // K of one member
    const int C = grp == 5 ? g.M * h1 : Cm;
    const int which = (grp == 0 || grp >= 5) ? 0 : (grp == 1 || grp == 4) ? 1 : 2;                           // w0 / w2 / w4
    const float* src = which == 0 ? g.w0 : which == 1 ? g.w2 : g.w4;
    const int so = which == 0 ? g.o0 : which == 1 ? g.o2 : g.o4, si = which == 0 ? g.F : which == 1 ? g.i2 : g.i4;
    const bool gather = set == 1 && which == 0;              // the columns of w0 are the live blocks'
    const int nb = (R + 15) >> 4, steps = (C + 31) >> 5, per = nb * steps;
    const int lf = t - g.frag0[slot], m = lf / per, f = lf % per;
    const int rb = transposed ? f % nb : f / steps, s = transposed ? f / nb : f % steps;
    const int sm = Cm >> 5;                                  // (group 5: K runs over the members, h1 / 32 steps each)
    const int m_src = grp == 5 ? s / sm : m, s_src = grp == 5 ? s % sm : s;
    const float* base = src + ((size_t)kind * g.M + m_src) * (size_t)so * si;
    const int r16 = lane & 15, kg = lane >> 4, row = rb * 16 + r16;
    const int last_block = (g.F >> 4) - 1;
    auto column = [&](int c) {                               // column c of the packed first layer -> column of w0 (a bad list gives wrong numbers, not a fault)
        return gather ? 16 * min(max(g.blocks[c >> 4], 0), last_block) + (c & 15) : c;
    };
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = 0.f;
    if (!transposed) {
        const int lim_b = gather ? Fx : min(C, si);
        if (row < min(R, so)) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int b0 = 32 * s_src + (permute ? 16 * q + 4 * kg : 8 * kg + 4 * q);
                if (b0 >= lim_b) continue;
                const float* p = base + (size_t)row * si + column(b0);          // (a run of 4 stays inside its 16-column block)
                if (((g.vec >> which) & 1) && b0 + 3 < lim_b) {
                    const float4 x = *reinterpret_cast<const float4*>(p);
                    v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (b0 + j < lim_b) v[4 * q + j] = p[j];
                }
            }
        }
    } else {
        const int lim_a = min(Cm, so), lim_b = which == 0 ? Fx : min(R, si);
        if (row < lim_b) {
            const float* p = base + column(row);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int a = 32 * s_src + (i < 4 ? 4 * kg + i : 16 + 4 * kg + i - 4);
                if (a < lim_a) v[i] = p[(size_t)a * si];
            }
        }
    }
    f16x8 h, l;
    pk_split8(v, h, l);
    _Float16* out = (set ? g.live : g.planes) + g.out[slot] + ((size_t)m * per + (size_t)rb * steps + s) * 2 * kFrag + lane * 8;
    *reinterpret_cast<f16x8*>(out) = h;
    *reinterpret_cast<f16x8*>(out + kFrag) = l;
}

__device__ __forceinline__ double pk_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double pk_wave_max(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ void pk_max(int* status, int scalar, double v) {      // v >= 0: doubles of one sign order as their bits
    if (v > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(status + kPkScalars) + scalar, (unsigned long long)__double_as_longlong(v));
}

// A workgroup (four waves) per task.  A: (kind, layer 0 / 2 / 4, row) -- wave w takes the members w, w + 4, ...: is the row used, its largest
// abs-sum, the largest |bias|;  B: (kind) the largest |w6|;  C: (kind, member, layer 2 / 4, 64 columns) the largest column abs-sum, wave w
// adding the rows w, w + 4, ... and the four partial sums meeting in their order.
__global__ __launch_bounds__(256) void mlp_networks_status(const PkArgs g) {
    __shared__ double red[2][4][64];
    __shared__ int flags[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int w = (int)blockIdx.x;
    const int rows_of_kind = g.o0 + g.o2 + g.o4, nA = g.kinds * rows_of_kind;
    const int cb2 = (g.i2 + 63) >> 6, cb4 = (g.i4 + 63) >> 6, nC = g.kinds * g.M * (cb2 + cb4);
    if (w < nA) {
        const int kind = w / rows_of_kind;
        int r = w % rows_of_kind;
        const int L = r < g.o0 ? 0 : r < g.o0 + g.o2 ? 1 : 2;
        r -= L == 0 ? 0 : L == 1 ? g.o0 : g.o0 + g.o2;
        const float* src = L == 0 ? g.w0 : L == 1 ? g.w2 : g.w4;
        const float* bias = L == 0 ? g.b0 : L == 1 ? g.b2 : g.b4;
        const int so = L == 0 ? g.o0 : L == 1 ? g.o2 : g.o4, si = L == 0 ? g.F : L == 1 ? g.i2 : g.i4;
        const bool vec = (g.vec >> L) & 1;
        double best = 0.0, bmax = 0.0;
        bool nz = false, nan = false, bad = false, bnz = false, bnan = false;
        for (int m = wv; m < g.M; m += 4) {
            const float* p = src + (((size_t)kind * g.M + m) * so + r) * (size_t)si;
            double acc = 0.0;
            auto take = [&](float x) {
                const float a = fabsf(x);
                acc += (double)a;
                nz |= a > 0.f; nan |= x != x; bad |= !(a <= 3.402823466e38f);
            };
            if (vec) {
                for (int c = 4 * lane; c < si; c += 256) {
                    const float4 x = *reinterpret_cast<const float4*>(p + c);
                    take(x.x); take(x.y); take(x.z); take(x.w);
                }
            } else {
                for (int c = lane; c < si; c += 64) take(p[c]);
            }
            acc = pk_wave_sum(acc);
            if (acc == acc) best = fmax(best, acc);
            const float bv = bias[((size_t)kind * g.M + m) * so + r], ba = fabsf(bv);
            bnz |= ba > 0.f; bnan |= bv != bv; bad |= !(ba <= 3.402823466e38f);
            if (ba == ba) bmax = fmax(bmax, (double)ba);
        }
        nz = __any(nz); nan = __any(nan); bad = __any(bad);
        if (lane == 0) {
            red[0][wv][0] = best; red[1][wv][0] = bmax;
            flags[wv] = (nz ? 1 : 0) | (nan ? 2 : 0) | (bad ? 4 : 0) | (bnz ? 8 : 0) | (bnan ? 16 : 0);
        }
        __syncthreads();
        if (threadIdx.x != 0) return;
        int f = 0;
        for (int i = 0; i < 4; i++) { f |= flags[i]; best = fmax(best, red[0][i][0]); bmax = fmax(bmax, red[1][i][0]); }
        if (((f & 1) && !(f & 2)) || ((f & 8) && !(f & 16))) atomicMax(g.status + 3 * kind + L, r + 1);      // (a NaN hides its row, as `amax(...) > 0` does)
        pk_max(g.status, L, best);
        pk_max(g.status, 5 + L, bmax);
        if (f & 4) atomicMax(g.status + kPkNonFinite, 1);
        return;
    }
    w -= nA;
    if (w < g.kinds) {
        const size_t n = (size_t)g.M * g.o6 * g.i6;
        const float* p = g.w6 + (size_t)w * n;
        double best = 0.0;
        bool bad = false;
        for (size_t c = threadIdx.x; c < n; c += 256) {
            const float a = fabsf(p[c]);
            bad |= !(a <= 3.402823466e38f);
            if (a == a) best = fmax(best, (double)a);
        }
        best = pk_wave_max(best); bad = __any(bad);
        if (lane != 0) return;
        pk_max(g.status, 8, best);                           // (a maximum: every wave brings its own)
        if (bad) atomicMax(g.status + kPkNonFinite, 1);
        return;
    }
    w -= g.kinds;
    if (w >= nC) return;
    {
        const int per_kind = g.M * (cb2 + cb4), kind = w / per_kind, r = w % per_kind, m = r / (cb2 + cb4), cb = r % (cb2 + cb4);
        const bool second = cb < cb2;                        // w2, else w4
        const float* src = second ? g.w2 : g.w4;
        const int so = second ? g.o2 : g.o4, si = second ? g.i2 : g.i4;
        const int col = 64 * (second ? cb : cb - cb2) + lane;
        double acc = 0.0;
        if (col < si) {
            const float* p = src + ((size_t)kind * g.M + m) * (size_t)so * si + col;
#pragma unroll 4
            for (int row = wv; row < so; row += 4) acc += (double)fabsf(p[(size_t)row * si]);
        }
        red[0][wv][lane] = acc;
        __syncthreads();
        if (wv != 0) return;
        acc = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
        if (!(acc == acc)) acc = 0.0;                        // (the flag of task A speaks for it)
        acc = pk_wave_max(acc);
        if (lane == 0) pk_max(g.status, second ? 4 : 3, acc);
    }
}

int pk_launch(hipStream_t stream, const nnpops_mlp_networks* n, void* planes, float* floats, void* live_planes, void* status) {
    PkArgs g{};
    int64_t halves[2];
    const int rc = pk_plan(n, g, halves);
    if (rc != NNPOPS_OK) return rc;
    NNPOPS_REQUIRE(n->layer0_weights && n->layer0_biases && n->layer2_weights && n->layer2_biases && n->layer4_weights && n->layer4_biases &&
                   n->layer6_weights && n->layer6_biases, "NULL parameter pointer");
    NNPOPS_REQUIRE(planes && floats && status, "NULL output pointer");
    NNPOPS_REQUIRE(g.Fl == 0 || (n->live_blocks && live_planes), "live blocks need their list and a buffer for their planes");
    NNPOPS_REQUIRE(((uintptr_t)planes % 16) == 0 && ((uintptr_t)live_planes % 16) == 0 && ((uintptr_t)status % 8) == 0 && ((uintptr_t)floats % 4) == 0,
                   "the planes must be 16-byte aligned, the status block 8-byte aligned");
    g.w0 = n->layer0_weights; g.b0 = n->layer0_biases; g.w2 = n->layer2_weights; g.b2 = n->layer2_biases;
    g.w4 = n->layer4_weights; g.b4 = n->layer4_biases; g.w6 = n->layer6_weights; g.b6 = n->layer6_biases;
    g.blocks = n->live_blocks; g.planes = (_Float16*)planes; g.live = (_Float16*)live_planes; g.floats = floats; g.status = (int*)status;
    g.vec = ((g.F % 4 == 0 && (uintptr_t)g.w0 % 16 == 0) ? 1 : 0) | ((g.i2 % 4 == 0 && (uintptr_t)g.w2 % 16 == 0) ? 2 : 0) |
            ((g.i4 % 4 == 0 && (uintptr_t)g.w4 % 16 == 0) ? 4 : 0);
    const int float_blocks = (g.float0[g.kinds] + 255) / 256;
    hipLaunchKernelGGL(mlp_pack_networks, dim3(g.frag_blocks + float_blocks), dim3(256), 0, stream, g);
    NNPOPS_HIP_TRY(hipGetLastError());
    const int tasks = g.kinds * (g.o0 + g.o2 + g.o4) + g.kinds + g.kinds * g.M * ((g.i2 + 63) / 64 + (g.i4 + 63) / 64);
    hipLaunchKernelGGL(mlp_networks_status, dim3(tasks), dim3(256), 0, stream, g);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}
