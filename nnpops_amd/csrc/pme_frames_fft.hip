// pme_frames_fft.hip -- the reciprocal-space middle of PME over frames in ONE launch: a frame's three-dimensional real-to-complex
// transform, the Green's-function scaling with its energy, and the inverse transform, all inside one workgroup whose LDS holds the
// frame's half-spectrum.  It stands where the library transforms stand in the default route
// (rfft, fftn, convolve, energy, ifftn, irfft and their copies): global memory is read once (the spread's real grid) and written once
// (the potential grid), plus the scaled spectrum when the box gradient asks for it.
//
//   LDS      grid [Kx][Ky][ZP] complex float32, ZP = Kz/2 + 1 rounded up to odd (a z line's stride in words is then 2 mod 4: lanes that
//            walk neighbouring z lines spread over the banks even when Kz/2 + 1 is a power of two); the real grid [Kx][Ky][Kz] is loaded
//            into the same rows (Kz reals take Kz/2 of a row's ZP complex slots).  Behind it the twiddles exp(-2 pi i t / K) of the
//            three axes (sincospi in double, rounded once), the wave sums of the energy, and the index tables.
//   1-D      mixed radix Cooley-Tukey, in place: radix 4 as long as it divides, then 2, 3, 5, 7 (2-5 written out, 7 from the twiddle
//            table).  Forward is decimation in frequency and leaves a line in digit-reversed order; the inverse is the transposed
//            conjugate, decimation in time, and takes exactly that order: no permutation pass.  nat[] maps a storage slot to its
//            natural frequency, for the convolution's (kx, ky, kz) and the natural-order store of the scaled spectrum.
//   z        Kz is even: the Kz reals of a line are Kz/2 complex numbers (even, odd) as they lie; a half-length complex transform and
//            the split pass give bins 0 .. Kz/2 (bin Kz/2 in the row's slot Kz/2); the inverse undoes the split and transforms back.
//   work     every stage deals (butterfly, line) items over the whole workgroup, lines fastest: in the x and y passes neighbouring
//            lanes hold neighbouring kz of the same butterfly (consecutive words), in the z pass neighbouring rows.
//   energy   per-lane strided float64 sums, the xor tree in a wave, the waves in index order, one lane stores: no partials, no atomics.
// The convolution's float expressions are those of pme_recip_convolve_frames (pme_frames.hip), statement for statement, and this unit is
// compiled as that one is, without packed float32 arithmetic (build.py).
#include <cmath>
#include <type_traits>

#include "device_common.h"
#include "host_common.h"
#include "pme_recip_common.h"

using namespace nnpops;

namespace {

constexpr int kThreads = 1024;                // (measured against 256 and 512: docs/LAB_NOTEBOOK_pme_frames_fft.md)
constexpr int kMaxStages = 6;
constexpr int kMaxDim = 64;
constexpr int64_t kLdsBudget = 160 * 1024;

struct AxisPlan { int n, stages, radix[kMaxStages]; };           // n: length of the complex transform (Kz / 2 along z)
struct Plan { int kx, ky, kz, zc, zp; AxisPlan ax[3]; };         // zc = Kz/2 + 1 bins, zp = a z line's stride in complex slots

typedef float2 cf;
__device__ __forceinline__ cf cadd(cf a, cf b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cf csub(cf a, cf b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cf cmul(cf a, cf b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cf cmulc(cf a, cf b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }     // a conj(b)
__device__ __forceinline__ cf conj(cf a) { return make_float2(a.x, -a.y); }
// -i a forward, +i a inverse: the quarter turn of the transform's own direction
template <bool INV> __device__ __forceinline__ cf turn(cf a) { return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x); }

// y[p] = sum_q v[q] w^(pq), w = exp(-+ 2 pi i / R), in place
template <int R, bool INV>
__device__ __forceinline__ void butterfly(cf (&v)[R], const cf* __restrict__ tw, int twn) {
    if constexpr (R == 2) {
        const cf a = v[0];
        v[0] = cadd(a, v[1]); v[1] = csub(a, v[1]);
    } else if constexpr (R == 3) {
        const cf t = cadd(v[1], v[2]), d = csub(v[1], v[2]);
        const cf m = make_float2(v[0].x - 0.5f * t.x, v[0].y - 0.5f * t.y);
        const cf s = turn<INV>(make_float2(0.86602540378443864676f * d.x, 0.86602540378443864676f * d.y));
        v[0] = cadd(v[0], t); v[1] = cadd(m, s); v[2] = csub(m, s);
    } else if constexpr (R == 4) {
        const cf t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]), t2 = cadd(v[1], v[3]), t3 = turn<INV>(csub(v[1], v[3]));
        v[0] = cadd(t0, t2); v[2] = csub(t0, t2); v[1] = cadd(t1, t3); v[3] = csub(t1, t3);
    } else if constexpr (R == 5) {
        constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;      // cos 72, cos 144
        constexpr float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;       // sin 72, sin 144
        const cf a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]), b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
        const cf e1 = make_float2(v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y);
        const cf e2 = make_float2(v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y);
        const cf d1 = turn<INV>(make_float2(s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y));
        const cf d2 = turn<INV>(make_float2(s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y));
        v[0] = cadd(v[0], cadd(a1, a2));
        v[1] = cadd(e1, d1); v[4] = csub(e1, d1); v[2] = cadd(e2, d2); v[3] = csub(e2, d2);
    } else {                                                    // any other prime: the O(R^2) sums, w^a = tw[a twn / R]
        cf y[R];
        const int step = twn / R;
#pragma unroll
        for (int p = 0; p < R; p++) {
            cf s = v[0];
#pragma unroll
            for (int q = 1; q < R; q++) {
                const cf w = tw[((p * q) % R) * step];
                s = cadd(s, INV ? cmulc(v[q], w) : cmul(v[q], w));
            }
            y[p] = s;
        }
#pragma unroll
        for (int p = 0; p < R; p++) v[p] = y[p];
    }
}

// Where a line lies: line l of a pass starts at (l / inner) * histride + l % inner, its elements estride apart.
struct Lines { int count, inner, histride, estride; };

// One stage of every line of a pass: sub-transforms of length L split by radix R.  Forward: butterfly, then the twiddles w_L^(j p);
// inverse: the conjugate twiddles, then the conjugate butterfly -- the transposed stage, on the same slots.
template <int R, bool INV>
__device__ __forceinline__ void fft_stage(cf* __restrict__ grid, const cf* __restrict__ tw, int twn, int n, int L, const Lines ln) {
    const int m = L / R, per_line = n / R, twstep = twn / L, items = ln.count * per_line;
    for (int it = threadIdx.x; it < items; it += kThreads) {
        const int bf = it / ln.count, line = it - bf * ln.count;
        const int blk = bf / m, j = bf - blk * m;
        const int hi = line / ln.inner;
        cf* p = grid + hi * ln.histride + (line - hi * ln.inner) + (blk * L + j) * ln.estride;
        const int step = m * ln.estride;
        cf v[R];
#pragma unroll
        for (int q = 0; q < R; q++) v[q] = p[q * step];
        if (INV) {
#pragma unroll
            for (int q = 1; q < R; q++) v[q] = cmulc(v[q], tw[j * q * twstep]);
        }
        butterfly<R, INV>(v, tw, twn);
        if (!INV) {
#pragma unroll
            for (int q = 1; q < R; q++) v[q] = cmul(v[q], tw[j * q * twstep]);
        }
#pragma unroll
        for (int q = 0; q < R; q++) p[q * step] = v[q];
    }
}

template <bool INV>
__device__ __noinline__ void fft_axis(cf* __restrict__ grid, const cf* __restrict__ tw, int twn, const AxisPlan a, const Lines ln) {
    int L = a.n;
    if (INV)
        for (int s = 0; s + 1 < a.stages; s++) L /= a.radix[s];            // the last stage's length first
    for (int k = 0; k < a.stages; k++) {
        const int s = INV ? a.stages - 1 - k : k;
        switch (a.radix[s]) {                                              // (uniform)
            case 2: fft_stage<2, INV>(grid, tw, twn, a.n, L, ln); break;
            case 3: fft_stage<3, INV>(grid, tw, twn, a.n, L, ln); break;
            case 4: fft_stage<4, INV>(grid, tw, twn, a.n, L, ln); break;
            case 5: fft_stage<5, INV>(grid, tw, twn, a.n, L, ln); break;
            default: fft_stage<7, INV>(grid, tw, twn, a.n, L, ln); break;
        }
        __syncthreads();
        if (INV) { if (s > 0) L *= a.radix[s - 1]; } else L /= a.radix[s];
    }
}

// the natural frequency of storage slot `pos` after the forward stages: slot = p1 n/r1 + p2 n/(r1 r2) + ..., k = p1 + r1 (p2 + r2 (...))
__device__ __forceinline__ int natural_index(const AxisPlan& a, int pos) {
    int L = a.n, k = 0, mult = 1;
    for (int s = 0; s < a.stages; s++) {
        const int r = a.radix[s], m = L / r, p = pos / m;
        pos -= p * m;
        k += p * mult;
        mult *= r;
        L = m;
    }
    return k;
}

template <int VEC>
__global__ __launch_bounds__(kThreads) void pme_frames_transform(const Plan P, const float* __restrict__ boxes, float recip_exp_factor,
                                                                 const float* __restrict__ xmod, const float* __restrict__ ymod,
                                                                 const float* __restrict__ zmod, const float* real_grids,
                                                                 float* potential_grids, float2* __restrict__ scaled_grids,
                                                                 float* __restrict__ energies) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int frame = blockIdx.x, tid = threadIdx.x;
    const int gx = P.kx, gy = P.ky, gz = P.kz, zsize = P.zc, zp = P.zp, H = gz / 2, rows = gx * gy;
    cf* grid = (cf*)lds;
    cf* twx = grid + rows * zp;
    cf* twy = twx + gx;
    cf* twz = twy + gy;
    double* red = (double*)(twz + gz);
    int* natx = (int*)(red + kThreads / 64);
    int* naty = natx + gx;
    int* natz = naty + gy;                                      // [H + 1]: slot H holds bin H
    int* posz = natz + (H + 1);                                 // [H + 1]: the slot of bin k
    float* rgrid = (float*)grid;                                // the real rows: row r's Kz reals from word 2 zp r

    // 1. the frame's real grid, every row into the front of its complex row
    const size_t frame_reals = (size_t)rows * gz;
    {
        typedef typename std::conditional<VEC == 4, float4, float2>::type vec_t;
        const vec_t* src = (const vec_t*)(real_grids + (size_t)frame * frame_reals);
        for (int i = tid; i < (int)(frame_reals / VEC); i += kThreads) {
            const vec_t v = src[i];
            const int e = i * VEC, row = e / gz;
            float2* dst = (float2*)(rgrid + row * 2 * zp + (e - row * gz));
            dst[0] = make_float2(v.x, v.y);
            if constexpr (VEC == 4) dst[1] = make_float2(v.z, v.w);
        }
    }
    // 2. twiddles and index tables
    for (int t = tid; t < gx + gy + gz; t += kThreads) {
        const int axis = t < gx ? 0 : t < gx + gy ? 1 : 2;
        const int i = axis == 0 ? t : axis == 1 ? t - gx : t - gx - gy, n = axis == 0 ? gx : axis == 1 ? gy : gz;
        double s, c;
        sincospi(-2.0 * (double)i / (double)n, &s, &c);
        (axis == 0 ? twx : axis == 1 ? twy : twz)[i] = make_float2((float)c, (float)s);
        if (axis == 0) natx[i] = natural_index(P.ax[0], i);
        if (axis == 1) naty[i] = natural_index(P.ax[1], i);
        if (axis == 2 && i < H) {
            const int k = natural_index(P.ax[2], i);
            natz[i] = k;
            posz[k] = i;
        }
        if (axis == 2 && i == H) { natz[H] = H; posz[H] = H; }
    }
    __syncthreads();

    const Lines zl{rows, 1, zp, 1}, yl{gx * zsize, zsize, gy * zp, zp}, xl{gy * zsize, zsize, zp, gy * zp};
    // 3. z: the half-length transform of (even, odd), then the split: with A = Z[k], B = conj(Z[H - k]), E = (A + B) / 2,
    //    T = w^k (A - B) / (2 i):  X[k] = E + T, X[H - k] = conj(E - T)
    fft_axis<false>(grid, twz, gz, P.ax[2], zl);
    for (int it = tid; it < rows * (H / 2 + 1); it += kThreads) {
        const int k = it / rows, row = it - k * rows;
        cf* r = grid + row * zp;
        if (k == 0) {
            const cf a = r[0];
            r[0] = make_float2(a.x + a.y, 0.f);
            r[H] = make_float2(a.x - a.y, 0.f);
        } else {
            const int pa = posz[k], pb = posz[H - k];
            const cf A = r[pa], B = conj(r[pb]);
            const cf E = make_float2(0.5f * (A.x + B.x), 0.5f * (A.y + B.y));
            const cf D = csub(A, B);
            const cf T = cmul(twz[k], make_float2(0.5f * D.y, -0.5f * D.x));
            r[pa] = cadd(E, T);
            if (pb != pa) r[pb] = conj(csub(E, T));
        }
    }
    __syncthreads();
    // 4. y, then x
    fft_axis<false>(grid, twy, gy, P.ax[1], yl);
    fft_axis<false>(grid, twx, gx, P.ax[0], xl);

    // 5. the convolution: the float expressions of pme_recip_convolve_frames at the slot's natural (kx, ky, kz)
    float b[9];
#pragma unroll
    for (int i = 0; i < 9; i++) b[i] = boxes[9 * (size_t)frame + i];        // (uniform: scalar loads)
    const RecipBox r = recip_box(b);
    const float scale_factor = (float)M_PI * b[0] * b[4] * b[8];
    const int points = rows * zsize;
    float2* scaled = scaled_grids ? scaled_grids + (size_t)frame * points : nullptr;
    double energy = 0.0;
    for (int s = tid; s < points; s += kThreads) {
        const int sx = s / (gy * zsize), rem = s - sx * gy * zsize, sy = rem / zsize, sz = rem - sy * zsize;
        const int kx = natx[sx], ky = naty[sy], kz = natz[sz];
        const int mx = kx < (gx + 1) / 2 ? kx : kx - gx;
        const int my = ky < (gy + 1) / 2 ? ky : ky - gy;
        const int mz = kz < (gz + 1) / 2 ? kz : kz - gz;
        const float mhx = mx * r.r00;
        const float mhy = mx * r.r10 + my * r.r11;
        const float mhz = mx * r.r20 + my * r.r21 + mz * r.r22;
        const float m2 = mhx * mhx + mhy * mhy + mhz * mhz;
        const float denom = m2 * (scale_factor * xmod[kx]) * ymod[ky] * zmod[kz];
        const float eterm = (kx | ky | kz) == 0 ? 0.f : expf(-recip_exp_factor * m2) / denom;
        const float w = (kz > 0 && kz <= (gz - 1) / 2) ? 2.f : 1.f;
        cf* slot = grid + (sx * gy + sy) * zp + sz;
        float2 g = *slot;
        energy += (double)(w * eterm * (g.x * g.x + g.y * g.y));
        g.x *= eterm; g.y *= eterm;
        *slot = g;
        if (scaled) scaled[(kx * gy + ky) * zsize + kz] = g;                // 7. natural order, as box_pi reads it
    }
    // 6. the frame's energy: lanes of a wave in the xor order, then the waves in index order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) energy += __shfl_xor(energy, off, 64);
    if (lane_id() == 0) red[tid >> 6] = energy;
    __syncthreads();                                                        // (and: every slot is scaled)
    if (tid == 0) {
        double e = 0.0;
        for (int w = 0; w < kThreads / 64; w++) e += red[w];
        energies[frame] = (float)(0.5 * e);
    }

    // 8. back: x, y, then z: Z[k] = S + U, Z[H - k] = conj(S - U) with S = X[k] + conj(X[H - k]), U = i conj(w^k) (X[k] - conj(X[H - k]));
    //    no factor anywhere (irfftn with norm = "forward"); the imaginary parts of bins 0 and H are not read, as a library's c2r.
    fft_axis<true>(grid, twx, gx, P.ax[0], xl);
    fft_axis<true>(grid, twy, gy, P.ax[1], yl);
    for (int it = tid; it < rows * (H / 2 + 1); it += kThreads) {
        const int k = it / rows, row = it - k * rows;
        cf* rw = grid + row * zp;
        if (k == 0) {
            const float x0 = rw[0].x, xh = rw[H].x;
            rw[0] = make_float2(x0 + xh, x0 - xh);
        } else {
            const int pa = posz[k], pb = posz[H - k];
            const cf A = rw[pa], B = conj(rw[pb]);
            const cf S = cadd(A, B), D = csub(A, B);
            const cf m = cmulc(D, twz[k]);
            const cf U = make_float2(-m.y, m.x);
            rw[pa] = cadd(S, U);
            if (pb != pa) rw[pb] = conj(csub(S, U));
        }
    }
    __syncthreads();
    fft_axis<true>(grid, twz, gz, P.ax[2], zl);

    // 9. the real potential grid
    {
        typedef typename std::conditional<VEC == 4, float4, float2>::type vec_t;
        vec_t* dst = (vec_t*)(potential_grids + (size_t)frame * frame_reals);
        for (int i = tid; i < (int)(frame_reals / VEC); i += kThreads) {
            const int e = i * VEC, row = e / gz;
            const float2* src = (const float2*)(rgrid + row * 2 * zp + (e - row * gz));
            const float2 lo = src[0];
            if constexpr (VEC == 4) {
                const float2 hi = src[1];
                dst[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
            } else {
                dst[i] = lo;
            }
        }
    }
}

// radix 4 while it divides, then 2, 3, 5, 7; false when a larger prime is left
bool factorize(int n, AxisPlan& a) {
    a.n = n;
    a.stages = 0;
    for (int r : {4, 2, 3, 5, 7})
        while (n % r == 0 && a.stages < kMaxStages) { a.radix[a.stages++] = r; n /= r; }
    return n == 1;
}

// the shape rule; 0 and the reason in last_error when the grid is not served
int64_t make_plan(int gx, int gy, int gz, Plan& p) {
    const int dims[3] = {gx, gy, gz};
    const char* names[3] = {"gridx", "gridy", "gridz"};
    for (int i = 0; i < 3; i++)
        if (dims[i] < 2 || dims[i] > kMaxDim)
            return fail(0, "the LDS transform serves grid dimensions from 2 to %d: %s is %d", kMaxDim, names[i], dims[i]);
    if (gz % 2 != 0) return fail(0, "the LDS transform needs an even gridz (the real transform runs at half length): gridz is %d", gz);
    p.kx = gx; p.ky = gy; p.kz = gz; p.zc = gz / 2 + 1; p.zp = p.zc | 1;
    for (int i = 0; i < 3; i++)
        if (!factorize(i == 2 ? gz / 2 : dims[i], p.ax[i]))
            return fail(0, "the LDS transform serves grid dimensions whose prime factors are at most 7: %s is %d", names[i], dims[i]);
    const int64_t bytes = (int64_t)gx * gy * p.zp * 8 + (int64_t)(gx + gy + gz) * 8 + (kThreads / 64) * 8 + (int64_t)(gx + gy + 2 * (gz / 2 + 1)) * 4;
    if (bytes > kLdsBudget)
        return fail(0, "the LDS transform keeps a frame's half-spectrum in the 160 KiB of LDS of one workgroup: a %d x %d x %d grid needs "
                       "%lld bytes (gridx * gridy * (gridz / 2 + 1) * 8 and its tables)", gx, gy, gz, (long long)bytes);
    return bytes;
}

}  // namespace

extern "C" {

int64_t nnpops_pme_reciprocal_frames_transform_lds_bytes(int gridx, int gridy, int gridz) {
    Plan p;
    return make_plan(gridx, gridy, gridz, p);
}

int nnpops_pme_reciprocal_frames_transform(int num_atoms, int num_frames, int gridx, int gridy, int gridz, int order, const float* box_vectors,
                                           float alpha, const float* xmoduli, const float* ymoduli, const float* zmoduli,
                                           const float* real_grids, float* potential_grids, void* scaled_grids, float* energies, void* stream) {
    NNPOPS_REQUIRE(num_atoms >= 0 && num_frames >= 1, "bad sizes (atoms %d, frames %d)", num_atoms, num_frames);
    NNPOPS_REQUIRE(order == 4 || order == 5, "Only pmeOrder 4 or 5 is supported (got %d)", order);
    Plan p;
    const int64_t bytes = make_plan(gridx, gridy, gridz, p);
    if (bytes == 0) return NNPOPS_ERR_INVALID_ARGUMENT;                     // (make_plan left the reason)
    NNPOPS_REQUIRE(alpha > 0, "alpha must be positive");
    NNPOPS_REQUIRE(box_vectors && xmoduli && ymoduli && zmoduli && real_grids && potential_grids && energies, "NULL device pointer");
    NNPOPS_REQUIRE((uintptr_t)real_grids % 8 == 0 && (uintptr_t)potential_grids % 8 == 0 && (uintptr_t)scaled_grids % 8 == 0,
                   "the grids must be 8-byte aligned");
    const bool vec4 = gridz % 4 == 0 && (uintptr_t)real_grids % 16 == 0 && (uintptr_t)potential_grids % 16 == 0;
    auto k = vec4 ? pme_frames_transform<4> : pme_frames_transform<2>;
    // the LDS grant of each of the two kernels, per device: raised when a shape needs more than any before it
    static int granted[2][64];
    int device = 0;
    NNPOPS_HIP_TRY(hipGetDevice(&device));
    int& have = granted[vec4 ? 1 : 0][device & 63];
    if (bytes > 64 * 1024 && bytes > have) {
        NNPOPS_HIP_TRY(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = (int)bytes;
    }
    const float recip_exp_factor = (float)(M_PI * M_PI / ((double)alpha * (double)alpha));
    hipLaunchKernelGGL(k, dim3((unsigned)num_frames), dim3(kThreads), (size_t)bytes, (hipStream_t)stream, p, box_vectors, recip_exp_factor,
                       xmoduli, ymoduli, zmoduli, real_grids, potential_grids, (float2*)scaled_grids, energies);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // extern "C"
