// cfconv_build.h -- the CFConv neighbour list: full rows {dx, dy, dz, j} per atom (from the shared cell grid of celllist.h or an
// all-pairs scan for small systems) and, behind them, the half list -- a slot per pair that both ends know (scan_half / half_slots).
// Included by cfconv.hip only.
#pragma once

#include "celllist.h"

namespace {
using namespace nnpops;

enum { kStOverflow = 0, kStMaxRow = 1, kStPairs = 2, kStUnmatched = 3, kStWordsN = 4 };


// ---------------------------------------------------------------------------------------------
// neighbour rows (full list): one wave per atom
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void append(float4* __restrict__ row, int* __restrict__ row_ids, int cap, bool keep, float dx, float dy,
                                       float dz, int j, int& n) {
    const unsigned long long m = __ballot(keep);
    if (keep) {
        const int slot = n + prefix_popc(m);
        if (slot < cap) {
            row[slot] = make_float4(dx, dy, dz, __int_as_float(j));
            row_ids[slot] = j;                              // the ids alone, 4 bytes apart: what half_slots searches
        }
    }
    n += __popcll(m);
}

// One lane per row: the row's length and how many of its pairs are with a higher index -- scan_half turns those into
// the row's range of pair slots (see "Half list" below).
__device__ __forceinline__ void publish_row(int i, int n, int n_lo, int* __restrict__ cnt, int* __restrict__ lo_cnt) {
    cnt[i] = n;
    lo_cnt[i] = n_lo;
}

template <bool PERIODIC>
__global__ __launch_bounds__(64) void rows_allpairs(int N, const float* __restrict__ pos, const float* __restrict__ box,
                                                    float cutoff2, float4* __restrict__ rows, int* __restrict__ ids, int cap,
                                                    int* __restrict__ cnt, int* __restrict__ lo_cnt) {
    const int i = blockIdx.x, lane = lane_id();
    Box b{};
    if (PERIODIC) b = load_box(box);
    const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
    float4* row = rows + (size_t)i * cap;
    int n = 0, n_lo = 0;
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        bool keep = false;
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (j < N && j != i) {
            dx = pos[3 * j] - xi; dy = pos[3 * j + 1] - yi; dz = pos[3 * j + 2] - zi;
            min_image<PERIODIC>(dx, dy, dz, b);
            keep = dx * dx + dy * dy + dz * dz < cutoff2;          // strict, on r^2 (ref :110)
        }
        append(row, ids + (size_t)i * cap, cap, keep, dx, dy, dz, j, n);
        n_lo += __popcll(__ballot(keep && j > i));
    }
    if (lane == 0) publish_row(i, n, n_lo, cnt, lo_cnt);
}

// Batched molecules (nnpops_cfconv_neighbors_set_molecules): rows_allpairs<false> with the scan confined to the atom's own molecule,
// segment[i] = {lo, hi} as in ani_kernels.h.  The same displacement arithmetic and strict test, candidates in ascending index order,
// so a molecule's rows are those of rows_allpairs on the molecule alone with every index moved by lo -- whatever the other molecules
// hold, NaN included: no lane ever reads a position outside [lo, hi).  One wave per atom; a molecule of up to 64 atoms is one pass.
__global__ __launch_bounds__(64) void rows_segments(int N, const float* __restrict__ pos, const int2* __restrict__ segment,
                                                    float cutoff2, float4* __restrict__ rows, int* __restrict__ ids, int cap,
                                                    int* __restrict__ cnt, int* __restrict__ lo_cnt) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= N) return;
    const int2 seg = segment[i];
    const int lo = max(seg.x, 0), hi = min(seg.y, N);       // (the host validated the table: the clamps keep a damaged one in bounds)
    const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
    float4* row = rows + (size_t)i * cap;
    int n = 0, n_lo = 0;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        bool keep = false;
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (j < hi && j != i) {
            dx = pos[3 * j] - xi; dy = pos[3 * j + 1] - yi; dz = pos[3 * j + 2] - zi;
            keep = dx * dx + dy * dy + dz * dz < cutoff2;          // strict, on r^2, as rows_allpairs
        }
        append(row, ids + (size_t)i * cap, cap, keep, dx, dy, dz, j, n);
        n_lo += __popcll(__ballot(keep && j > i));
    }
    if (lane == 0) publish_row(i, n, n_lo, cnt, lo_cnt);
}

// Periodic frames (nnpops_cfconv_neighbors_set_frames): rows_segments with every frame in its own box.  frame[i] = {lo, hi, m, 0}, the
// atom's frame [lo, hi) and its number: one 16-byte entry at a wave-uniform address (blockIdx.x = i), so the frame, and behind it the
// nine floats of boxes[m] (load_box), arrive through scalar loads and no vector load stands before the scan.  The displacement
// arithmetic is that of rows_allpairs<true> -- pos[j] - pos[i], min_image<true> against the frame's box, the strict test on r^2,
// candidates in ascending index -- so a frame's rows are those of rows_allpairs<true> on the frame alone with every index moved by
// lo, whatever the other frames and their boxes hold: no lane reads a position outside [lo, hi) or a box other than m's.
__global__ __launch_bounds__(64) void rows_frames(int N, int num_frames, const float* __restrict__ pos, const float* __restrict__ boxes,
                                                  const int4* __restrict__ frame, float cutoff2, float4* __restrict__ rows,
                                                  int* __restrict__ ids, int cap, int* __restrict__ cnt, int* __restrict__ lo_cnt) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= N) return;
    const int4 fr = frame[i];
    const int lo = max(fr.x, 0), hi = min(fr.y, N);         // (the host validated the table: the clamps keep a damaged one in bounds)
    const int m = min(max(fr.z, 0), num_frames - 1);
    const Box b = load_box(boxes + 9 * (size_t)m);
    const float xi = pos[3 * i], yi = pos[3 * i + 1], zi = pos[3 * i + 2];
    float4* row = rows + (size_t)i * cap;
    int n = 0, n_lo = 0;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        bool keep = false;
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (j < hi && j != i) {
            dx = pos[3 * j] - xi; dy = pos[3 * j + 1] - yi; dz = pos[3 * j + 2] - zi;
            min_image<true>(dx, dy, dz, b);
            keep = dx * dx + dy * dy + dz * dz < cutoff2;          // strict, on r^2, as rows_allpairs
        }
        append(row, ids + (size_t)i * cap, cap, keep, dx, dy, dz, j, n);
        n_lo += __popcll(__ballot(keep && j > i));
    }
    if (lane == 0) publish_row(i, n, n_lo, cnt, lo_cnt);
}

template <bool PERIODIC>
__global__ __launch_bounds__(64) void rows_cells(const float* __restrict__ box, float cutoff2,
                                                 const CellGrid* __restrict__ grid, const int* __restrict__ cell_start,
                                                 const int* __restrict__ sorted_cell, const float4* __restrict__ sorted_pos,
                                                 float4* __restrict__ rows, int* __restrict__ ids, int cap, int* __restrict__ cnt,
                                                 int* __restrict__ lo_cnt, int* __restrict__ status,
                                                 int* __restrict__ cell_hist) {
    const int lane = lane_id();
    clear_cell_histogram(cell_hist, (int)blockIdx.x * 64 + lane, (int)gridDim.x * 64);      // (one wave per workgroup)
    const CellGrid g = *grid;
    if (!g.ok) {
        if (lane == 0) {
            if (blockIdx.x == 0) atomicOr(&status[kStOverflow], refused_grid_bits(g));
            publish_row((int)blockIdx.x, 0, 0, cnt, lo_cnt);
        }
        return;
    }
    Box b{};
    if (PERIODIC) b = load_box(box);
    const float4 me = sorted_pos[blockIdx.x];
    const int i = __float_as_int(me.w) & kIdMask;
    const int c = sorted_cell[blockIdx.x];                  // (in sorted order, next to the position: no load that waits for the id)
    const int cx = c % g.nx, cy = (c / g.nx) % g.ny, cz = c / (g.nx * g.ny);
    float4* row = rows + (size_t)i * cap;
    int n = 0, n_lo = 0;
    // the 27-cell stencil as one flat candidate space (celllist.h): full iterations, FOUR batches of candidates requested at a
    // time -- this wave's time is the sum of its dependent round trips to memory (~380 candidates: six batches, one after the
    // other with one load ahead, were five trips; now two)
    const Stencil st = gather_stencil(g, cell_start, cx, cy, cz);
    const int last = max(st.total - 1, 0);
    constexpr int GROUP = 4;
    for (int base = 0; base < st.total; base += 64 * GROUP) {
        float4 pj[GROUP];
#pragma unroll
        for (int q = 0; q < GROUP; q++) pj[q] = sorted_pos[stencil_slot(st, min(base + 64 * q + lane, last))];   // (every lane: ds_bpermute inside)
#pragma unroll
        for (int q = 0; q < GROUP; q++) {
            if (base + 64 * q >= st.total) break;               // wave-uniform
            const int k = base + 64 * q + lane;
            const float4 cur = pj[q];
            bool keep = false;
            int j = -1;
            float dx = 0.f, dy = 0.f, dz = 0.f;
            if (k < st.total) {
                j = __float_as_int(cur.w) & kIdMask;
                if (j != i) {
                    dx = cur.x - me.x; dy = cur.y - me.y; dz = cur.z - me.z;
                    min_image<PERIODIC>(dx, dy, dz, b);
                    keep = dx * dx + dy * dy + dz * dz < cutoff2;
                }
            }
            append(row, ids + (size_t)i * cap, cap, keep, dx, dy, dz, j, n);
            n_lo += __popcll(__ballot(keep && j > i));
        }
    }
    if (lane == 0) publish_row(i, n, n_lo, cnt, lo_cnt);
}

// ---------------------------------------------------------------------------------------------
// Half list behind the full rows.  The matrix-core kernels evaluate the filter network ONCE per pair {i, j}: every
// pair gets a slot (`pid`) -- the pairs a row holds with a higher index, in row order -- and every entry
// of the full rows learns the slot of its pair, so that the owner-computes gather (cfconv_gather) can fetch the
// filter row from either end.  half_off[i] = first slot of row i (scan_half); the entry (i -> j), j < i finds its slot by looking i up in row j.  An entry whose mirror image is missing (a pair within rounding of the cutoff, where the
// cosine cutoff makes its contribution vanish) points at the all-zero row `pair_cap`.
// ---------------------------------------------------------------------------------------------
// Exclusive scan of lo_cnt -> half_off, total in half_off[N].  One workgroup: every thread takes kScanPerThread
// consecutive rows (independent 16-byte loads), one block-wide scan of the thread totals per 16 K rows.
constexpr int kScanPerThread = 16;
__global__ __launch_bounds__(1024) void scan_half(int N, const int* __restrict__ lo_cnt, int* __restrict__ half_off) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < N; base += 1024 * kScanPerThread) {
        const int k0 = base + threadIdx.x * kScanPerThread;
        int v[kScanPerThread], mine = 0;
        if (k0 + kScanPerThread <= N) {
#pragma unroll
            for (int q = 0; q < kScanPerThread; q += 4) {
                const int4 t = *reinterpret_cast<const int4*>(lo_cnt + k0 + q);
                v[q] = t.x; v[q + 1] = t.y; v[q + 2] = t.z; v[q + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < kScanPerThread; q++) v[q] = k0 + q < N ? lo_cnt[k0 + q] : 0;
        }
#pragma unroll
        for (int q = 0; q < kScanPerThread; q++) mine += v[q];
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const int t = wsum[w];
            before += w < wave ? t : 0;
            total += t;
        }
        int run = carry + before + incl - mine;
#pragma unroll
        for (int q = 0; q < kScanPerThread; q++) {
            const int mine_q = run;
            run += v[q];
            v[q] = mine_q;
        }
        if (k0 + kScanPerThread <= N) {
#pragma unroll
            for (int q = 0; q < kScanPerThread; q += 4)
                *reinterpret_cast<int4*>(half_off + k0 + q) = make_int4(v[q], v[q + 1], v[q + 2], v[q + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < kScanPerThread; q++)
                if (k0 + q < N) half_off[k0 + q] = v[q];
        }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) half_off[N] = carry;
}

// (the reverse lookup of a pair is described where it happens, below)
__global__ __launch_bounds__(64) void half_slots(const float4* __restrict__ rows, const int* __restrict__ row_ids,
                                                 const int* __restrict__ cnt, const int* __restrict__ half_off, int cap,
                                                 int pair_cap, int* __restrict__ pid, float* __restrict__ half_r,
                                                 int2* __restrict__ half_ij, int* __restrict__ status, int N,
                                                 const float4* __restrict__ sorted_pos) {
    const int lane = lane_id();
    const int k0 = __builtin_amdgcn_readfirstlane(xcd_contiguous_wave_id());      // atoms in cell order when there is one: the rows looked up are L2-hot (wave-uniform: scalar loads)
    if (k0 >= N) return;
    const int i = sorted_pos ? __float_as_int(sorted_pos[k0].w) & kIdMask : k0;
    if (i >= N) return;
    const int n = min(cnt[i], cap);
    const int first = half_off[i];
    int lo_before = 0;
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        int j = i;
        bool lower = false;
        float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < n) {
            rec = rows[(size_t)i * cap + s];
            j = __float_as_int(rec.w) & kIdMask;
            lower = j > i;
        }
        const unsigned long long lm = __ballot(lower);
        int my_pid = pair_cap, unmatched = 0;
        if (lower) {
            int p = first + lo_before + prefix_popc(lm);
            if (p >= pair_cap) p = pair_cap;                 // (only after a row overflow: check() grows and rebuilds)
            my_pid = p;
            if (p < pair_cap) {
                half_r[p] = sqrtf(rec.x * rec.x + rec.y * rec.y + rec.z * rec.z);
                half_ij[p] = make_int2(i, j);
            }
        }
        lo_before += __popcll(lm);
        // entries towards a lower index j: slot = first slot of row j + rank of i among j's higher-index neighbours.  Every such lane
        // looks its own pair up: the whole id row of j (64 ids per pass) is requested at once, sixteen 16-byte loads per lane with
        // nothing between them, so all lookups of the atom cost ONE round trip to memory -- taking the rows eight at a time with the
        // wave scanning each one together (rounds 1-3) was four dependent round trips for the ~26 lower neighbours of an atom, and
        // this kernel is nothing but its chain of dependent first-touch loads (33 us for 10 000 atoms against 10 us without lookups).
        if (s < n && !lower) {
            const int nj = min(cnt[j], cap), fj = half_off[j];
            const int4* rid = reinterpret_cast<const int4*>(row_ids + (size_t)j * cap);      // (cap is a multiple of 4)
            const int pieces = cap >> 2;
            bool hit = false;
            int rank = 0;
            for (int t0 = 0; t0 < nj && !hit; t0 += 64) {
                int4 v[16];
#pragma unroll
                for (int q = 0; q < 16; q++) v[q] = rid[min((t0 >> 2) + q, pieces - 1)];
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    const int id4[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const bool open = !hit && t0 + 4 * q + c < nj;          // (before the hit, inside the row)
                        hit = hit || (open && id4[c] == i);
                        rank += (open && id4[c] != i && id4[c] > j) ? 1 : 0;
                    }
                }
            }
            my_pid = hit ? min(fj + rank, pair_cap) : pair_cap;
            unmatched += hit ? 0 : 1;
        }
        if (s < n) pid[(size_t)i * cap + s] = my_pid;
        if (unmatched) atomicAdd(&status[kStUnmatched], 1);
    }
}

// max row length and number of half pairs (j > i) of the last build
__global__ __launch_bounds__(256) void row_stats(int N, const int* __restrict__ cnt, const float4* __restrict__ rows, int cap,
                                                 int* __restrict__ status) {
    __shared__ int red[2][256];
    int mrow = 0, half = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const int n = cnt[i];
        mrow = max(mrow, n);
        const int m = min(n, cap);
        for (int e = 0; e < m; e++) half += (__float_as_int(rows[(size_t)i * cap + e].w) & kIdMask) > i;
    }
    red[0][threadIdx.x] = mrow;
    red[1][threadIdx.x] = half;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            red[0][threadIdx.x] = max(red[0][threadIdx.x], red[0][threadIdx.x + off]);
            red[1][threadIdx.x] += red[1][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMax(&status[kStMaxRow], red[0][0]);
        atomicAdd(&status[kStPairs], red[1][0]);
        if (red[0][0] > cap) atomicOr(&status[kStOverflow], 1);
    }
}

}  // namespace
