// neighbor_pairs_frames.h -- getNeighborPairsFrames: the pair lists of a batch of frames, every frame in its own box, in one launch
// sequence (C ABI: nnpops_neighbor_pairs_frames_*).  Included by neighbor_pairs.hip, whose wrapped_delta, scan_rows and fill_unused it
// shares: a frame's outputs are the bits the single-system all-pairs path gives for that frame alone.
//
// Work split.  A frame of n atoms has n(n-1)/2 candidate pairs, flat index p <-> (row, col < row) in row-major order.  The host cuts
// every frame's flat range into SEGMENTS of at most kPartPairs pairs (frame_table: one int32 record {frame, first atom, atom count,
// first flat pair, pair count} per segment, ordered by frame, then by first pair) and one workgroup of four waves takes one segment:
//   * the record is uniform: frame, atom range and the frame's nine box entries are scalar loads, done once;
//   * the atoms the segment's rows and columns can touch are the frame's atoms 0 .. r_hi (r_hi the row of its last pair): they are
//     staged in LDS when there are at most kFrameLdsAtoms of them, and read from global memory otherwise;
//   * every wave owns a contiguous quarter of the segment and its lanes walk flat indices, 64 at a time: a wave is as full for a frame
//     of 5 atoms as for one of 300, where one wave per row (pairs_allpairs) idles two thirds of its lanes on a 21-atom frame.
// Counts are kept per (segment, wave), not per row: a wave's pairs are contiguous in the output -- (frame, row, col) ascending is the
// order of the flat index -- so one count per wave is all the scan needs, a frame of n atoms costs 4 ceil(n(n-1)/2 / kPartPairs) scan
// entries instead of n, and no wave ever has to find out where a row that it shares with its neighbour begins.
//   PASS 0 counts, scan_rows turns the 4 S counts into every wave's first slot and num_pairs, PASS 1 recomputes and writes with ballot
//   ranks.  max_num_pairs == -1 is one pass: slot = (pairs of all earlier segments) + offset in the segment.
// The first slot of every segment (segment_slots [S + 1]) is kept: the box gradient walks a segment's slots with that segment's box.
//
// The kernels never read positions outside [0, N) or boxes outside [0, B) whatever the table holds: load_segment clamps.
#pragma once

#include "box_grad.h"

namespace {

constexpr int kPartPairs = NNPOPS_PAIRS_FRAMES_PART_PAIRS;
constexpr int kFrameLdsAtoms = 512;      // 6 KiB (float32) / 12 KiB (float64) of LDS per workgroup: 13 workgroups per CU still fit
constexpr int kFrameMaxAtoms = 65536;    // a frame's triangle must fit the table's int32 flat indices

// The kernels of this header are compiled without packed float32 arithmetic (v_pk_add / mul / fma_f32): plain VALU instructions give
// the same IEEE results, element by element, so the bits still match pairs_allpairs.
#define NNPOPS_FRAMES_KERNEL __attribute__((target("no-packed-fp32-ops"))) __global__

struct Segment { int frame, first, n, p0, cnt; };

__device__ __forceinline__ Segment load_segment(const int32_t* __restrict__ table, int seg, int N, int B) {
    const int32_t* r = table + 5 * (size_t)seg;                             // (uniform address: scalar loads)
    Segment s;
    s.frame = min(max(r[0], 0), max(B - 1, 0));
    s.first = min(max(r[1], 0), N);
    s.n = min(min(max(r[2], 0), N - s.first), kFrameMaxAtoms);
    const long long tri = (long long)s.n * (s.n - 1) / 2;
    s.p0 = (int)min((long long)max(r[3], 0), tri);
    s.cnt = (int)min((long long)min(max(r[4], 0), kPartPairs), tri - s.p0);
    return s;
}

// the row of flat pair p: the largest r with r (r - 1) / 2 <= p.  The square root only proposes; the integer steps decide.
__device__ __forceinline__ int tri_row(int p) {
    int r = (int)((1.0f + sqrtf(8.0f * (float)p + 1.0f)) * 0.5f);
    r = max(r, 1);
    while ((long long)r * (r - 1) / 2 > p) r--;
    while ((long long)(r + 1) * r / 2 <= p) r++;
    return r;
}

template <typename T, int PASS, bool ALL_SLOTS>
NNPOPS_FRAMES_KERNEL __launch_bounds__(256) void pairs_frames(int N, int B, int S, const int32_t* __restrict__ table, const T* __restrict__ pos,
                                                    const T* __restrict__ boxes, T cutoff2, long long num_slots,
                                                    int* __restrict__ wave_count, const int* __restrict__ row_offset,
                                                    const int* __restrict__ block_prefix, int* __restrict__ ticket,
                                                    int32_t* __restrict__ segment_slots, int32_t* __restrict__ neighbors,
                                                    T* __restrict__ deltas, T* __restrict__ distances, int32_t* __restrict__ num_pairs) {
    __shared__ T spos[3 * kFrameLdsAtoms];
    __shared__ long long before[4];
    const int seg = blockIdx.x;
    const int lane = lane_id(), wave = wave_in_group();
    if (PASS == 0 && !ALL_SLOTS && seg == 0 && threadIdx.x == 0) *ticket = 0;      // the scan's ticket counter (workspace is not zeroed)
    const Segment s = load_segment(table, seg, N, B);
    const T* box = boxes ? boxes + 9 * (size_t)s.frame : nullptr;
    const T* fpos = pos + 3 * (size_t)s.first;
    const int r_hi = s.cnt > 0 ? tri_row(s.p0 + s.cnt - 1) : 0;            // (< s.n: p0 + cnt lies inside the frame's triangle)
    const bool staged = r_hi < kFrameLdsAtoms;
    if (staged && s.cnt > 0)
        for (int k = threadIdx.x; k < 3 * (r_hi + 1); k += 256) spos[k] = fpos[k];
    if (ALL_SLOTS) {
        // the slots of all earlier segments: frames are concatenated, and a frame's segments tile its triangle
        long long sum = 0;
        for (int q = threadIdx.x; q < seg; q += 256) sum += table[5 * (size_t)q + 4];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (lane == 0) before[wave] = sum;
    }
    __syncthreads();
    long long base_slot = 0;
    if (ALL_SLOTS) base_slot = before[0] + before[1] + before[2] + before[3];
    else if (PASS == 1) base_slot = first_slot(row_offset, block_prefix, 4 * seg + wave);
    if ((ALL_SLOTS || PASS == 1) && threadIdx.x == 0) {
        segment_slots[seg] = (int32_t)base_slot;
        if (seg == S - 1) segment_slots[S] = ALL_SLOTS ? (int32_t)(base_slot + s.cnt) : block_prefix[(4 * S + kScanBlock - 1) / kScanBlock];
    }
    const int quarter = (s.cnt + 3) >> 2;
    const int lo = min(wave * quarter, s.cnt), hi = min(lo + quarter, s.cnt);
    int found = 0;
    for (int b0 = lo; b0 < hi; b0 += 64) {
        const int k = b0 + lane;
        bool keep = false;
        Vec3<T> d{0, 0, 0};
        T d2 = 0;
        int row = 0, col = 0;
        if (k < hi) {
            const int p = s.p0 + k;
            row = tri_row(p);
            col = p - (int)((long long)row * (row - 1) / 2);
            d = staged ? wrapped_delta<T>(spos, row, col, box, box != nullptr) : wrapped_delta<T>(fpos, row, col, box, box != nullptr);
            d2 = allpairs_norm2<T>(d);
            keep = !(d2 > cutoff2);
        }
        const unsigned long long m = __ballot(keep);
        if (keep && (PASS == 1 || ALL_SLOTS)) {
            const long long slot = ALL_SLOTS ? base_slot + k : base_slot + found + prefix_popc(m);
            if ((unsigned long long)slot < (unsigned long long)num_slots) {
                neighbors[slot] = s.first + row;
                neighbors[num_slots + slot] = s.first + col;
                deltas[3 * slot] = d.x; deltas[3 * slot + 1] = d.y; deltas[3 * slot + 2] = d.z;
                distances[slot] = sqrt(d2);
            }
        }
        found += __popcll(m);
    }
    if (lane == 0) {
        if (PASS == 0 && !ALL_SLOTS) wave_count[4 * seg + wave] = found;
        if (ALL_SLOTS && found) atomicAdd(num_pairs, found);
    }
}

// grad_box[m][a][:] = - sum_k n_ka G_k over the slots of frame m (pairs_second_order.hip: derivation; box_grad.h: image_shift).
// One workgroup per segment walks the segment's own slots [segment_slots[seg], segment_slots[seg + 1]), clamped to the list, lane t
// slots t, t + 256, ... in float64, then box_block_sum9: a fixed order.
template <typename T>
NNPOPS_FRAMES_KERNEL __launch_bounds__(kBoxThreads) void pairs_box_partials_frames(int N, int B, const int32_t* __restrict__ table,
                                                                         const int32_t* __restrict__ segment_slots, long long num_slots,
                                                                         const int32_t* __restrict__ neighbors, const T* __restrict__ pos,
                                                                         const T* __restrict__ boxes, const T* __restrict__ deltas,
                                                                         const T* __restrict__ distances, const T* __restrict__ grad_deltas,
                                                                         const T* __restrict__ grad_distances, double* __restrict__ partials) {
    const int seg = blockIdx.x;
    const Segment s = load_segment(table, seg, N, B);
    const T* box = boxes + 9 * (size_t)s.frame;
    const long long k0 = min((long long)max(segment_slots[seg], 0), num_slots);
    const long long k1 = min((long long)max(segment_slots[seg + 1], 0), num_slots);
    double acc[9];
#pragma unroll
    for (int q = 0; q < 9; q++) acc[q] = 0.0;
    for (long long k = k0 + threadIdx.x; k < k1; k += kBoxThreads) {
        const int i = neighbors[k] - s.first, j = neighbors[num_slots + k] - s.first;
        if ((unsigned)i >= (unsigned)s.n || (unsigned)j >= (unsigned)s.n) continue;      // (unused, or not this frame's: nothing is read)
        const T dx = deltas[3 * k], dy = deltas[3 * k + 1], dz = deltas[3 * k + 2];
        const T gd = grad_distances[k] / distances[k];                      // (the first-order kernels' G, bit for bit)
        const T G[3] = {grad_deltas[3 * k] + dx * gd, grad_deltas[3 * k + 1] + dy * gd, grad_deltas[3 * k + 2] + dz * gd};
        T n[3];
        image_shift(pos + 3 * (size_t)s.first, i, j, dx, dy, dz, box, n);
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int q = 0; q < 3; q++) acc[3 * a + q] -= (double)n[a] * (double)G[q];
    }
    box_block_sum9(acc, partials + (size_t)seg * 9);
}

// one wave per frame: the frame's segments are consecutive in the table; lane q < 9 adds their partial sums in segment order
template <typename T>
NNPOPS_FRAMES_KERNEL __launch_bounds__(64) void pairs_box_finish_frames(int S, const int32_t* __restrict__ table, const double* __restrict__ partials,
                                                              T* __restrict__ grad_boxes) {
    const int frame = blockIdx.x;
    auto first_of = [&](int f) {                                            // the first segment whose frame is >= f
        int lo = 0, hi = S;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (table[5 * (size_t)mid] < f) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    const int begin = first_of(frame), end = first_of(frame + 1);
    if (threadIdx.x < 9) {
        double sum = 0.0;
        for (int q = begin; q < end; q++) sum += partials[(size_t)q * 9 + threadIdx.x];
        grad_boxes[(size_t)frame * 9 + threadIdx.x] = (T)sum;
    }
}

size_t frames_workspace_bytes(int S) {
    // wave_count [4S + 1] | row_offset [4S + 1] | block_prefix [ceil(4S / 1024) + 1] and the scan's ticket behind it
    return 3 * 256 + sizeof(int) * (2 * (4 * (size_t)S + 1) + (4 * (size_t)S / kScanBlock + 4));
}

template <typename T>
int frames_forward_impl(int N, int B, int S, const int32_t* table, const T* pos, const T* boxes, double cutoff, bool all_slots,
                        long long num_slots, int32_t* neighbors, T* deltas, T* distances, int32_t* num_pairs, int32_t* segment_slots,
                        void* workspace, hipStream_t stream) {
    const T c = (T)cutoff;
    const T cutoff2 = c * c;
    const int rows = 4 * S, nscan = div_up(rows, kScanBlock);
    char* base = (char*)workspace;
    int* wave_count = (int*)base;
    int* row_offset = (int*)(base + align_up(sizeof(int) * ((size_t)rows + 1)));
    int* block_prefix = (int*)((char*)row_offset + align_up(sizeof(int) * ((size_t)rows + 1)));
    int* ticket = block_prefix + nscan + 1;
    if (num_slots > 0)
        hipLaunchKernelGGL(fill_unused<T>, dim3(div_up(num_slots, 256)), dim3(256), 0, stream, num_slots, neighbors, deltas, distances, num_pairs);
    else
        hipLaunchKernelGGL(zero_words, dim3(1), dim3(256), 0, stream, 1LL, (int*)num_pairs);
    if (S == 0) {
        hipLaunchKernelGGL(zero_words, dim3(1), dim3(256), 0, stream, 1LL, (int*)segment_slots);
        NNPOPS_HIP_TRY(hipGetLastError());
        return NNPOPS_OK;
    }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(S), dim3(256), 0, stream, N, B, S, table, pos, boxes, cutoff2, num_slots, wave_count, row_offset,
                           block_prefix, ticket, segment_slots, neighbors, deltas, distances, num_pairs);
    };
    if (all_slots) {
        launch(pairs_frames<T, 1, true>);
    } else {
        launch(pairs_frames<T, 0, false>);
        hipLaunchKernelGGL(scan_rows, dim3(nscan), dim3(kScanBlock), 0, stream, rows, wave_count, row_offset, block_prefix, ticket, num_pairs);
        launch(pairs_frames<T, 1, false>);
    }
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

template <typename T>
void frames_box_backward_impl(int N, int B, int S, const int32_t* table, const int32_t* segment_slots, long long num_slots,
                              const int32_t* neighbors, const void* pos, const void* boxes, const void* deltas, const void* distances,
                              const void* grad_deltas, const void* grad_distances, void* grad_boxes, double* partials, hipStream_t stream) {
    if (S > 0)
        hipLaunchKernelGGL(pairs_box_partials_frames<T>, dim3(S), dim3(kBoxThreads), 0, stream, N, B, table, segment_slots, num_slots,
                           neighbors, (const T*)pos, (const T*)boxes, (const T*)deltas, (const T*)distances, (const T*)grad_deltas,
                           (const T*)grad_distances, partials);
    hipLaunchKernelGGL(pairs_box_finish_frames<T>, dim3(B), dim3(64), 0, stream, S, table, (const double*)partials, (T*)grad_boxes);
}

}  // namespace

extern "C" {

int64_t nnpops_neighbor_pairs_frames_table(int num_frames, const int64_t* offsets, int32_t* rows) {
    NNPOPS_REQUIRE(num_frames >= 0 && offsets != nullptr, "Expected \"offsets\" to hold at least one entry");
    NNPOPS_REQUIRE(offsets[0] == 0, "Expected \"offsets\" to start at 0");
    int64_t S = 0;
    for (int m = 0; m < num_frames; m++) {
        const int64_t first = offsets[m], n = offsets[m + 1] - first;
        NNPOPS_REQUIRE(n >= 0, "Expected \"offsets\" to be ascending");
        NNPOPS_REQUIRE(offsets[m + 1] <= std::numeric_limits<int32_t>::max(), "Too many atoms for getNeighborPairsFrames");
        NNPOPS_REQUIRE(n <= kFrameMaxAtoms, "Expected every frame of \"offsets\" to hold at most %d atoms", kFrameMaxAtoms);
        const int64_t tri = n * (n - 1) / 2;
        for (int64_t p0 = 0; p0 < tri; p0 += kPartPairs, S++) {
            if (!rows) continue;
            int32_t* r = rows + 5 * S;
            r[0] = m; r[1] = (int32_t)first; r[2] = (int32_t)n; r[3] = (int32_t)p0; r[4] = (int32_t)std::min<int64_t>(kPartPairs, tri - p0);
        }
        NNPOPS_REQUIRE(S <= std::numeric_limits<int32_t>::max() / 8, "Too many segments for getNeighborPairsFrames");
    }
    return S;
}

int64_t nnpops_neighbor_pairs_frames_workspace_bytes(int num_segments) {
    return num_segments < 0 ? 0 : (int64_t)frames_workspace_bytes(num_segments);
}

int nnpops_neighbor_pairs_frames_forward(int dtype, int num_atoms, int num_frames, int num_segments, const int32_t* table,
                                         const void* positions, const void* boxes, double cutoff, int64_t max_num_pairs, int64_t num_slots,
                                         int32_t* neighbors, void* deltas, void* distances, int32_t* num_pairs, int32_t* segment_slots,
                                         void* workspace, void* stream) {
    NNPOPS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (float32) or 1 (float64)");
    NNPOPS_REQUIRE(num_atoms > 0, "Expected the 1nd dimension size of \"positions\" to be more than 0");
    NNPOPS_REQUIRE(num_frames > 0, "Expected \"table\" to describe at least one frame");
    NNPOPS_REQUIRE(num_segments >= 0 && num_segments <= std::numeric_limits<int32_t>::max() / 8, "Too many segments for getNeighborPairsFrames");
    NNPOPS_REQUIRE(cutoff > 0, "Expected \"cutoff\" to be positive");
    NNPOPS_REQUIRE(max_num_pairs > 0 || max_num_pairs == -1, "Expected \"max_num_pairs\" to be positive or equal to -1");
    NNPOPS_REQUIRE(num_slots >= 0 && (max_num_pairs == -1 || num_slots == max_num_pairs),
                   "Expected \"num_slots\" to be \"max_num_pairs\", or the pairs of every frame's triangle when it is -1");
    NNPOPS_REQUIRE(num_slots <= std::numeric_limits<int32_t>::max(), "Too many pair slots for getNeighborPairsFrames");
    NNPOPS_REQUIRE(positions && num_pairs && segment_slots && workspace, "NULL device pointer");
    NNPOPS_REQUIRE(num_segments == 0 || table, "NULL device pointer");
    NNPOPS_REQUIRE(num_slots == 0 || (neighbors && deltas && distances), "NULL output pointer");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        return frames_forward_impl<float>(num_atoms, num_frames, num_segments, table, (const float*)positions, (const float*)boxes, cutoff,
                                          max_num_pairs == -1, num_slots, neighbors, (float*)deltas, (float*)distances, num_pairs,
                                          segment_slots, workspace, s);
    return frames_forward_impl<double>(num_atoms, num_frames, num_segments, table, (const double*)positions, (const double*)boxes, cutoff,
                                       max_num_pairs == -1, num_slots, neighbors, (double*)deltas, (double*)distances, num_pairs,
                                       segment_slots, workspace, s);
}

int64_t nnpops_neighbor_pairs_frames_box_backward_workspace_bytes(int num_segments) {
    return num_segments < 0 ? 0 : (int64_t)sizeof(double) * 9 * std::max(num_segments, 1);
}

int nnpops_neighbor_pairs_frames_box_backward(int dtype, int num_atoms, int num_frames, int num_segments, const int32_t* table,
                                              const int32_t* segment_slots, int64_t num_slots, const int32_t* neighbors,
                                              const void* positions, const void* boxes, const void* deltas, const void* distances,
                                              const void* grad_deltas, const void* grad_distances, void* grad_boxes, void* workspace,
                                              void* stream) {
    NNPOPS_REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (float32) or 1 (float64)");
    NNPOPS_REQUIRE(num_atoms > 0 && num_frames > 0 && num_segments >= 0 && num_slots >= 0, "bad sizes");
    NNPOPS_REQUIRE(positions && boxes && grad_boxes && workspace && segment_slots, "NULL device pointer");
    NNPOPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "the workspace must be 8-byte aligned");
    NNPOPS_REQUIRE(num_segments == 0 || table, "NULL device pointer");
    NNPOPS_REQUIRE(num_slots == 0 || (neighbors && deltas && distances && grad_deltas && grad_distances), "NULL device pointer");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == 0)
        frames_box_backward_impl<float>(num_atoms, num_frames, num_segments, table, segment_slots, num_slots, neighbors, positions, boxes,
                                        deltas, distances, grad_deltas, grad_distances, grad_boxes, (double*)workspace, s);
    else
        frames_box_backward_impl<double>(num_atoms, num_frames, num_segments, table, segment_slots, num_slots, neighbors, positions, boxes,
                                         deltas, distances, grad_deltas, grad_distances, grad_boxes, (double*)workspace, s);
    NNPOPS_HIP_TRY(hipGetLastError());
    return NNPOPS_OK;
}

}  // extern "C"
