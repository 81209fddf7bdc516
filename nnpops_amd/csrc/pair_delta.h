// pair_delta.h -- the displacement of a pair under the minimum image of a triclinic box and its squared length, as the all-pairs
// searches of neighbor_pairs.hip form them.  Shared with pme_frames.hip, whose direct term must keep exactly the pairs
// getNeighborPairsFrames lists.
#pragma once

namespace {

template <typename T> struct Vec3 { T x, y, z; };

// pos[row] - pos[col], wrapped z, then y, then x (one round each)
template <typename T>
__device__ __forceinline__ Vec3<T> wrapped_delta(const T* __restrict__ pos, int row, int col, const T* __restrict__ box,
                                                 bool periodic) {
    Vec3<T> d{pos[3 * row] - pos[3 * col], pos[3 * row + 1] - pos[3 * col + 1], pos[3 * row + 2] - pos[3 * col + 2]};
    if (periodic) {
        const T s3 = round(d.z / box[8]);
        d.x -= s3 * box[6]; d.y -= s3 * box[7]; d.z -= s3 * box[8];
        const T s2 = round(d.y / box[4]);
        d.x -= s2 * box[3]; d.y -= s2 * box[4];
        const T s1 = round(d.x / box[0]);
        d.x -= s1 * box[0];
    }
    return d;
}

// |d|^2 with the roundings of pairs_allpairs.  Its float32 sum is compiled as two rounded products and one fused step,
// (fma(y, y, x * x)) + z * z; without packed arithmetic the same source line would fuse twice, so the steps are spelled out here.
// float64 has one compiled form, the source line's.
template <typename T>
__device__ __forceinline__ T allpairs_norm2(const Vec3<T>& d) { return d.x * d.x + d.y * d.y + d.z * d.z; }
template <>
__device__ __forceinline__ float allpairs_norm2<float>(const Vec3<float>& d) {
#pragma clang fp contract(off)
    const float xx = d.x * d.x, zz = d.z * d.z;
    const float xy = __builtin_fmaf(d.y, d.y, xx);
    return xy + zz;
}

}  // namespace
