// What the loss kernels share (ln_nll.hip, ln_dice.hip, ln_lovasz.hip, ln_iou.hip): how a cloud-major batch of n rows is cut into clouds,
// and the fixed-order sum of a 256-thread workgroup.  (The 64-lane shuffle sum stays written out where it is used: as a function of its
// own it changed the order of the instructions around it.)  Argument checks and their error codes stay in each file.
#pragma once
#include "ln_common.h"

// Cloud b owns rows [b n0, min((b + 1) n0, n)): only the last cloud may be shorter.
struct LnCloudRange {
    long long first, len;
};
__device__ __forceinline__ LnCloudRange ln_cloud_range(long long n, long long n0, long long cloud) {
    LnCloudRange r;
    r.first = cloud * n0;
    r.len = n - r.first < n0 ? n - r.first : n0;
    return r;
}

// Rows of a full cloud and the clouds of n rows.  Total: any argument gives a split (a negative n counts as 0, points_per_cloud is
// brought into [1, max(n, 1)]); n = 0 is one empty cloud.
struct LnCloudSplit {
    long long n0, clouds;
};
static inline LnCloudSplit ln_cloud_split(long long n, long long points_per_cloud) {
    const size_t N = n > 0 ? size_t(n) : 0;
    const size_t P = points_per_cloud < 1 || N == 0 ? 1 : (size_t(points_per_cloud) > N ? N : size_t(points_per_cloud));
    return LnCloudSplit{(long long)P, (long long)(N == 0 ? 1 : (N + P - 1) / P)};
}

// fixed tree over a 256-thread workgroup: shuffle tree inside every wave, the four wave sums in order (valid in thread 0)
__device__ __forceinline__ float ln_block_sum_256(float x, float* s_w) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    float t = s_w[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) t += s_w[w];
    return t;
}
