// What the loss kernels share (ln_nll.hip, ln_dice.hip, ln_lovasz.hip, ln_iou.hip): how a cloud-major batch of n rows is cut into clouds,
// and the fixed-order sum of a 256-thread workgroup.  (The 64-lane shuffle sum stays written out where it is used: as a function of its
// own it changed the order of the instructions around it.)  Argument checks and their error codes stay in each file.
#pragma once
#include "ln_common.h"

// Clouds of equal sizes: cloud b owns rows [b n0, min((b + 1) n0, n)), only the last cloud may be shorter.
struct LnCloudRange {
    long long first, len;
};
__device__ __forceinline__ LnCloudRange ln_cloud_range(long long n, long long n0, long long cloud) {
    LnCloudRange r;
    r.first = cloud * n0;
    r.len = n - r.first < n0 ? n - r.first : n0;
    return r;
}

// The two ways a batch is cut.  A kernel that walks a cloud takes its cut as a template parameter CUT — the rows of a full cloud (an integer:
// the range above) or LnCloudsListed — and the HOST picks the instance (the precedent of the ragged build, ln_simplex.h: a uniform branch
// on the pointer inside one kernel cost k_point_keys 0.3 - 0.45 us).  The instances of the equal-size entry points never see a list.
//
// Clouds of unequal sizes: cloud b owns rows [starts[b], starts[b + 1]) of clouds + 1 ascending ints from 0 to n (the list of
// LnTableClouds.batch_point_starts), none longer than `longest`, by which the host sizes grids and workspace strides.  The range is clamped
// into [0, n] and its length to `longest`: whatever the list holds, a kernel stays inside the n rows and inside its cloud's share of the
// workspace.  starts[b] == starts[b + 1] is a cloud of no rows.
struct LnCloudsListed {
    const int* starts;
    long long longest;
};
__device__ __forceinline__ LnCloudRange ln_cloud_range(long long n, LnCloudsListed cut, long long cloud) {
    long long lo = cut.starts[cloud], hi = cut.starts[cloud + 1];
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
    LnCloudRange r;
    r.first = lo;
    r.len = hi - lo < cut.longest ? hi - lo : cut.longest;
    return r;
}
// The cloud of a row, for the elementwise backward kernels (their template parameter CLOUD_OF: a division by n0, or this): the binary
// search of the build (ln_common.h), which steps over empty clouds.
struct LnCloudOfRowListed {
    const int* starts;
    int clouds;
};
__device__ __forceinline__ int ln_cloud_of_row(int row, LnCloudOfRowListed list) { return ln_cloud_of_point(list.starts, list.clouds, row); }

// What a _ranges entry point checks of (point_starts, clouds, longest) before anything else; `max_clouds` is the grid limit of its family.
#define LN_REQUIRE_CLOUD_LIST(who, n, point_starts, clouds, longest, max_clouds, limit_code)                                                 \
    do {                                                                                                                                    \
        LN_REQUIRE((point_starts) != nullptr, LN_ERR_ARG, "%s: null point_starts", who);                                                    \
        LN_REQUIRE((clouds) >= 1, LN_ERR_ARG, "%s: bad sizes (clouds >= 1)", who);                                                          \
        LN_REQUIRE((clouds) <= (max_clouds), limit_code, "%s: %d clouds, at most %d (the cloud is a coordinate of the grid)", who, int(clouds), \
                   int(max_clouds));                                                                                                        \
        LN_REQUIRE((longest) >= 0 && (longest) <= (n), LN_ERR_ARG, "%s: bad sizes (0 <= longest <= n)", who);                               \
    } while (0)

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
