// Cloud batches (LnTable.batch_points / batch_key_step): does every cloud stay inside its key band?  ln_simplex_of_cloud moves cloud c by
// c * batch_key_step along the first key coordinate and nothing else looks at the width of a cloud: one that is wider than its band shares
// vertices with its neighbour, gets neighbour-list entries that cross into it, and has rows decoded into the wrong cloud by
// k_cloud_row_starts.  The check is a launch sequence of its own, queued behind the build on the build's stream; the build kernels do
// not know about it.
//
//   k_cloud_extents_init   extents[c] = (INT_MAX, INT_MIN) for the B clouds, *first_bad = INT_MAX.
//   k_cloud_key_extents    one pass over the positions of the build (what k_point_keys reads; nothing but extents is written).  A thread
//                          locates the simplex of its point with ln_simplex, BEFORE ln_simplex_of_cloud, and takes the minimum and the
//                          maximum of the first key coordinate over the d + 1 vertices (ln_vertex_key).  The cloud is the grid's y
//                          coordinate: a workgroup never straddles two clouds and the shorter last cloud just has fewer live threads.
//                          Shuffle tree in the wave, four LDS words per bound, one atomicMin and one atomicMax per workgroup.  Integer
//                          atomics only: the result does not depend on the order of the workgroups and is bitwise reproducible.
//   k_cloud_key_extents_ranges   the same pass for clouds of unequal sizes (LnTableClouds.batch_point_starts): cloud y takes its own point range.
//   k_cloud_band_verdict   one workgroup over the B extents.  Cloud c is inside its band when -half + guard <= lo_c and hi_c < half - guard,
//                          half = batch_key_step >> 1; a cloud without a point (lo_c > hi_c) is inside.  On a violation: LN_STATUS_CLOUD_BAND
//                          is ORed into *t.status, the smallest offending cloud goes to *first_bad, and the build's report word in
//                          t.host_counters is stored again with the bit in it (count | status << 32 | seq << 40, the build's own form:
//                          the count and the other bits are read from the device words the build left).  Without a violation nothing
//                          but the init values is written.
#include "ln_simplex.h"

#include <limits.h>

#define LN_BAND_THREADS 256
#define LN_BAND_MAX_CLOUDS 65535  // grid y

__global__ void __launch_bounds__(LN_BAND_THREADS) k_cloud_extents_init(int* __restrict__ extents, int B, int* __restrict__ first_bad) {
    const int c = blockIdx.x * LN_BAND_THREADS + threadIdx.x;
    if (c < B) {
        extents[2 * c] = INT_MAX;
        extents[2 * c + 1] = INT_MIN;
    }
    if (c == 0) *first_bad = INT_MAX;
}

// (lo, hi) of the first key coordinate over the d + 1 simplex vertices of point p, folded into the running pair
template <int D>
__device__ __forceinline__ void ln_point_extent(const float* __restrict__ pos_raw, const LnScale<D>& sc, long long p, int& lo, int& hi) {
    float pr[D];
#pragma unroll
    for (int i = 0; i < D; ++i) pr[i] = pos_raw[(size_t)p * D + i];
    LnSimplex<D> s;
    ln_simplex<D>(pr, sc, s);
#pragma unroll
    for (int r = 0; r <= D; ++r) {
        int key[D];
        ln_vertex_key<D>(s, r, key);
        lo = min(lo, key[0]);
        hi = max(hi, key[0]);
    }
}

// workgroup reduction of (lo, hi) and the two atomics of the workgroup on the extents of cloud c
__device__ __forceinline__ void ln_extent_reduce(int lo, int hi, int c, int* __restrict__ extents) {
    __shared__ int s_lo[LN_BAND_THREADS / 64], s_hi[LN_BAND_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < LN_BAND_THREADS / 64; ++k) {
            lo = min(lo, s_lo[k]);
            hi = max(hi, s_hi[k]);
        }
        if (lo <= hi) {  // (a workgroup behind the end of a shorter last cloud, or of an empty cloud, has no point)
            atomicMin(&extents[2 * c], lo);
            atomicMax(&extents[2 * c + 1], hi);
        }
    }
}

template <int D>
__global__ void __launch_bounds__(LN_BAND_THREADS)
    k_cloud_key_extents(const float* __restrict__ pos_raw, LnScale<D> sc, int n, int batch_points, int* __restrict__ extents) {
    const int c = blockIdx.y;
    const long long local = (long long)blockIdx.x * LN_BAND_THREADS + threadIdx.x;
    const long long p = (long long)c * batch_points + local;
    int lo = INT_MAX, hi = INT_MIN;
    if (local < batch_points && p < n) ln_point_extent<D>(pos_raw, sc, p, lo, hi);
    ln_extent_reduce(lo, hi, c, extents);
}

// Clouds of unequal sizes (LnTableClouds.batch_point_starts): cloud c = blockIdx.y reduces its own range [starts[c], starts[c + 1]), clamped to
// [0, n] so that no list, however wrong, makes a thread read a position that is not there.  The grid's x extent is sized from the mean
// cloud (the host does not know the lengths) and the workgroups of a cloud stride over its range; an empty cloud keeps the empty extent.
template <int D>
__global__ void __launch_bounds__(LN_BAND_THREADS)
    k_cloud_key_extents_ranges(const float* __restrict__ pos_raw, LnScale<D> sc, int n, const int* __restrict__ starts,
                               int* __restrict__ extents) {
    const int c = blockIdx.y;
    const int first = min(max(starts[c], 0), n), last = min(max(starts[c + 1], first), n);
    int lo = INT_MAX, hi = INT_MIN;
    for (long long p = (long long)first + (long long)blockIdx.x * LN_BAND_THREADS + threadIdx.x; p < last;
         p += (long long)gridDim.x * LN_BAND_THREADS)
        ln_point_extent<D>(pos_raw, sc, p, lo, hi);
    ln_extent_reduce(lo, hi, c, extents);
}

__global__ void __launch_bounds__(LN_BAND_THREADS)
    k_cloud_band_verdict(LnTable t, const int* __restrict__ extents, int B, int guard, int* __restrict__ first_bad, bool report_starts) {
    __shared__ int s_bad[LN_BAND_THREADS / 64];
    const int half = t.batch_key_step >> 1;
    int bad = INT_MAX;
    for (int c = threadIdx.x; c < B; c += LN_BAND_THREADS) {
        const int lo = extents[2 * c], hi = extents[2 * c + 1];
        const bool inside = lo > hi || (lo >= -half + guard && hi < half - guard);
        if (!inside) bad = min(bad, c);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad = min(bad, __shfl_xor(bad, off, 64));
    if ((threadIdx.x & 63) == 0) s_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < LN_BAND_THREADS / 64; ++k) bad = min(bad, s_bad[k]);
        // (clouds of unequal sizes: a list that ln_cloud_point_starts_check, queued in front, found wrong is reported in the same word)
        const bool starts_bad = report_starts && (atomicOr(t.status, 0) & LN_STATUS_CLOUD_STARTS) != 0;
        if (bad != INT_MAX || starts_bad) {
            const int status = atomicOr(t.status, bad != INT_MAX ? LN_STATUS_CLOUD_BAND : 0) | (bad != INT_MAX ? LN_STATUS_CLOUD_BAND : 0);
            if (bad != INT_MAX) atomicMin(first_bad, bad);
            if (t.host_counters) {
                const unsigned long long word = (unsigned long long)(unsigned int)*t.nr_filled | ((unsigned long long)(status & 0xFF) << 32) |
                                                ((unsigned long long)(t.host_seq & 0xFFFFFF) << 40);
                __hip_atomic_store(reinterpret_cast<unsigned long long*>(t.host_counters), word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

extern "C" int ln_cloud_key_extents(const LnTable* t, const float* positions_raw, const float* sigmas_host, int n, int guard, int* extents,
                                    int* first_bad, void* stream) {
    LN_REQUIRE(t != nullptr, LN_ERR_ARG, "ln_cloud_key_extents: null table");
    LN_REQUIRE(t->pos_dim >= 1 && t->pos_dim <= LN_MAX_POS_DIM, LN_ERR_UNSUPPORTED, "ln_cloud_key_extents: pos_dim %d unsupported", t->pos_dim);
    LN_REQUIRE((t->batch_points > 0 || t->batch_points == LN_BATCH_POINT_STARTS) && t->batch_key_step >= 2, LN_ERR_ARG,
               "ln_cloud_key_extents: the table holds no batch of clouds");
    LN_REQUIRE(t->nr_filled && t->status, LN_ERR_ARG, "ln_cloud_key_extents: table has a null buffer");
    LN_REQUIRE(n >= 0 && positions_raw && sigmas_host && extents && first_bad, LN_ERR_ARG, "ln_cloud_key_extents: null buffer or n < 0");
    const int half = t->batch_key_step >> 1;
    LN_REQUIRE(guard >= 0 && guard < half, LN_ERR_ARG, "ln_cloud_key_extents: guard %d outside [0, %d) (half of batch_key_step)", guard, half);
    LN_REQUIRE(ln_cloud_starts_ok(t), LN_ERR_ARG, "ln_cloud_key_extents: LN_BATCH_POINT_STARTS without a list of point starts (batch_clouds >= 1)");
    const LnCloudStarts cs = ln_cloud_starts_of(t);
    const int* starts = cs.starts;
    const long long B = starts ? cs.clouds : ((long long)n + t->batch_points - 1) / t->batch_points;
    LN_REQUIRE(B <= LN_BAND_MAX_CLOUDS, LN_ERR_UNSUPPORTED, "ln_cloud_key_extents: %lld clouds, at most %d (the cloud is the y coordinate of the grid)",
               B, LN_BAND_MAX_CLOUDS);
    if (B == 0) return LN_OK;  // no point, no cloud: nothing to write
    hipStream_t st = (hipStream_t)stream;
    LN_LAUNCH("k_cloud_extents_init", k_cloud_extents_init, dim3(ln_div_up(B, LN_BAND_THREADS)), dim3(LN_BAND_THREADS), 0, st, extents, int(B),
              first_bad);
    // equal sizes: the workgroups of one cloud; unequal sizes: those of two mean clouds, which stride over the cloud's own range
    const long long per_cloud = starts ? 2 * ln_div_up((long long)n, B) : (t->batch_points < n ? t->batch_points : n);
    const dim3 grid(per_cloud > 0 ? ln_div_up(per_cloud, LN_BAND_THREADS) : 1, (unsigned)B), thr(LN_BAND_THREADS);
    switch (t->pos_dim) {
#define LN_BAND_CASE(DD)                                                                                                               \
    case DD:                                                                                                                           \
        if (starts)                                                                                                                    \
            LN_LAUNCH("k_cloud_key_extents_ranges", k_cloud_key_extents_ranges<DD>, grid, thr, 0, st, positions_raw,                  \
                      ln_make_scale<DD>(sigmas_host), n, starts, extents);                                                            \
        else                                                                                                                           \
            LN_LAUNCH("k_cloud_key_extents", k_cloud_key_extents<DD>, grid, thr, 0, st, positions_raw, ln_make_scale<DD>(sigmas_host), \
                      n, t->batch_points, extents);                                                                                    \
        break
        LN_BAND_CASE(1);
        LN_BAND_CASE(2);
        LN_BAND_CASE(3);
        LN_BAND_CASE(4);
        LN_BAND_CASE(5);
        LN_BAND_CASE(6);
#undef LN_BAND_CASE
    }
    LN_LAUNCH("k_cloud_band_verdict", k_cloud_band_verdict, dim3(1), thr, 0, st, *t, (const int*)extents, int(B), guard, first_bad, starts != nullptr);
    return ln_check_launch("ln_cloud_key_extents");
}

// LnTableClouds.batch_point_starts, verified where it lives: one workgroup walks the clouds + 1 ints.
__global__ void __launch_bounds__(LN_BAND_THREADS) k_cloud_point_starts_check(const int* __restrict__ starts, int clouds, int n, int* __restrict__ status) {
    bool bad = false;
    for (int c = threadIdx.x; c < clouds; c += LN_BAND_THREADS) bad |= starts[c] > starts[c + 1];
    if (threadIdx.x == 0) bad |= starts[0] != 0 || starts[clouds] != n;
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(status, LN_STATUS_CLOUD_STARTS);
}

extern "C" int ln_cloud_point_starts_check(const int* starts, int clouds, int n, int* status, void* stream) {
    LN_REQUIRE(starts && status, LN_ERR_ARG, "ln_cloud_point_starts_check: null starts or status");
    LN_REQUIRE(clouds >= 1 && n >= 0, LN_ERR_ARG, "ln_cloud_point_starts_check: clouds %d < 1 or n %d < 0", clouds, n);
    LN_LAUNCH("k_cloud_point_starts_check", k_cloud_point_starts_check, dim3(1), dim3(LN_BAND_THREADS), 0, (hipStream_t)stream, starts, clouds, n,
              status);
    return ln_check_launch("ln_cloud_point_starts_check");
}
