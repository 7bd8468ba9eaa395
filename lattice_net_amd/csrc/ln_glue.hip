// Launch diet of the glue around the lattice operators in a training step: pieces the reference writes as
// chains of torch broadcasting operators on tiny or token-sized tensors, each a launch of its own.
//
//  * weight normalisation (utils.py:72-158 weight_norm_wrapper with v_dim=None, used by LinearWN / ConvLatticeIm2RowWN / ...):
//        w = v * g / ||v||_F                   (g: one magnitude per row or per column of v)
//    forward = norm + div + mul, backward ~10 elementwise / reduction launches on a parameter of a few thousand numbers.
//    Here: one workgroup forward, one workgroup backward, sums in a fixed order (deterministic).
//        grad_g[j] = sum_k gw[j,k] v[j,k] / n
//        grad_v    = gw * g / n  -  v * (sum_j g[j] sum_k gw[j,k] v[j,k]) / n^3
//
//  * DistributeLatticeModule (lattice_modules.py:72-94): per token, positions minus the mean position of the token's vertex, rows
//    of the tokens of vertex 0 (the "invalid" bucket, also every token that found no vertex) zeroed:
//        out[t, :D] = d[t, :D] - sums[idx[t]] / max(count[idx[t]], 1),  out[t, D:] = d[t, D:]     (idx[t] > 0; zeros otherwise)
//    in one pass instead of div / clamp / index_select / sub / cat / eq / masked_fill.
#include "ln_common.h"
#include "ln_simplex.h"

#define LN_WN_THREADS 1024
#define LN_WN_MAX_G 1024

// element (j, k): j indexes g, k the other dimension of v [R, C]
//   g_dim == 0 (g per row):    address j * C + k, K = C
//   g_dim == 1 (g per column): address k * C + j, K = R
struct LnWnShape {
    int J, K, sj, sk;
    int C, per_col;  // row width of v [R, C] and "g runs along the columns" — stated, not inferred from the strides (sj == 1 also holds for
                     // g_dim 0 with one column)
};

__device__ __forceinline__ float ln_wn_block_sum(float x, float* s_red) {
    // fixed tree over the 1024 threads: wave sums by DPP-free shuffles, then 16 wave totals in LDS
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();  // s_red may still be read from a previous call
    if ((threadIdx.x & 63) == 0) s_red[wave] = x;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < LN_WN_THREADS / 64; ++w) t += s_red[w];
    return t;
}

__global__ void __launch_bounds__(LN_WN_THREADS)
    k_weight_norm_forward(const float* __restrict__ v, const float* __restrict__ g, LnWnShape s, float* __restrict__ w,
                          float* __restrict__ norm_out) {
    __shared__ float s_red[LN_WN_THREADS / 64];
    const long long total = (long long)s.J * s.K;
    float acc = 0.f;
    for (long long i = threadIdx.x; i < total; i += LN_WN_THREADS) {
        const float x = v[i];
        acc += x * x;
    }
    const float n = sqrtf(ln_wn_block_sum(acc, s_red));
    if (threadIdx.x == 0) norm_out[0] = n;
    // plain [R, C] walk: i = row * C + col; j = row (g_dim 0) or col (g_dim 1)
    const int C = s.C;
    for (long long i = threadIdx.x; i < total; i += LN_WN_THREADS) {
        const int row = int(i / C), col = int(i - (long long)row * C);
        const int j = s.per_col ? col : row;
        w[i] = v[i] * (g[j] / n);
    }
}

__global__ void __launch_bounds__(LN_WN_THREADS)
    k_weight_norm_backward(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ gw,
                           const float* __restrict__ norm, LnWnShape s, float* __restrict__ gv, float* __restrict__ gg) {
    __shared__ float s_part[LN_WN_THREADS];
    __shared__ float s_dot[LN_WN_MAX_G];
    __shared__ float s_red[LN_WN_THREADS / 64];
    const float n = norm[0];
    const int lanes = LN_WN_THREADS / s.J;  // threads per g entry
    const int kl = threadIdx.x / s.J;
    const int j = threadIdx.x - kl * s.J;
    float acc = 0.f;
    if (kl < lanes)
        for (int k = kl; k < s.K; k += lanes) {
            const long long a = (long long)j * s.sj + (long long)k * s.sk;
            acc += gw[a] * v[a];
        }
    s_part[threadIdx.x] = acc;
    __syncthreads();
    float mine = 0.f;
    if (threadIdx.x < s.J) {
        float d = 0.f;
        for (int l = 0; l < lanes; ++l) d += s_part[l * s.J + threadIdx.x];
        s_dot[threadIdx.x] = d;
        gg[threadIdx.x] = d / n;
        mine = d * g[threadIdx.x];
    }
    const float t = ln_wn_block_sum(mine, s_red);  // sum_j g[j] * dot[j]
    const float dn_over_n = -t / (n * n * n);       // (dL/dn) / n
    const long long total = (long long)s.J * s.K;
    const int C = s.C;
    for (long long i = threadIdx.x; i < total; i += LN_WN_THREADS) {
        const int row = int(i / C), col = int(i - (long long)row * C);
        const int jj = s.per_col ? col : row;
        gv[i] = gw[i] * (g[jj] / n) + v[i] * dn_over_n;
    }
}

static int ln_wn_shape(const char* who, int rows, int cols, int g_dim, LnWnShape& s) {
    LN_REQUIRE(rows >= 1 && cols >= 1 && (g_dim == 0 || g_dim == 1), LN_ERR_ARG, "%s: bad sizes", who);
    s = g_dim == 0 ? LnWnShape{rows, cols, cols, 1, cols, 0} : LnWnShape{cols, rows, 1, cols, cols, 1};
    LN_REQUIRE(s.J <= LN_WN_MAX_G, LN_ERR_UNSUPPORTED, "%s: at most %d magnitudes (got %d)", who, LN_WN_MAX_G, s.J);
    LN_REQUIRE((long long)rows * cols <= (1ll << 24), LN_ERR_UNSUPPORTED, "%s: parameter too large for the one-workgroup form", who);
    return LN_OK;
}

extern "C" int ln_weight_norm_forward(const float* v, const float* g, int rows, int cols, int g_dim, float* w, float* norm, void* stream) {
    LnWnShape s;
    int rc = ln_wn_shape("ln_weight_norm_forward", rows, cols, g_dim, s);
    if (rc) return rc;
    LN_REQUIRE(v && g && w && norm, LN_ERR_ARG, "ln_weight_norm_forward: null buffer");
    LN_LAUNCH("k_weight_norm_forward", k_weight_norm_forward, dim3(1), dim3(LN_WN_THREADS), 0, (hipStream_t)stream, v, g, s, w, norm);
    return ln_check_launch("ln_weight_norm_forward");
}

extern "C" int ln_weight_norm_backward(const float* v, const float* g, const float* grad_w, const float* norm, int rows, int cols, int g_dim,
                                       float* grad_v, float* grad_g, void* stream) {
    LnWnShape s;
    int rc = ln_wn_shape("ln_weight_norm_backward", rows, cols, g_dim, s);
    if (rc) return rc;
    LN_REQUIRE(v && g && grad_w && norm && grad_v && grad_g, LN_ERR_ARG, "ln_weight_norm_backward: null buffer");
    LN_LAUNCH("k_weight_norm_backward", k_weight_norm_backward, dim3(1), dim3(LN_WN_THREADS), 0, (hipStream_t)stream, v, g, grad_w, norm, s,
              grad_v, grad_g);
    return ln_check_launch("ln_weight_norm_backward");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// thread = (token, column); 256 threads walk consecutive elements of out (coalesced); the per-vertex rows come from L2.
// One body for the three kernels: IDX is int when every element index fits 31 bits (32-bit divisions), else long long, and FIRST names
// the "invalid" vertex of token t, whose tokens are zeroed with those that found no vertex — the first row of the token's cloud.  The
// cloud comes from t alone (cloud_of); its first row is read only for a token that found a vertex (first_row):
//  * LnFirstRowZero: no batch, row 0 of the table.
//  * LnFirstRowEqualClouds: a batch of clouds in one table (LnTable.batch_points); the first vertex of EVERY cloud is invalid,
//    row_starts[cloud] (ln_cloud_row_starts), and token t belongs to cloud min(t / tokens_per_cloud, clouds - 1).  A wave reads one or
//    two of the at most 1025 ints: one cache line.
//    (Measured and dropped: row_starts in LDS behind a barrier, and cloud / boundary / first rows computed once per workgroup — both slower.)
//  * LnFirstRowListedClouds: clouds of unequal sizes (LnTableClouds.batch_point_starts); the cloud of token t is that of its point
//    t / tokens_per_point, found by the binary search of the key pass (ln_cloud_of_point: reads inside the list and returns a cloud in
//    [0, clouds) whatever the list holds).
struct LnFirstRowZero {
    template <typename IDX> __device__ __forceinline__ int cloud_of(IDX) const { return 0; }
    __device__ __forceinline__ int first_row(int) const { return 0; }
};
struct LnFirstRowEqualClouds {
    long long tokens_per_cloud;
    const int* row_starts;
    int clouds;
    template <typename IDX> __device__ __forceinline__ int cloud_of(IDX t) const {
        const IDX cloud = t / (IDX)tokens_per_cloud;
        return cloud < (IDX)(clouds - 1) ? (int)cloud : clouds - 1;
    }
    __device__ __forceinline__ int first_row(int cloud) const { return row_starts[cloud]; }
};
struct LnFirstRowListedClouds {
    int tokens_per_point;
    const int* point_starts;
    const int* row_starts;
    int clouds;
    template <typename IDX> __device__ __forceinline__ int cloud_of(IDX t) const {
        return ln_cloud_of_point(point_starts, clouds, int(t / (IDX)tokens_per_point));
    }
    __device__ __forceinline__ int first_row(int cloud) const { return row_starts[cloud]; }
};

template <typename IDX, class FIRST>
__device__ __forceinline__ void ln_distribute_centre_body(const float* __restrict__ d, const int* __restrict__ idx, const float* __restrict__ sums,
                                                          const int* __restrict__ counts, long long tokens, int width, int pos_dim, FIRST first,
                                                          float* __restrict__ out) {
    const long long i64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i64 >= tokens * width) return;
    const IDX i = (IDX)i64;
    const IDX t = i / (IDX)width;
    const int c = int(i - t * (IDX)width);
    const int cloud = first.cloud_of(t);
    const int row = idx[t];
    float x = 0.f;
    if (row >= 0 && row != first.first_row(cloud)) {
        x = d[i64];
        if (c < pos_dim) x -= sums[(size_t)row * pos_dim + c] / (float)max(counts[row], 1);
    }
    out[i64] = x;
}

__global__ void __launch_bounds__(256)
    k_distribute_centre(const float* __restrict__ d, const int* __restrict__ idx, const float* __restrict__ sums,
                        const int* __restrict__ counts, long long tokens, int width, int pos_dim, float* __restrict__ out) {
    ln_distribute_centre_body<long long>(d, idx, sums, counts, tokens, width, pos_dim, LnFirstRowZero{}, out);
}

template <typename IDX>
__global__ void __launch_bounds__(256)
    k_distribute_centre_clouds(const float* __restrict__ d, const int* __restrict__ idx, const float* __restrict__ sums,
                               const int* __restrict__ counts, long long tokens, int width, int pos_dim, long long tokens_per_cloud,
                               const int* __restrict__ row_starts, int clouds, float* __restrict__ out) {
    ln_distribute_centre_body<IDX>(d, idx, sums, counts, tokens, width, pos_dim, LnFirstRowEqualClouds{tokens_per_cloud, row_starts, clouds}, out);
}

template <typename IDX>
__global__ void __launch_bounds__(256)
    k_distribute_centre_cloud_starts(const float* __restrict__ d, const int* __restrict__ idx, const float* __restrict__ sums,
                                     const int* __restrict__ counts, long long tokens, int width, int pos_dim, int tokens_per_point,
                                     const int* __restrict__ point_starts, const int* __restrict__ row_starts, int clouds,
                                     float* __restrict__ out) {
    ln_distribute_centre_body<IDX>(d, idx, sums, counts, tokens, width, pos_dim,
                                   LnFirstRowListedClouds{tokens_per_point, point_starts, row_starts, clouds}, out);
}

extern "C" int ln_distribute_centre(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                    long long tokens, int width, int pos_dim, float* out, void* stream) {
    LN_REQUIRE(tokens >= 0 && width >= 1 && pos_dim >= 0 && pos_dim <= width, LN_ERR_ARG, "ln_distribute_centre: bad sizes");
    if (tokens == 0) return LN_OK;
    LN_REQUIRE(distributed && splat_idx && position_sums && counts && out, LN_ERR_ARG, "ln_distribute_centre: null buffer");
    LN_LAUNCH("k_distribute_centre", k_distribute_centre, dim3(ln_div_up(tokens * width, 256)), dim3(256), 0, (hipStream_t)stream, distributed,
              splat_idx, position_sums, counts, tokens, width, pos_dim, out);
    return ln_check_launch("ln_distribute_centre");
}

// The four cloud entry points: `per` is tokens_per_cloud, or for the entry points that take a list of point starts (`listed`) tokens_per_point.
// The kernels read the starts from global memory, any number of them: the plain and the _many entry points differ in the limit they check.
static int ln_distribute_centre_clouds_run(const char* who, int max_clouds, bool listed, const float* distributed, const int* splat_idx,
                                           const float* position_sums, const int* counts, long long tokens, int width, int pos_dim, long long per,
                                           const int* point_starts, const int* row_starts, int clouds, float* out, void* stream) {
    LN_REQUIRE(tokens >= 0 && width >= 1 && pos_dim >= 0 && pos_dim <= width && per >= 1, LN_ERR_ARG, "%s: bad sizes", who);
    LN_REQUIRE(!listed || tokens / per <= 0x7fffffffll, LN_ERR_ARG, "%s: more than 2^31 points", who);
    LN_REQUIRE(clouds >= 1 && clouds <= max_clouds, LN_ERR_UNSUPPORTED, "%s: 1 <= clouds <= %d (got %d)", who, max_clouds, clouds);
    LN_REQUIRE(!listed || point_starts != nullptr, LN_ERR_ARG, "%s: null point_starts", who);
    if (tokens == 0) return LN_OK;
    LN_REQUIRE(distributed && splat_idx && position_sums && counts && row_starts && out, LN_ERR_ARG, "%s: null buffer", who);
    const dim3 grid(ln_div_up(tokens * width, 256));
    const bool narrow = tokens * width <= 0x7fffffffll && (listed || per <= 0x7fffffffll);  // int: every element index, and the divisor, fit 31 bits
    if (listed) {
        const auto kernel = narrow ? k_distribute_centre_cloud_starts<int> : k_distribute_centre_cloud_starts<long long>;
        LN_LAUNCH("k_distribute_centre_cloud_starts", kernel, grid, dim3(256), 0, (hipStream_t)stream, distributed, splat_idx, position_sums, counts,
                  tokens, width, pos_dim, (int)per, point_starts, row_starts, clouds, out);
    } else {
        const auto kernel = narrow ? k_distribute_centre_clouds<int> : k_distribute_centre_clouds<long long>;
        LN_LAUNCH("k_distribute_centre_clouds", kernel, grid, dim3(256), 0, (hipStream_t)stream, distributed, splat_idx, position_sums, counts, tokens,
                  width, pos_dim, per, row_starts, clouds, out);
    }
    return ln_check_launch(who);
}

extern "C" int ln_distribute_centre_clouds(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                           long long tokens, int width, int pos_dim, long long tokens_per_cloud, const int* row_starts,
                                           int clouds, float* out, void* stream) {
    return ln_distribute_centre_clouds_run("ln_distribute_centre_clouds", LN_CLOUDS_MAX, false, distributed, splat_idx, position_sums, counts, tokens,
                                           width, pos_dim, tokens_per_cloud, nullptr, row_starts, clouds, out, stream);
}

extern "C" int ln_distribute_centre_many_clouds(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                                long long tokens, int width, int pos_dim, long long tokens_per_cloud, const int* row_starts,
                                                int clouds, float* out, void* stream) {
    return ln_distribute_centre_clouds_run("ln_distribute_centre_many_clouds", LN_CLOUDS_MANY_MAX, false, distributed, splat_idx, position_sums, counts,
                                           tokens, width, pos_dim, tokens_per_cloud, nullptr, row_starts, clouds, out, stream);
}

extern "C" int ln_distribute_centre_cloud_starts(const float* distributed, const int* splat_idx, const float* position_sums, const int* counts,
                                                 long long tokens, int width, int pos_dim, int tokens_per_point, const int* point_starts,
                                                 const int* row_starts, int clouds, float* out, void* stream) {
    return ln_distribute_centre_clouds_run("ln_distribute_centre_cloud_starts", LN_CLOUDS_MAX, true, distributed, splat_idx, position_sums, counts, tokens,
                                           width, pos_dim, tokens_per_point, point_starts, row_starts, clouds, out, stream);
}

extern "C" int ln_distribute_centre_many_cloud_starts(const float* distributed, const int* splat_idx, const float* position_sums,
                                                      const int* counts, long long tokens, int width, int pos_dim, int tokens_per_point,
                                                      const int* point_starts, const int* row_starts, int clouds, float* out, void* stream) {
    return ln_distribute_centre_clouds_run("ln_distribute_centre_many_cloud_starts", LN_CLOUDS_MANY_MAX, true, distributed, splat_idx, position_sums,
                                           counts, tokens, width, pos_dim, tokens_per_point, point_starts, row_starts, clouds, out, stream);
}
