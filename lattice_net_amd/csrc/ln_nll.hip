// Mean negative log-likelihood of a cloud-major batch, forward value and the gradient wrt the log-probabilities: every NLL kernel of the
// library.  Two forward entry points into one host function (ln_nllc_forward), two backward ones into another:
//   ln_nll_forward_clouds / ln_nll_backward_clouds   class weights, per cloud (torch.nn.NLLLoss(weight=, ignore_index=) on every cloud, the
//                                                    mean over the clouds);
//   ln_nll_forward / ln_nll_backward                 the loss of the training loop: one cloud of all n rows, no weights, no mean over the
//                                                    clouds — per_cloud and weight_sum are the two words of loss_count.
//
//   ln_nll_forward_ranges / ln_nll_backward_ranges   the first pair for clouds of unequal sizes: cloud b owns the rows point_starts[b] ..
//                                                    point_starts[b + 1] of a device list (LnCloudsListed, ln_loss_common.h); the same
//                                                    kernels, instantiated on the list, grids and strides by the longest cloud.
//
// Cloud b owns rows [b n0, min((b + 1) n0, n)), B = ceil(n / n0).  A label counts when it differs from ignore_index; labels outside
// [0, C) are clamped and take the weight of the class they clamp to; w = 1 without class weights.  Per cloud
//     N_b = sum_counted w[y_i] lp[i, y_i],   W_b = sum_counted w[y_i],   D_b = W_b != 0 ? W_b : 1
//     per_cloud[b] = -N_b / D_b,   weight_sum[b] = D_b,   loss = (sum_b per_cloud[b]) / B
//     d loss / d lp[i, y_i] = -grad_loss w[y_i] / (B D_b)  on the counted rows, 0 everywhere else.
// log_probs is read at (counted row, clamped label) only and class_weight at the clamped label of a counted row only.
//
// Arithmetic, pinned so that tests/glue_reference.py (nll_emulate_cloud) can count its roundings and repeat its order: every sum in a
// fixed order, no float atomics, IEEE division, no contraction (-ffp-contract=off).  A cloud of len rows is cut into
// blocks = clamp(ceil(len / 1024), 1, 512) workgroups of 256 threads, grid-stride by blocks * 256, the shuffle tree of a wave,
// (s0 + s1) + (s2 + s3) over the four waves, then the finish: partial t in lane t of a 512-lane layout, the shuffle tree of each of its
// 8 waves, the 8 wave totals added in order from 0.  The sum depends on the cloud's rows alone: a cloud of a batch and a one-cloud call of
// the same rows run the same code and give the same bits.
//
//   k_nll_clouds_wave      n0 <= 64: a wave per cloud, four clouds per workgroup, no LDS and no barrier.  One row per lane; the other three
//                          waves of the 256-thread layout and the 511 other lanes of the finish would add +0, which changes no bit (an
//                          accumulator that starts at +0 is never -0).  Writes per_cloud / weight_sum itself.  A cloud of no rows (the
//                          one-cloud entry at n = 0) reads nothing and publishes -0 / 1.
//   k_nll_clouds_partials  grid (blocks of the longest cloud, clouds): a workgroup takes part of ONE cloud; workgroups behind a cloud's
//                          last block leave.  n0 <= 1024 (one block per cloud): writes per_cloud / weight_sum itself, by the same
//                          argument; otherwise one (N, W) partial per workgroup.
//   k_nll_clouds_finish    16 waves.  Phase 1 (n0 > 1024): a wave per cloud, the finish above by 8 loads per lane and 8 shuffle trees, no
//                          LDS.  Phase 2: the clouds strided over the 1024 threads in series, the shuffle tree of every wave, the 16 wave
//                          totals in order, / B.  Up to LN_NLLC_FUSED_CLOUDS clouds one workgroup runs both phases (two launches
//                          forward); more clouds of more than 1024 rows take phase 1 on a grid and phase 2 in a launch of its own.  The
//                          one-cloud entry never runs phase 2: its sum starts from +0 and would turn the -0 of a call without a counted
//                          label into +0.
//   k_nll_clouds_backward  elementwise, every element of [n, C] written.
#include "ln_loss_common.h"

#define LN_NLLC_BLOCKS 512        // workgroups of a cloud at the most; ln_nll_workspace_bytes holds their partials
#define LN_NLLC_THREADS 256
#define LN_NLLC_ROWS_PER_BLOCK 1024
#define LN_NLLC_WAVE_ROWS 64      // clouds up to this many rows: a wave per cloud
#define LN_NLLC_FINISH_THREADS 1024
#define LN_NLLC_FINISH_WAVES (LN_NLLC_FINISH_THREADS / 64)
#define LN_NLLC_FUSED_CLOUDS 64   // clouds whose phase 1 the single finishing workgroup takes (4 per wave)
#define LN_NLLC_MAX_CLOUDS 65535  // grid y

// blocks of a cloud of len rows
LN_HD int ln_nllc_blocks(long long len) {
    const long long b = (len + LN_NLLC_ROWS_PER_BLOCK - 1) / LN_NLLC_ROWS_PER_BLOCK;
    return b < 1 ? 1 : (b > LN_NLLC_BLOCKS ? LN_NLLC_BLOCKS : int(b));
}

// one row of a cloud: adds w lp and w (or lp and 1) when the label counts
template <bool WEIGHTED>
__device__ __forceinline__ void ln_nllc_row(const float* __restrict__ lp, const long long* __restrict__ target, long long row, int C,
                                            long long ignore_index, const float* __restrict__ cw, float& acc, float& wsum) {
    const long long t = target[row];
    if (t != ignore_index) {
        const long long tc = t < 0 ? 0 : (t >= C ? C - 1 : t);
        if (WEIGHTED) {
            const float w = cw[tc];
            acc += w * lp[row * C + tc];
            wsum += w;
        } else {
            acc += lp[row * C + tc];
            wsum += 1.f;
        }
    }
}

__device__ __forceinline__ void ln_nllc_publish(float a, float w, float* __restrict__ per_cloud, float* __restrict__ weight_sum, int b) {
    const float d = w != 0.f ? w : 1.f;  // (without weights: max(count, 1))
    per_cloud[b] = -a / d;
    weight_sum[b] = d;
}

// CUT, in every kernel that walks a cloud: how the batch is cut (ln_loss_common.h) — the rows of a full cloud (int here, long long below:
// the instances of the equal-size entry points), or LnCloudsListed (the _ranges entry points).  The host picks the instance.
template <bool WEIGHTED, class CUT>
__global__ void __launch_bounds__(LN_NLLC_THREADS)
    k_nll_clouds_wave(const float* __restrict__ lp, const long long* __restrict__ target, long long n, CUT cut, int C, int B,
                      long long ignore_index, const float* __restrict__ cw, float* __restrict__ per_cloud, float* __restrict__ weight_sum) {
    const int b = blockIdx.x * (LN_NLLC_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= B) return;  // (the whole wave; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    const LnCloudRange cloud = ln_cloud_range(n, cut, b);
    float acc = 0.f, wsum = 0.f;
    if (lane < cloud.len) ln_nllc_row<WEIGHTED>(lp, target, cloud.first + lane, C, ignore_index, cw, acc, wsum);
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off, 64);
        wsum += __shfl_down(wsum, off, 64);
    }
    if (lane == 0) ln_nllc_publish(acc, wsum, per_cloud, weight_sum, b);
}

template <int MODE, class CUT>  // bit 0: class weights; bit 1: one block per cloud, per_cloud / weight_sum written here
__global__ void __launch_bounds__(LN_NLLC_THREADS)
    k_nll_clouds_partials(const float* __restrict__ lp, const long long* __restrict__ target, long long n, CUT cut, int C,
                          long long ignore_index, const float* __restrict__ cw, float* __restrict__ partial, float* __restrict__ per_cloud,
                          float* __restrict__ weight_sum) {
    constexpr bool WEIGHTED = (MODE & 1) != 0, DIRECT = (MODE & 2) != 0;
    __shared__ float s_sum[4], s_cnt[4];
    const LnCloudRange cloud = ln_cloud_range(n, cut, blockIdx.y);
    const int blocks = ln_nllc_blocks(cloud.len);
    if ((int)blockIdx.x >= blocks) return;  // (the whole workgroup)
    float acc = 0.f, wsum = 0.f;
    for (long long i = (long long)blockIdx.x * LN_NLLC_THREADS + threadIdx.x; i < cloud.len; i += (long long)blocks * LN_NLLC_THREADS)
        ln_nllc_row<WEIGHTED>(lp, target, cloud.first + i, C, ignore_index, cw, acc, wsum);
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_down(acc, off, 64);
        wsum += __shfl_down(wsum, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = acc;
        s_cnt[threadIdx.x >> 6] = wsum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float a = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        const float w = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (DIRECT) {
            ln_nllc_publish(a, w, per_cloud, weight_sum, blockIdx.y);
        } else {
            float* out = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
            out[0] = a;
            out[1] = w;
        }
    }
}

template <int MODE, class CUT>  // bit 0: phase 1 (per cloud, from the partials); bit 1: phase 2 (the mean over the clouds)
__global__ void __launch_bounds__(LN_NLLC_FINISH_THREADS)
    k_nll_clouds_finish(const float* __restrict__ partial, long long n, CUT cut, int B, int grid_blocks, float* __restrict__ per_cloud,
                        float* __restrict__ weight_sum, float* __restrict__ loss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (MODE & 1) {
        for (int b = blockIdx.x * LN_NLLC_FINISH_WAVES + wave; b < B; b += gridDim.x * LN_NLLC_FINISH_WAVES) {
            const int blocks = ln_nllc_blocks(ln_cloud_range(n, cut, b).len);
            const float* p = partial + (long long)b * grid_blocks * 2;
            float x[LN_NLLC_BLOCKS / 64], y[LN_NLLC_BLOCKS / 64];
#pragma unroll
            for (int k = 0; k < LN_NLLC_BLOCKS / 64; ++k) {
                const int t = k * 64 + lane;
                x[k] = t < blocks ? p[2 * t] : 0.f;
                y[k] = t < blocks ? p[2 * t + 1] : 0.f;
            }
            float a = 0.f, w = 0.f;
#pragma unroll
            for (int k = 0; k < LN_NLLC_BLOCKS / 64; ++k) {
                // (a 64-lane chunk behind the cloud's last block holds +0 only and a, w are never -0: leaving it out changes no bit, and
                // sixteen waves at 96 shuffles each are what this workgroup's time was)
                if (k * 64 >= blocks) break;
                for (int off = 32; off > 0; off >>= 1) {
                    x[k] += __shfl_down(x[k], off, 64);
                    y[k] += __shfl_down(y[k], off, 64);
                }
                a += x[k];
                w += y[k];
            }
            if (lane == 0) ln_nllc_publish(a, w, per_cloud, weight_sum, b);
        }
    }
    if (MODE & 2) {
        __shared__ float s_w[LN_NLLC_FINISH_WAVES];
        if (MODE & 1) __syncthreads();  // per_cloud was written by this workgroup
        float acc = 0.f;
        for (int b = threadIdx.x; b < B; b += LN_NLLC_FINISH_THREADS) acc += per_cloud[b];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) s_w[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = s_w[0];
            for (int k = 1; k < LN_NLLC_FINISH_WAVES; ++k) t += s_w[k];
            loss[0] = t / float(B);
        }
    }
}

// x / d for 0 <= x < 2^31 and 1 <= d < 2^31 as a multiplication and a shift (Granlund & Montgomery 1994, N = 31): with l = ceil(log2 d)
// and m = ceil(2^(31 + l) / d) < 2^32,  2^(31 + l) <= m d < 2^(31 + l) + 2^l,  so  floor(x m / 2^(31 + l)) = floor(x / d).  The backward
// divides every element index twice (row, cloud); with two runtime divisions it took 7.1 us at 120 000 x 20 on an MI355X (a one-cloud
// kernel with one runtime division: 5.7 us), like this 5.4 us.
struct LnDivU31 {
    unsigned m;
    int shift;
};
static LnDivU31 ln_div_u31(long long d) {
    int l = 0;
    while ((1ll << l) < d) ++l;
    return LnDivU31{(unsigned)(((1ull << (31 + l)) + (unsigned long long)d - 1) / (unsigned long long)d), 31 + l};
}
__device__ __forceinline__ int ln_div(int x, LnDivU31 k) { return int(((unsigned long long)(unsigned)x * k.m) >> k.shift); }

// the cloud of a row: row / n0 for equal sizes, the search of the list otherwise (no division by n0 in that form)
__device__ __forceinline__ int ln_cloud_of_row(int row, LnDivU31 by_n0) { return ln_div(row, by_n0); }

template <bool WEIGHTED, class CLOUD_OF>  // CLOUD_OF: LnDivU31 (by n0) or LnCloudOfRowListed; the host picks
__global__ void __launch_bounds__(256)
    k_nll_clouds_backward(const long long* __restrict__ target, const float* __restrict__ grad_loss, const float* __restrict__ weight_sum,
                          int total, CLOUD_OF cloud_of, LnDivU31 by_C, int C, int B, long long ignore_index, const float* __restrict__ cw,
                          float* __restrict__ grad_lp) {
    const long long g64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g64 >= total) return;
    const int g = int(g64);  // n * C < 2^31
    const int i = ln_div(g, by_C), c = g - i * C;
    const long long t = target[i];
    const float d = float(B) * weight_sum[ln_cloud_of_row(i, cloud_of)];  // (read for every row, beside the label: not a second trip behind it)
    const float gl = -grad_loss[0];
    const long long tc = t < 0 ? 0 : (t >= C ? C - 1 : t);
    float v = 0.f;
    if (t != ignore_index && c == tc) v = WEIGHTED ? (gl * cw[tc]) / d : gl / d;
    grad_lp[g] = v;
}


// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
struct LnNllcLayout {
    long long n0, clouds;  // rows of a full cloud (<= max(n, 1)), clouds (>= 1)
    int grid_blocks;       // blocks of the longest cloud
    size_t bytes;
};
// total: any argument gives a layout (ln_cloud_split)
LnNllcLayout ln_nllc_layout(long long n, long long points_per_cloud) {
    LnNllcLayout L;
    const LnCloudSplit S = ln_cloud_split(n < (1ll << 31) ? n : 1ll << 31, points_per_cloud);  // (2^31 rows and more are refused: any size will do)
    L.n0 = S.n0;
    L.clouds = S.clouds;
    L.grid_blocks = ln_nllc_blocks(L.n0);
    // clouds of one block publish their sums themselves: no partials
    L.bytes = 256 + (L.grid_blocks > 1 ? ((size_t(L.clouds) * size_t(L.grid_blocks) * 2 * sizeof(float) + 255) & ~size_t(255)) : 0);
    return L;
}
// The layout of a listed batch: grids and the stride of a cloud's partials by the longest cloud.  Total: clouds is brought into
// [1, LN_NLLC_MAX_CLOUDS], longest into [0, n].
LnNllcLayout ln_nllc_layout_ranges(long long n, long long clouds, long long longest) {
    LnNllcLayout L;
    const long long N = n < 0 ? 0 : (n < (1ll << 31) ? n : 1ll << 31);
    L.n0 = longest < 0 ? 0 : (longest > N ? N : longest);
    L.clouds = clouds < 1 ? 1 : (clouds > LN_NLLC_MAX_CLOUDS ? LN_NLLC_MAX_CLOUDS : clouds);
    L.grid_blocks = ln_nllc_blocks(L.n0);
    L.bytes = 256 + (L.grid_blocks > 1 ? ((size_t(L.clouds) * size_t(L.grid_blocks) * 2 * sizeof(float) + 255) & ~size_t(255)) : 0);
    return L;
}
int ln_nllc_sizes(const char* who, long long n, long long points_per_cloud, int classes, LnNllcLayout& L) {
    LN_REQUIRE(n >= 0 && classes >= 1, LN_ERR_ARG, "%s: bad sizes (n >= 0, classes >= 1)", who);
    LN_REQUIRE(points_per_cloud >= 1, LN_ERR_ARG, "%s: bad sizes (points_per_cloud >= 1)", who);
    LN_REQUIRE(n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_UNSUPPORTED, "%s: n * classes must stay below 2^31", who);
    L = ln_nllc_layout(n, points_per_cloud);
    LN_REQUIRE(L.clouds <= LN_NLLC_MAX_CLOUDS, LN_ERR_UNSUPPORTED, "%s: %lld clouds, at most %d (the cloud is the y coordinate of the grid)",
               who, L.clouds, LN_NLLC_MAX_CLOUDS);
    return LN_OK;
}

int ln_nllc_sizes_ranges(const char* who, long long n, const int* point_starts, int clouds, long long longest, int classes, LnNllcLayout& L) {
    LN_REQUIRE(n >= 0 && classes >= 1, LN_ERR_ARG, "%s: bad sizes (n >= 0, classes >= 1)", who);
    LN_REQUIRE(n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_UNSUPPORTED, "%s: n * classes must stay below 2^31", who);
    LN_REQUIRE_CLOUD_LIST(who, n, point_starts, clouds, longest, LN_NLLC_MAX_CLOUDS, LN_ERR_UNSUPPORTED);
    L = ln_nllc_layout_ranges(n, clouds, longest);
    return LN_OK;
}

// what k_nll_clouds_wave takes of a cut: its clouds have at most 64 rows
int ln_nllc_wave_cut(long long n0) { return int(n0); }
LnCloudsListed ln_nllc_wave_cut(LnCloudsListed cut) { return cut; }

// Every forward entry point, its arguments checked.  loss == nullptr: the one-cloud entry, which takes no mean over the clouds (phase 2).
// cut: L.n0 (long long) for the equal-size entries, the list for the _ranges entries (L by ln_nllc_layout_ranges: L.n0 the longest cloud).
template <class CUT>
int ln_nllc_forward(const char* who, const float* log_probs, const long long* target, long long n, const LnNllcLayout& L, int classes,
                    long long ignore_index, const float* class_weight, float* partial, float* loss, float* per_cloud, float* weight_sum,
                    hipStream_t st, CUT cut) {
    using WAVE_CUT = decltype(ln_nllc_wave_cut(cut));
    const int B = int(L.clouds);
    const bool direct = L.grid_blocks == 1, mean = loss != nullptr;
    if (L.n0 <= LN_NLLC_WAVE_ROWS) {
        const dim3 grid(ln_div_up(B, LN_NLLC_THREADS / 64)), thr(LN_NLLC_THREADS);
        if (class_weight)
            LN_LAUNCH("k_nll_clouds_wave", (k_nll_clouds_wave<true, WAVE_CUT>), grid, thr, 0, st, log_probs, target, n, ln_nllc_wave_cut(cut), classes, B, ignore_index,
                      class_weight, per_cloud, weight_sum);
        else
            LN_LAUNCH("k_nll_clouds_wave", (k_nll_clouds_wave<false, WAVE_CUT>), grid, thr, 0, st, log_probs, target, n, ln_nllc_wave_cut(cut), classes, B, ignore_index,
                      class_weight, per_cloud, weight_sum);
    } else {
        const dim3 grid(L.grid_blocks, (unsigned)B), thr(LN_NLLC_THREADS);
#define LN_NLLC_PARTIALS(MODE)                                                                                                                 \
    LN_LAUNCH("k_nll_clouds_partials", (k_nll_clouds_partials<MODE, CUT>), grid, thr, 0, st, log_probs, target, n, cut, classes, ignore_index, \
              class_weight, partial, per_cloud, weight_sum)
        if (direct) {
            if (class_weight) LN_NLLC_PARTIALS(3);
            else LN_NLLC_PARTIALS(2);
        } else {
            if (class_weight) LN_NLLC_PARTIALS(1);
            else LN_NLLC_PARTIALS(0);
        }
#undef LN_NLLC_PARTIALS
    }
    const dim3 fthr(LN_NLLC_FINISH_THREADS);
#define LN_NLLC_FINISH(MODE, GRID) \
    LN_LAUNCH("k_nll_clouds_finish", (k_nll_clouds_finish<MODE, CUT>), dim3(GRID), fthr, 0, st, partial, n, cut, B, L.grid_blocks, per_cloud, weight_sum, loss)
    if (direct) {
        if (mean) LN_NLLC_FINISH(2, 1);
    } else if (B <= LN_NLLC_FUSED_CLOUDS) {
        if (mean) LN_NLLC_FINISH(3, 1);
        else LN_NLLC_FINISH(1, 1);
    } else {
        LN_NLLC_FINISH(1, ln_div_up(B, LN_NLLC_FINISH_WAVES));
        if (mean) LN_NLLC_FINISH(2, 1);
    }
#undef LN_NLLC_FINISH
    return ln_check_launch(who);
}

// Every backward entry point, its arguments checked and n > 0.  cloud_of: ln_div_u31(L.n0), or the list.
template <class CLOUD_OF>
int ln_nllc_backward(const char* who, const long long* target, const float* grad_loss, const float* weight_sum, long long n,
                     const LnNllcLayout& L, int classes, long long ignore_index, const float* class_weight, float* grad_log_probs,
                     hipStream_t st, CLOUD_OF cloud_of) {
    const dim3 grid(ln_div_up(n * classes, 256)), thr(256);
    const LnDivU31 by_C = ln_div_u31(classes);  // (1 <= classes <= n * classes < 2^31)
    if (class_weight)
        LN_LAUNCH("k_nll_clouds_backward", (k_nll_clouds_backward<true, CLOUD_OF>), grid, thr, 0, st, target, grad_loss, weight_sum, int(n * classes), cloud_of,
                  by_C, classes, int(L.clouds), ignore_index, class_weight, grad_log_probs);
    else
        LN_LAUNCH("k_nll_clouds_backward", (k_nll_clouds_backward<false, CLOUD_OF>), grid, thr, 0, st, target, grad_loss, weight_sum, int(n * classes), cloud_of,
                  by_C, classes, int(L.clouds), ignore_index, class_weight, grad_log_probs);
    return ln_check_launch(who);
}
}  // namespace

extern "C" size_t ln_nll_clouds_workspace_bytes(long long n, long long points_per_cloud) { return ln_nllc_layout(n, points_per_cloud).bytes; }

extern "C" int ln_nll_forward_clouds(const float* log_probs, const long long* target, long long n, long long points_per_cloud, int classes,
                                     long long ignore_index, const float* class_weight, void* workspace, size_t workspace_bytes, float* loss,
                                     float* per_cloud, float* weight_sum, void* stream) {
    LnNllcLayout L;
    const int rc = ln_nllc_sizes("ln_nll_forward_clouds", n, points_per_cloud, classes, L);
    if (rc != LN_OK) return rc;
    LN_REQUIRE(loss, LN_ERR_ARG, "ln_nll_forward_clouds: null buffer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return ln_zero_async(loss, sizeof(float), st);  // no cloud: the loss is 0; per_cloud and weight_sum have no element
    LN_REQUIRE(log_probs && target && per_cloud && weight_sum, LN_ERR_ARG, "ln_nll_forward_clouds: null buffer");
    LN_REQUIRE(workspace && workspace_bytes >= L.bytes, LN_ERR_ARG, "ln_nll_forward_clouds: null / small workspace (%zu bytes needed)", L.bytes);
    return ln_nllc_forward("ln_nll_forward_clouds", log_probs, target, n, L, classes, ignore_index, class_weight, static_cast<float*>(workspace),
                           loss, per_cloud, weight_sum, st, L.n0);
}

extern "C" int ln_nll_backward_clouds(const long long* target, const float* grad_loss, const float* weight_sum, long long n,
                                      long long points_per_cloud, int classes, long long ignore_index, const float* class_weight,
                                      float* grad_log_probs, void* stream) {
    LnNllcLayout L;
    const int rc = ln_nllc_sizes("ln_nll_backward_clouds", n, points_per_cloud, classes, L);
    if (rc != LN_OK) return rc;
    if (n == 0) return LN_OK;
    LN_REQUIRE(target && grad_loss && weight_sum && grad_log_probs, LN_ERR_ARG, "ln_nll_backward_clouds: null buffer");
    return ln_nllc_backward("ln_nll_backward_clouds", target, grad_loss, weight_sum, n, L, classes, ignore_index, class_weight, grad_log_probs,
                            (hipStream_t)stream, ln_div_u31(L.n0));  // (1 <= n0 <= n < 2^31)
}

// Clouds of unequal sizes: the rows of cloud b from point_starts (ln_loss_common.h, LnCloudsListed).
extern "C" size_t ln_nll_ranges_workspace_bytes(long long n, int clouds, long long longest) { return ln_nllc_layout_ranges(n, clouds, longest).bytes; }

extern "C" int ln_nll_forward_ranges(const float* log_probs, const long long* target, long long n, const int* point_starts, int clouds,
                                     long long longest, int classes, long long ignore_index, const float* class_weight, void* workspace,
                                     size_t workspace_bytes, float* loss, float* per_cloud, float* weight_sum, void* stream) {
    LnNllcLayout L;
    const int rc = ln_nllc_sizes_ranges("ln_nll_forward_ranges", n, point_starts, clouds, longest, classes, L);
    if (rc != LN_OK) return rc;
    LN_REQUIRE(loss && per_cloud && weight_sum, LN_ERR_ARG, "ln_nll_forward_ranges: null buffer");
    LN_REQUIRE(n == 0 || (log_probs && target), LN_ERR_ARG, "ln_nll_forward_ranges: null buffer");
    LN_REQUIRE(workspace && workspace_bytes >= L.bytes, LN_ERR_ARG, "ln_nll_forward_ranges: null / small workspace (%zu bytes needed)", L.bytes);
    // (n = 0: every cloud is empty; a wave over a cloud of no rows reads nothing and writes -0 and 1)
    const LnCloudsListed cut{point_starts, L.n0};
    return ln_nllc_forward("ln_nll_forward_ranges", log_probs, target, n, L, classes, ignore_index, class_weight, static_cast<float*>(workspace),
                           loss, per_cloud, weight_sum, (hipStream_t)stream, cut);
}

extern "C" int ln_nll_backward_ranges(const long long* target, const float* grad_loss, const float* weight_sum, long long n,
                                      const int* point_starts, int clouds, long long longest, int classes, long long ignore_index,
                                      const float* class_weight, float* grad_log_probs, void* stream) {
    LnNllcLayout L;
    const int rc = ln_nllc_sizes_ranges("ln_nll_backward_ranges", n, point_starts, clouds, longest, classes, L);
    if (rc != LN_OK) return rc;
    if (n == 0) return LN_OK;
    LN_REQUIRE(target && grad_loss && weight_sum && grad_log_probs, LN_ERR_ARG, "ln_nll_backward_ranges: null buffer");
    return ln_nllc_backward("ln_nll_backward_ranges", target, grad_loss, weight_sum, n, L, classes, ignore_index, class_weight, grad_log_probs,
                            (hipStream_t)stream, LnCloudOfRowListed{point_starts, clouds});
}

// The one-cloud, unweighted entry: points_per_cloud = n.  One size serves every n: the partials of one cloud.
extern "C" size_t ln_nll_workspace_bytes(void) { return (size_t)LN_NLLC_BLOCKS * 2 * sizeof(float); }

extern "C" int ln_nll_forward(const float* log_probs, const long long* target, long long n, int classes, long long ignore_index,
                              void* workspace, size_t workspace_bytes, float* loss_count, void* stream) {
    LnNllcLayout L;
    const int rc = ln_nllc_sizes("ln_nll_forward", n, n > 0 ? n : 1, classes, L);
    if (rc != LN_OK) return rc;
    LN_REQUIRE(loss_count && workspace && workspace_bytes >= ln_nll_workspace_bytes(), LN_ERR_ARG, "ln_nll_forward: null buffer / small workspace");
    LN_REQUIRE(n == 0 || (log_probs && target), LN_ERR_ARG, "ln_nll_forward: null buffer");
    // (n = 0: a wave over a cloud of no rows writes -0 and 1)
    return ln_nllc_forward("ln_nll_forward", log_probs, target, n, L, classes, ignore_index, nullptr, static_cast<float*>(workspace), nullptr,
                           loss_count, loss_count + 1, (hipStream_t)stream, L.n0);
}

extern "C" int ln_nll_backward(const long long* target, const float* grad_loss, const float* loss_count, long long n, int classes,
                               long long ignore_index, float* grad_log_probs, void* stream) {
    LnNllcLayout L;
    const int rc = ln_nllc_sizes("ln_nll_backward", n, n > 0 ? n : 1, classes, L);
    if (rc != LN_OK) return rc;
    if (n == 0) return LN_OK;
    LN_REQUIRE(target && grad_loss && loss_count && grad_log_probs, LN_ERR_ARG, "ln_nll_backward: null buffer");
    return ln_nllc_backward("ln_nll_backward", target, grad_loss, loss_count + 1, n, L, classes, ignore_index, nullptr, grad_log_probs,
                            (hipStream_t)stream, ln_div_u31(L.n0));  // (1 <= n0 <= n < 2^31)
}
