// Generalized soft Dice loss of the training loop (ln_train.py:127, diceloss.py:172-209) over log-probabilities [n, C] and labels [n],
// single and per cloud of a cloud-major batch, forward value and the gradient wrt the log-probabilities.
//
// Per cloud, with p = exp(lp), w_c = 0 for c == ignore_index, else 1:
//     I_c = sum_i p_ic [y_i = c],   S_c = sum_i p_ic,   G_c = #{i : y_i = c},   D_c = S_c + G_c + 1e-6
//     loss = sum_c w_c (1 - 2 I_c / D_c) / C
//     d loss / d lp[i, c] = -p_ic (a_c [y_i = c] - b_c),   a_c = 2 w_c / (C D_c),   b_c = 2 w_c I_c / (C D_c^2)
// A label outside [0, C) belongs to no class: the point counts in S only (what ln_nll_forward's "no class" means; the torch form
// faults on such a label).  Points labelled ignore_index count in S of every class; the division keeps all C classes; a class absent
// from the cloud contributes w_c / C.  A batch: cloud b owns rows [b n0, min((b + 1) n0, n)), the loss is the mean over the clouds of
// each cloud's own loss, and a, b carry the 1 / clouds.
//
// Clouds of unequal sizes (ln_dice_forward_ranges / ln_dice_backward_ranges): cloud b owns the rows point_starts[b] .. point_starts[b + 1] of
// a device list (LnCloudsListed, ln_loss_common.h); the same kernels instantiated on the list, the grid and the stride of a cloud's
// partials by the longest cloud.  A cloud of no rows has no tile: its I, S, G are 0 and its loss sum_c w_c / C.
//
// Arithmetic, pinned so that tests/dice_reference.py can count its roundings: p = expf(lp) (OCML, 1 ulp); every sum in a fixed order,
// no float atomics; G in 32-bit integers, converted once; IEEE division; no contraction (-ffp-contract=off).
//
//   k_dice_partials   grid (tiles, clouds): a workgroup takes a tile of rows of ONE cloud.  The tiling is a function of the cloud's own
//                     length (ln_dice_tiling: LN_DICE_STEPS steps of a workgroup per tile until the cloud has LN_DICE_MAX_TILES tiles,
//                     longer tiles from there on), so a cloud is cut, and summed, exactly as when it is handed over alone; workgroups
//                     behind a cloud's last tile leave.  C <= 256: a workgroup steps through the tile's elements R C at a time, R =
//                     256 / C whole rows — lane t keeps class t % C for its whole walk, loads are consecutive over the lanes; the R
//                     lanes of a class are added in LDS in row order.  C > 256: one row per step, lane t walks columns t, t + 256, ..
//                     One [3, C] partial per workgroup: I, S as float, G as uint32.
//   k_dice_finish     one workgroup.  Per (cloud, class): the cloud's partials in tile order, D, the class term, a, b (coef [B, 2, C]),
//                     stats [B, 3, C].  Per cloud: the class terms in class order, / C.  Then the clouds strided over the 256 threads in
//                     series and the workgroup's fixed tree, / B.
//   k_dice_backward   elementwise: grad[i, c] = -grad_loss p (y_i == c ? a - b : -b), every element written.
#include "ln_loss_common.h"

#define LN_DICE_THREADS 256
#define LN_DICE_WAVES (LN_DICE_THREADS / 64)
#define LN_DICE_STEPS 16        // steps of a workgroup through its tile ..
#define LN_DICE_MAX_TILES 512   // .. until a cloud has this many tiles: longer tiles from there on
#define LN_DICE_MAX_CLASSES 1024
#define LN_DICE_COLS (LN_DICE_MAX_CLASSES / LN_DICE_THREADS)  // columns of a lane, C > 256
#define LN_DICE_MAX_CLOUDS 65535  // grid y
#define LN_DICE_FINISH_LOADS 16   // partials a thread of k_dice_finish has in flight

// How a cloud of `len` rows is cut into tiles: rows per step of a workgroup, rows per tile, tiles.  (tests/dice_reference.py repeats it.)
struct LnDiceTiling {
    int step_rows;
    long long tile_rows;
    int tiles;
};
LN_HD LnDiceTiling ln_dice_tiling(long long len, int C) {
    LnDiceTiling t;
    t.step_rows = C <= LN_DICE_THREADS ? LN_DICE_THREADS / C : 1;
    long long steps = LN_DICE_STEPS;
    const long long cap = (long long)t.step_rows * LN_DICE_MAX_TILES;  // rows of one step of every tile
    if (len > cap * LN_DICE_STEPS) steps = (len + cap - 1) / cap;
    t.tile_rows = t.step_rows * steps;
    t.tiles = int((len + t.tile_rows - 1) / t.tile_rows);
    return t;
}
// tiles of the grid: at least the tiles of every cloud of at most n0 rows
static inline int ln_dice_grid_tiles(long long n0, int C) {
    const long long base = (long long)(C <= LN_DICE_THREADS ? LN_DICE_THREADS / C : 1) * LN_DICE_STEPS;
    const long long t = (n0 + base - 1) / base;
    return int(t < LN_DICE_MAX_TILES ? t : LN_DICE_MAX_TILES);
}

// CUT, in the kernels that walk a cloud: how the batch is cut (ln_loss_common.h) — the rows of a full cloud (long long: the instances of
// ln_dice_forward) or LnCloudsListed (ln_dice_forward_ranges).  The host picks the instance.
template <bool WIDE, class CUT>  // WIDE: C > 256
__global__ void __launch_bounds__(LN_DICE_THREADS)
    k_dice_partials(const float* __restrict__ lp, const long long* __restrict__ target, long long n, CUT cut, int C,
                    uint32_t* __restrict__ partial) {
    const LnCloudRange cloud = ln_cloud_range(n, cut, blockIdx.y);
    const long long first = cloud.first, len = cloud.len;
    const LnDiceTiling T = ln_dice_tiling(len, C);
    if ((int)blockIdx.x >= T.tiles) return;  // (the whole workgroup)
    const long long row0 = (long long)blockIdx.x * T.tile_rows;
    const long long row1 = row0 + T.tile_rows < len ? row0 + T.tile_rows : len;
    uint32_t* out = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 3 * C;
    if (!WIDE) {
        __shared__ float s_I[LN_DICE_THREADS], s_S[LN_DICE_THREADS];
        __shared__ uint32_t s_G[LN_DICE_THREADS];
        const int R = T.step_rows;
        const int r = threadIdx.x / C, c = threadIdx.x - r * C;
        float I = 0.f, S = 0.f;
        uint32_t G = 0u;
        if (r < R) {
#pragma unroll 4
            for (long long row = row0 + r; row < row1; row += R) {
                const long long t = target[first + row];
                const float p = expf(lp[(first + row) * C + c]);
                S += p;
                if (t == c) {
                    I += p;
                    ++G;
                }
            }
        }
        s_I[threadIdx.x] = I;
        s_S[threadIdx.x] = S;
        s_G[threadIdx.x] = G;
        __syncthreads();
        if (threadIdx.x < C) {
            I = s_I[threadIdx.x];
            S = s_S[threadIdx.x];
            G = s_G[threadIdx.x];
            for (int k = 1; k < R; ++k) {
                I += s_I[k * C + threadIdx.x];
                S += s_S[k * C + threadIdx.x];
                G += s_G[k * C + threadIdx.x];
            }
            out[threadIdx.x] = __float_as_uint(I);
            out[C + threadIdx.x] = __float_as_uint(S);
            out[2 * C + threadIdx.x] = G;
        }
    } else {
        float I[LN_DICE_COLS], S[LN_DICE_COLS];
        uint32_t G[LN_DICE_COLS];
#pragma unroll
        for (int j = 0; j < LN_DICE_COLS; ++j) {
            I[j] = S[j] = 0.f;
            G[j] = 0u;
        }
        for (long long row = row0; row < row1; ++row) {
            const long long t = target[first + row];
            const float* x = lp + (first + row) * C;
#pragma unroll
            for (int j = 0; j < LN_DICE_COLS; ++j) {
                const int c = threadIdx.x + j * LN_DICE_THREADS;
                if (c < C) {
                    const float p = expf(x[c]);
                    S[j] += p;
                    if (t == c) {
                        I[j] += p;
                        ++G[j];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < LN_DICE_COLS; ++j) {
            const int c = threadIdx.x + j * LN_DICE_THREADS;
            if (c < C) {
                out[c] = __float_as_uint(I[j]);
                out[C + c] = __float_as_uint(S[j]);
                out[2 * C + c] = G[j];
            }
        }
    }
}

// `terms` [B, C]: the class terms, written and read back by this workgroup alone (a barrier in between)
template <class CUT>
__global__ void __launch_bounds__(LN_DICE_THREADS)
    k_dice_finish(const uint32_t* __restrict__ partial, long long n, CUT cut, int C, int B, int grid_tiles, long long ignore_index,
                  float* __restrict__ terms, float* __restrict__ loss, float* __restrict__ per_cloud, float* __restrict__ stats,
                  float* __restrict__ coef) {
    __shared__ float s_w[LN_DICE_WAVES];
    const float Cf = float(C), Bf = float(B);
    for (long long item = threadIdx.x; item < (long long)B * C; item += LN_DICE_THREADS) {
        const int b = int(item / C), c = int(item - (long long)b * C);
        const int tiles = ln_dice_tiling(ln_cloud_range(n, cut, b).len, C).tiles;
        const uint32_t* p = partial + (long long)b * grid_tiles * 3 * C + c;
        float I = 0.f, S = 0.f;
        uint32_t G = 0u;
        // LN_DICE_FINISH_LOADS tiles' loads in flight, added in tile order (one at a time, the 500 tiles of one 120 000 x 20 cloud cost 0.08 ms)
        for (int k0 = 0; k0 < tiles; k0 += LN_DICE_FINISH_LOADS) {
            uint32_t vi[LN_DICE_FINISH_LOADS], vs[LN_DICE_FINISH_LOADS], vg[LN_DICE_FINISH_LOADS];
#pragma unroll
            for (int j = 0; j < LN_DICE_FINISH_LOADS; ++j) {
                const bool in = k0 + j < tiles;
                const uint32_t* q = p + (long long)(in ? k0 + j : k0) * 3 * C;
                vi[j] = in ? q[0] : 0u;
                vs[j] = in ? q[C] : 0u;
                vg[j] = in ? q[2 * C] : 0u;
            }
#pragma unroll
            for (int j = 0; j < LN_DICE_FINISH_LOADS; ++j)
                if (k0 + j < tiles) {
                    I += __uint_as_float(vi[j]);
                    S += __uint_as_float(vs[j]);
                    G += vg[j];
                }
        }
        const float Gf = float(G);
        const float D = (S + Gf) + 1e-6f;
        const float w = c == ignore_index ? 0.f : 1.f;
        terms[item] = w * (1.f - (2.f * I) / D);
        const float a = ((2.f * w) / (Cf * D)) / Bf;  // (the last division: no rounding when B is a power of two; x / 1 = x)
        coef[((long long)b * 2) * C + c] = a;
        coef[((long long)b * 2 + 1) * C + c] = (a * I) / D;
        if (stats) {
            stats[((long long)b * 3) * C + c] = I;
            stats[((long long)b * 3 + 1) * C + c] = S;
            stats[((long long)b * 3 + 2) * C + c] = Gf;
        }
    }
    __syncthreads();
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += LN_DICE_THREADS) {
        const float* t = terms + (long long)b * C;
        float sum = t[0];
        for (int c = 1; c < C; ++c) sum += t[c];
        const float v = sum / Cf;
        if (per_cloud) per_cloud[b] = v;
        acc += v;
    }
    const float total = ln_block_sum_256(acc, s_w);
    if (threadIdx.x == 0) loss[0] = total / Bf;
}

// the cloud of a row: row / n0 for equal sizes, the search of the list otherwise (no division by n0 in that form)
__device__ __forceinline__ int ln_cloud_of_row(int row, int n0) { return row / n0; }

template <class CLOUD_OF>  // CLOUD_OF: int (n0) or LnCloudOfRowListed; the host picks
__global__ void __launch_bounds__(256)
    k_dice_backward(const float* __restrict__ lp, const long long* __restrict__ target, const float* __restrict__ coef,
                    const float* __restrict__ grad_loss, int total, CLOUD_OF cloud_of, int C, float* __restrict__ grad_lp) {
    const long long g64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g64 >= total) return;
    const int g = int(g64);  // n * C < 2^31: 32-bit divisions
    const int i = g / C, c = g - i * C;
    const float* ab = coef + (long long)ln_cloud_of_row(i, cloud_of) * 2 * C;
    const float a = ab[c], b = ab[C + c];
    const float p = expf(lp[g]);
    const float t = target[i] == c ? a - b : -b;
    grad_lp[g] = -grad_loss[0] * (p * t);
}

// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
struct LnDiceLayout {
    long long n0, clouds;  // points of a full cloud (<= max(n, 1)), clouds (>= 1)
    int grid_tiles;
    size_t partial, terms, bytes;
};
// grid and workspace of a layout whose n0 and clouds are set: the grid by n0 (at least min_tiles), [clouds, grid_tiles, 3, C] partials,
// then [clouds, C] terms
LnDiceLayout ln_dice_layout_bytes(LnDiceLayout L, int classes, int min_tiles) {
    const size_t B = size_t(L.clouds);
    const int Cc = classes < 1 ? 1 : (classes > LN_DICE_MAX_CLASSES ? LN_DICE_MAX_CLASSES : classes);
    L.grid_tiles = ln_dice_grid_tiles(L.n0, Cc);
    if (L.grid_tiles < min_tiles) L.grid_tiles = min_tiles;
    L.partial = 0;
    L.terms = (B * size_t(L.grid_tiles) * 3 * size_t(Cc) * 4 + 255) & ~size_t(255);
    L.bytes = ((L.terms + B * size_t(Cc) * 4 + 255) & ~size_t(255)) + 256;
    return L;
}
// total: any argument gives a layout (ln_cloud_split)
LnDiceLayout ln_dice_layout(long long n, long long points_per_cloud, int classes) {
    LnDiceLayout L;
    const LnCloudSplit S = ln_cloud_split(n < (1ll << 31) ? n : 1ll << 31, points_per_cloud);  // (2^31 rows and more are refused: any size will do)
    L.n0 = S.n0;
    L.clouds = S.clouds;
    return ln_dice_layout_bytes(L, classes, 0);
}
// The layout of a listed batch (ln_loss_common.h, LnCloudsListed): the grid and the stride of a cloud's partials by the longest cloud, at
// least one tile (a batch of empty clouds still runs the finish).  Total: clouds is brought into [1, LN_DICE_MAX_CLOUDS], longest into [0, n].
LnDiceLayout ln_dice_layout_ranges(long long n, long long clouds, long long longest, int classes) {
    LnDiceLayout L;
    const long long N = n < 0 ? 0 : (n < (1ll << 31) ? n : 1ll << 31);
    L.n0 = longest < 0 ? 0 : (longest > N ? N : longest);
    L.clouds = clouds < 1 ? 1 : (clouds > LN_DICE_MAX_CLOUDS ? LN_DICE_MAX_CLOUDS : clouds);
    return ln_dice_layout_bytes(L, classes, 1);
}
int ln_dice_sizes_ranges(const char* who, long long n, const int* point_starts, int clouds, long long longest, int classes, LnDiceLayout& L) {
    LN_REQUIRE(n >= 0 && classes >= 1 && classes <= LN_DICE_MAX_CLASSES, LN_ERR_ARG, "%s: bad sizes (n >= 0, 1 <= classes <= %d)", who,
               LN_DICE_MAX_CLASSES);
    LN_REQUIRE(n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_ARG, "%s: n * classes must stay below 2^31", who);
    LN_REQUIRE_CLOUD_LIST(who, n, point_starts, clouds, longest, LN_DICE_MAX_CLOUDS, LN_ERR_ARG);
    L = ln_dice_layout_ranges(n, clouds, longest, classes);
    return LN_OK;
}
int ln_dice_sizes(const char* who, long long n, long long points_per_cloud, int classes, LnDiceLayout& L) {
    LN_REQUIRE(n >= 0 && classes >= 1 && classes <= LN_DICE_MAX_CLASSES, LN_ERR_ARG, "%s: bad sizes (n >= 0, 1 <= classes <= %d)", who,
               LN_DICE_MAX_CLASSES);
    LN_REQUIRE(points_per_cloud >= 1, LN_ERR_ARG, "%s: bad sizes (points_per_cloud >= 1)", who);
    LN_REQUIRE(n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_ARG, "%s: n * classes must stay below 2^31", who);
    L = ln_dice_layout(n, points_per_cloud, classes);
    LN_REQUIRE(L.clouds <= LN_DICE_MAX_CLOUDS, LN_ERR_ARG, "%s: %lld clouds, at most %d (the cloud is the y coordinate of the grid)", who,
               L.clouds, LN_DICE_MAX_CLOUDS);
    return LN_OK;
}
// The launch sequences, once for either cut (ln_loss_common.h): CUT = long long (n0) with CLOUD_OF = int (n0), or LnCloudsListed with
// LnCloudOfRowListed.
template <class CUT>
int ln_dice_forward_run(const char* who, const float* log_probs, const long long* target, long long n, CUT cut, const LnDiceLayout& L, int classes,
                        long long ignore_index, void* workspace, size_t workspace_bytes, float* loss, float* per_cloud, float* stats, float* coef,
                        hipStream_t st) {
    LN_REQUIRE(workspace && workspace_bytes >= L.bytes, LN_ERR_ARG, "%s: null / small workspace (%zu bytes needed)", who, L.bytes);
    char* ws = static_cast<char*>(workspace);
    uint32_t* partial = reinterpret_cast<uint32_t*>(ws + L.partial);
    float* terms = reinterpret_cast<float*>(ws + L.terms);
    const dim3 grid(L.grid_tiles, (unsigned)L.clouds), thr(LN_DICE_THREADS);
    if (classes <= LN_DICE_THREADS)
        LN_LAUNCH("k_dice_partials", (k_dice_partials<false, CUT>), grid, thr, 0, st, log_probs, target, n, cut, classes, partial);
    else
        LN_LAUNCH("k_dice_partials", (k_dice_partials<true, CUT>), grid, thr, 0, st, log_probs, target, n, cut, classes, partial);
    LN_LAUNCH("k_dice_finish", k_dice_finish<CUT>, dim3(1), thr, 0, st, partial, n, cut, classes, int(L.clouds), L.grid_tiles, ignore_index, terms, loss,
              per_cloud, stats, coef);
    return ln_check_launch(who);
}
template <class CLOUD_OF>
int ln_dice_backward_run(const char* who, const float* log_probs, const long long* target, const float* coef, const float* grad_loss, long long n,
                         CLOUD_OF cloud_of, int classes, float* grad_log_probs, void* stream) {
    if (n == 0) return LN_OK;
    LN_REQUIRE(log_probs && target && coef && grad_loss && grad_log_probs, LN_ERR_ARG, "%s: null buffer", who);
    LN_LAUNCH("k_dice_backward", k_dice_backward<CLOUD_OF>, dim3(ln_div_up(n * classes, 256)), dim3(256), 0, (hipStream_t)stream, log_probs, target, coef,
              grad_loss, int(n * classes), cloud_of, classes, grad_log_probs);
    return ln_check_launch(who);
}
}  // namespace

extern "C" size_t ln_dice_workspace_bytes(long long n, long long points_per_cloud, int classes) {
    return ln_dice_layout(n, points_per_cloud, classes).bytes;
}

extern "C" int ln_dice_forward(const float* log_probs, const long long* target, long long n, long long points_per_cloud, int classes,
                               long long ignore_index, void* workspace, size_t workspace_bytes, float* loss, float* per_cloud, float* stats,
                               float* coef, void* stream) {
    LnDiceLayout L;
    const int rc = ln_dice_sizes("ln_dice_forward", n, points_per_cloud, classes, L);
    if (rc != LN_OK) return rc;
    LN_REQUIRE(loss, LN_ERR_ARG, "ln_dice_forward: null buffer");
    if (n == 0) return ln_zero_async(loss, sizeof(float), (hipStream_t)stream);  // no cloud: the loss is 0; per_cloud, stats and coef have no element
    LN_REQUIRE(log_probs && target && coef, LN_ERR_ARG, "ln_dice_forward: null buffer");
    return ln_dice_forward_run("ln_dice_forward", log_probs, target, n, L.n0, L, classes, ignore_index, workspace, workspace_bytes, loss, per_cloud,
                               stats, coef, (hipStream_t)stream);
}

extern "C" int ln_dice_backward(const float* log_probs, const long long* target, const float* coef, const float* grad_loss, long long n,
                                long long points_per_cloud, int classes, float* grad_log_probs, void* stream) {
    LnDiceLayout L;
    const int rc = ln_dice_sizes("ln_dice_backward", n, points_per_cloud, classes, L);
    if (rc != LN_OK) return rc;
    return ln_dice_backward_run("ln_dice_backward", log_probs, target, coef, grad_loss, n, int(L.n0), classes, grad_log_probs, stream);
}

// Clouds of unequal sizes: the rows of cloud b from point_starts.
extern "C" size_t ln_dice_ranges_workspace_bytes(long long n, int clouds, long long longest, int classes) {
    return ln_dice_layout_ranges(n, clouds, longest, classes).bytes;
}

extern "C" int ln_dice_forward_ranges(const float* log_probs, const long long* target, long long n, const int* point_starts, int clouds,
                                      long long longest, int classes, long long ignore_index, void* workspace, size_t workspace_bytes,
                                      float* loss, float* per_cloud, float* stats, float* coef, void* stream) {
    LnDiceLayout L;
    const int rc = ln_dice_sizes_ranges("ln_dice_forward_ranges", n, point_starts, clouds, longest, classes, L);
    if (rc != LN_OK) return rc;
    LN_REQUIRE(loss && coef, LN_ERR_ARG, "ln_dice_forward_ranges: null buffer");
    LN_REQUIRE(n == 0 || (log_probs && target), LN_ERR_ARG, "ln_dice_forward_ranges: null buffer");
    return ln_dice_forward_run("ln_dice_forward_ranges", log_probs, target, n, LnCloudsListed{point_starts, L.n0}, L, classes, ignore_index, workspace,
                               workspace_bytes, loss, per_cloud, stats, coef, (hipStream_t)stream);
}

extern "C" int ln_dice_backward_ranges(const float* log_probs, const long long* target, const float* coef, const float* grad_loss, long long n,
                                       const int* point_starts, int clouds, long long longest, int classes, float* grad_log_probs,
                                       void* stream) {
    LnDiceLayout L;
    const int rc = ln_dice_sizes_ranges("ln_dice_backward_ranges", n, point_starts, clouds, longest, classes, L);
    if (rc != LN_OK) return rc;
    return ln_dice_backward_run("ln_dice_backward_ranges", log_probs, target, coef, grad_loss, n, LnCloudOfRowListed{point_starts, clouds}, classes,
                                grad_log_probs, stream);
}
