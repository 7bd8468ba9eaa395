// Lovasz-Softmax loss of the training loop (ln_train.py:156-158, lovasz_loss.py:17-57; Berman et al., CVPR 2018) over
// log-probabilities [n, C] and labels [n], all classes at once, forward value and the gradient wrt the log-probabilities.
//
// Per class c:  p_i = exp(lp[i, c]),  fg_i = [clamp(y_i, 0, C-1) == c],  e_i = |fg_i - p_i|;  the errors in DESCENDING order, equal
// errors by ASCENDING point index (a stable sort);  loss_c = sum_k e_(k) g_k  with g the discrete gradient of the Jaccard loss along
// that order.  With G = #fg, F_k / B_k = foreground / background elements among the first k+1, U = G + B_k, I = G - F_k:
//        g_k = 1 / U               (element k foreground)
//        g_k = I / (U (U - 1))     (element k background)
// — the closed form of J_k - J_{k-1}, J_k = 1 - I/U: no difference of two O(1) numbers that agree in all but their last digits.
// A class counts when G > 0 and c != ignore_index;  loss = sum over the counting classes (/ max(#counting, 1) for "mean").
//
// Arithmetic, pinned so that tests/lovasz_reference.py can count its roundings:
//   p = expf(lp), a result below the smallest normal float counts as 0 (whether expf returns subnormals is the math library's
//   business);  e = p for background and |expm1f(lp)| for foreground (1 - p cancels when the prediction is right: expm1f keeps e to
//   an ulp);  U (U - 1) in 64-bit integers, converted once;  IEEE division;  no contraction (-ffp-contract=off).
//
// Stages (every sum in a fixed order, no float atomics: loss and gradient are bitwise reproducible):
//   k_lovasz_keys      [n, C] -> class-major (key, payload): key = 0x7FFFFFFF - bits(e) (the bits of a non-negative float are monotone
//                      as an integer, so ascending keys = descending errors), payload = point | fg << 31
//   4 x { k_lovasz_hist, k_lovasz_scan, k_lovasz_scatter }   stable LSD radix sort of the C segments, 8 bits per pass; bit 31 of
//                      the key is 0, so four passes cover every non-negative float (also inf / NaN of wild inputs: no index
//                      depends on a value being in [0, 1]).  Points arrive in index order and every pass is stable: the tie rule.
//   k_lovasz_fg_count, k_lovasz_scan    foreground count of every tile of the sorted order, exclusive scan per class (its total: G)
//   k_lovasz_dot       F_k from the tile base + wave ballots, g_k, the tile's sum of e g, and the coefficient
//                      scale_c s g p scattered to dloss_dlogp[point, c]  (s = -1 foreground, +1 background)
//   k_lovasz_finish    tile sums -> per-class losses -> loss
//   k_lovasz_backward  grad_log_probs = grad_loss * dloss_dlogp
//
// Batch of clouds (ln_lovasz_forward_clouds): the same kernels over B x C segments.  The points are cloud-major, cloud b owns rows
// [b n0, min((b + 1) n0, n)): every cloud has n0 points, the last one len_B-1 <= n0.  The cloud is the z coordinate of every grid, the
// class its y coordinate, a tile of 2048 sorted positions its x coordinate — so a tile never spans two clouds, and the tiles behind a
// short last cloud find no item.  Segment (b, c) keeps its keys and payloads at  b n0 C + c len_b  (all clouds in front of b are
// full: the buffers stay n C words), its tile histograms, tile counts and tile sums at  (b C + c) * tiles(n0);  the payload is the
// point's index INSIDE its cloud.  The single-cloud call is the case n0 = n, B = 1 of the same launches.  k_lovasz_finish runs one
// workgroup per cloud; k_lovasz_cloud_mean adds the clouds' losses in a fixed order and divides by B.  The gradient coefficient is divided by B.
//
// Clouds of unequal sizes (ln_lovasz_forward_ranges): cloud b owns the rows point_starts[b] .. point_starts[b + 1] of a device list
// (LnCloudsListed, ln_loss_common.h).  The same kernels instantiated on the list: segment (b, c) at  starts[b] C + c len_b, tiles and
// strides by the longest cloud, the tiles behind a cloud's last one find no item; a cloud of no rows has G = 0 everywhere and loss 0.
#include "ln_loss_common.h"

#define LN_LV_THREADS 256
#define LN_LV_WAVES (LN_LV_THREADS / 64)
#define LN_LV_IPT 8                                  // items per thread
#define LN_LV_TILE (LN_LV_THREADS * LN_LV_IPT)       // items per workgroup: 2048
#define LN_LV_SCAN_THREADS 1024
#define LN_LV_PASSES 4
#define LN_LV_MAX_CLASSES 1024
#define LN_LV_MAX_CLOUDS 65535  // grid z
#define LN_LV_FG 0x80000000u

__device__ __forceinline__ float ln_lv_prob(float lp) {
    const float p = expf(lp);
    return p < 1.17549435e-38f ? 0.f : p;
}
__device__ __forceinline__ float ln_lv_error(float lp, bool fg) { return fg ? fabsf(expm1f(lp)) : ln_lv_prob(lp); }

// item `j` of this thread inside tile `b`: waves own contiguous runs of 64 * IPT items, a round of a wave is 64 consecutive items —
// position order = (wave, round, lane), loads and stores of a round are coalesced
__device__ __forceinline__ long long ln_lv_item(int b, int j) {
    return (long long)b * LN_LV_TILE + (threadIdx.x >> 6) * (64 * LN_LV_IPT) + j * 64 + (threadIdx.x & 63);
}

// Segment (cloud blockIdx.z, class blockIdx.y) of a launch: `first` = the cloud's first point row, `len` = its points (n0, less for the
// last cloud), `base` = the segment's first word in the key / payload buffers, `id` = cloud * C + class.
struct LnLvSegment {
    long long first, len, base, id;
};
// CUT, here and in the kernels that walk a segment: how the batch is cut (ln_loss_common.h) — the rows of a full cloud (long long: the
// instances of ln_lovasz_forward / ln_lovasz_forward_clouds) or LnCloudsListed (ln_lovasz_forward_ranges: `base` = starts[b] C + c len_b,
// the rows in front of cloud b times C, so the buffers stay n C words whatever the lengths are).  The host picks the instance.
template <class CUT>
__device__ __forceinline__ LnLvSegment ln_lv_segment(long long n, CUT cut, int C) {
    LnLvSegment s;
    const LnCloudRange cloud = ln_cloud_range(n, cut, blockIdx.z);
    s.first = cloud.first;
    s.len = cloud.len;
    s.base = s.first * C + (long long)blockIdx.y * s.len;
    s.id = (long long)blockIdx.z * C + blockIdx.y;
    return s;
}

template <class CUT>
__global__ void __launch_bounds__(LN_LV_THREADS)
    k_lovasz_keys(const float* __restrict__ lp, const long long* __restrict__ target, long long n, CUT cut, int C,
                  uint32_t* __restrict__ keys, uint32_t* __restrict__ pay) {
    const long long i = (long long)blockIdx.x * LN_LV_THREADS + threadIdx.x;  // inside the cloud
    const int c = blockIdx.y;
    const LnLvSegment s = ln_lv_segment(n, cut, C);
    if (i >= s.len) return;
    const long long t = target[s.first + i];
    const long long tc = t < 0 ? 0 : (t >= C ? C - 1 : t);
    const bool fg = tc == c;
    const float e = ln_lv_error(lp[(s.first + i) * C + c], fg);
    keys[s.base + i] = 0x7FFFFFFFu - (__float_as_uint(e) & 0x7FFFFFFFu);
    pay[s.base + i] = uint32_t(i) | (fg ? LN_LV_FG : 0u);
}

// digit histogram of every tile: hist[(segment * 256 + digit) * nblk + b]
template <class CUT>
__global__ void __launch_bounds__(LN_LV_THREADS)
    k_lovasz_hist(const uint32_t* __restrict__ keys, long long n, CUT cut, int C, int nblk, int shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[256];
    const int b = blockIdx.x;
    const LnLvSegment sg = ln_lv_segment(n, cut, C);
    const long long len = sg.len;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t* k = keys + sg.base;
#pragma unroll
    for (int j = 0; j < LN_LV_IPT; ++j) {
        const long long pos = ln_lv_item(b, j);
        if (pos < len) atomicAdd(&s_h[(k[pos] >> shift) & 255u], 1u);  // (integer: the order of the additions is immaterial)
    }
    __syncthreads();
    hist[(sg.id * 256 + threadIdx.x) * nblk + b] = s_h[threadIdx.x];
}

// exclusive scan in place of `len` ints per segment (one workgroup per segment, contiguous chunk per thread); totals[segment] = the sum.
// Grid (classes, clouds): with 1024 threads a one-dimensional grid of B C workgroups would pass the 2^32 work-items a launch may
// have in one dimension at B C = 2^22.
__global__ void __launch_bounds__(LN_LV_SCAN_THREADS)
    k_lovasz_scan(uint32_t* __restrict__ data, long long len, int* __restrict__ totals) {
    __shared__ int s_tmp[LN_LV_SCAN_THREADS / 64];
    const long long seg = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    uint32_t* d = data + seg * len;
    const long long chunk = (len + LN_LV_SCAN_THREADS - 1) / LN_LV_SCAN_THREADS;
    const long long lo = threadIdx.x * chunk;
    const long long hi = lo + chunk < len ? lo + chunk : len;
    int sum = 0;
    for (long long k = lo; k < hi; ++k) sum += int(d[k]);
    int total;
    int run = ln_block_excl_scan<LN_LV_SCAN_THREADS / 64>(sum, s_tmp, &total);
    for (long long k = lo; k < hi; ++k) {
        const int v = int(d[k]);
        d[k] = uint32_t(run);
        run += v;
    }
    if (totals && threadIdx.x == 0) totals[seg] = total;
}

// one stable pass: an item goes to  (items of smaller digits) + (items of its digit in earlier tiles)  [both: the scanned hist]
//                                 + (items of its digit earlier in this tile: earlier waves, earlier rounds, lower lanes)
template <class CUT>
__global__ void __launch_bounds__(LN_LV_THREADS)
    k_lovasz_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ pay_in, uint32_t* __restrict__ keys_out,
                     uint32_t* __restrict__ pay_out, const uint32_t* __restrict__ hist, long long n, CUT cut, int C, int nblk,
                     int shift) {
    __shared__ uint32_t s_cnt[LN_LV_WAVES][256];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LnLvSegment sg = ln_lv_segment(n, cut, C);
    const long long seg = sg.base, len = sg.len;
    uint32_t key[LN_LV_IPT], pl[LN_LV_IPT], rank[LN_LV_IPT];
#pragma unroll
    for (int j = 0; j < LN_LV_IPT; ++j) {
        const long long pos = ln_lv_item(b, j);
        key[j] = pos < len ? keys_in[seg + pos] : 0u;
        pl[j] = pos < len ? pay_in[seg + pos] : 0u;
    }
#pragma unroll
    for (int w = 0; w < LN_LV_WAVES; ++w) s_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < LN_LV_IPT; ++j) {
        const bool valid = ln_lv_item(b, j) < len;
        const uint32_t d = (key[j] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);  // lanes of this round that hold the same digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool mine = (d >> bit) & 1u;
            const unsigned long long m = __ballot(mine);
            peers &= mine ? m : ~m;
        }
        rank[j] = 0;
        if (valid) {
            const uint32_t prior = s_cnt[wave][d];  // items of this digit in the wave's earlier rounds
            rank[j] = prior + __popcll(peers & below);
            // every peer has read before the lowest one writes: the LDS serves one wave's accesses in program order
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if ((peers & below) == 0) s_cnt[wave][d] = prior + __popcll(peers);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {  // thread = digit: wave counts -> first destination of every wave's items of that digit
        uint32_t run = hist[(sg.id * 256 + threadIdx.x) * nblk + b];
#pragma unroll
        for (int w = 0; w < LN_LV_WAVES; ++w) {
            const uint32_t v = s_cnt[w][threadIdx.x];
            s_cnt[w][threadIdx.x] = run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LN_LV_IPT; ++j) {
        if (ln_lv_item(b, j) >= len) continue;
        const long long dst = (long long)s_cnt[wave][(key[j] >> shift) & 255u] + rank[j];
        if (dst < len) {  // (always, by construction)
            keys_out[seg + dst] = key[j];
            pay_out[seg + dst] = pl[j];
        }
    }
}

template <class CUT>
__global__ void __launch_bounds__(LN_LV_THREADS)
    k_lovasz_fg_count(const uint32_t* __restrict__ pay, long long n, CUT cut, int C, int nblk, uint32_t* __restrict__ fgcnt) {
    __shared__ int s_w[LN_LV_WAVES];
    const int b = blockIdx.x;
    const LnLvSegment sg = ln_lv_segment(n, cut, C);
    const long long len = sg.len;
    const uint32_t* p = pay + sg.base;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < LN_LV_IPT; ++j) {
        const long long pos = ln_lv_item(b, j);
        const bool fg = pos < len && (p[pos] & LN_LV_FG);
        cnt += __popcll(__ballot(fg));  // wave-uniform
    }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < LN_LV_WAVES; ++w) t += s_w[w];
        fgcnt[sg.id * nblk + b] = uint32_t(t);
    }
}

// number of classes that count (G > 0, not the ignore class), by every thread of the workgroup
__device__ __forceinline__ int ln_lv_counting(const int* __restrict__ G, int C, long long ignore_index, int* s_tmp) {
    int mine = 0;
    for (int k = threadIdx.x; k < C; k += LN_LV_THREADS) mine += (G[k] > 0 && k != ignore_index) ? 1 : 0;
    int total;
    (void)ln_block_excl_scan_256(mine, s_tmp, &total);
    return total;
}

template <class CUT>
__global__ void __launch_bounds__(LN_LV_THREADS)
    k_lovasz_dot(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pay, const uint32_t* __restrict__ fgbase,
                 const int* __restrict__ Gall, const float* __restrict__ lp, long long n, CUT cut, int C, int nblk,
                 long long ignore_index, int reduction, float clouds, float* __restrict__ partial, float* __restrict__ dl) {
    __shared__ int s_tmp[8];
    __shared__ int s_fg[LN_LV_WAVES];
    __shared__ float s_w[LN_LV_WAVES];
    const int b = blockIdx.x, c = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LnLvSegment sg = ln_lv_segment(n, cut, C);
    const long long seg = sg.base, len = sg.len;
    const int* G = Gall + (long long)blockIdx.z * C;  // of this cloud's classes
    const int counting = ln_lv_counting(G, C, ignore_index, s_tmp);
    const int Gc = G[c];
    const bool counts = Gc > 0 && c != ignore_index;
    const float scale = reduction == 0 ? 1.f / float(counting < 1 ? 1 : counting) : 1.f;
    uint32_t key[LN_LV_IPT], pl[LN_LV_IPT];
    unsigned long long fgmask[LN_LV_IPT];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < LN_LV_IPT; ++j) {
        const long long pos = ln_lv_item(b, j);
        key[j] = pos < len ? keys[seg + pos] : 0u;
        pl[j] = pos < len ? pay[seg + pos] : 0u;
        fgmask[j] = __ballot((pl[j] & LN_LV_FG) != 0);
        mine += __popcll(fgmask[j]);
    }
    if (lane == 0) s_fg[wave] = mine;
    __syncthreads();
    long long F = fgbase[sg.id * nblk + b];  // foreground elements in front of this wave's first item
#pragma unroll
    for (int w = 0; w < LN_LV_WAVES; ++w)
        if (w < wave) F += s_fg[w];
    const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < LN_LV_IPT; ++j) {
        const long long pos = ln_lv_item(b, j);
        const long long Fk = F + __popcll(fgmask[j] & upto);  // inclusive
        F += __popcll(fgmask[j]);
        if (pos >= len) continue;
        const bool fg = (pl[j] & LN_LV_FG) != 0;
        const long long i = pl[j] & ~LN_LV_FG;
        if (i >= len) continue;  // (never: the payload is a point index inside the cloud)
        const long long at = (sg.first + i) * C + c;
        float coef = 0.f;
        if (counts) {
            const long long U = Gc + (pos + 1 - Fk), I = Gc - Fk;
            const float g = fg ? 1.f / float(U) : float(I) / float((unsigned long long)(U * (U - 1)));
            const float e = __uint_as_float(0x7FFFFFFFu - key[j]);
            acc += e * g;
            coef = (((fg ? -g : g) * ln_lv_prob(lp[at])) * scale) / clouds;  // one rounding (none when `clouds` is a power of two; x / 1 = x)
        }
        dl[at] = coef;
    }
    const float t = ln_block_sum_256(acc, s_w);
    if (threadIdx.x == 0) partial[sg.id * nblk + b] = t;
}

// one workgroup per cloud: loss[cloud], per_class[cloud, :]
__global__ void __launch_bounds__(LN_LV_THREADS)
    k_lovasz_finish(const float* __restrict__ partial_all, const int* __restrict__ Gall, int nblk, int C, long long ignore_index,
                    int reduction, float* __restrict__ loss, float* __restrict__ per_class_all) {
    __shared__ float s_w[LN_LV_WAVES];
    const float* partial = partial_all + (long long)blockIdx.x * C * nblk;
    const int* G = Gall + (long long)blockIdx.x * C;
    float* per_class = per_class_all ? per_class_all + (long long)blockIdx.x * C : nullptr;
    float total = 0.f;
    int counting = 0;
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        for (int k = threadIdx.x; k < nblk; k += LN_LV_THREADS) acc += partial[(long long)c * nblk + k];
        const float pc = ln_block_sum_256(acc, s_w);
        if (threadIdx.x == 0) {
            const bool counts = G[c] > 0 && c != ignore_index;
            if (counts) {
                total += pc;
                ++counting;
            }
            if (per_class) per_class[c] = counts ? pc : 0.f;
        }
    }
    if (threadIdx.x == 0) loss[blockIdx.x] = reduction == 0 ? total / float(counting < 1 ? 1 : counting) : total;
}

// loss[0] = (cloud[0] + .. + cloud[B - 1]) / B: the clouds strided over the 256 threads in series, then the workgroup's fixed tree
__global__ void __launch_bounds__(LN_LV_THREADS)
    k_lovasz_cloud_mean(const float* __restrict__ cloud, long long B, float* __restrict__ loss, float* __restrict__ per_cloud) {
    __shared__ float s_w[LN_LV_WAVES];
    float acc = 0.f;
    for (long long k = threadIdx.x; k < B; k += LN_LV_THREADS) {
        const float v = cloud[k];
        acc += v;
        if (per_cloud) per_cloud[k] = v;
    }
    const float t = ln_block_sum_256(acc, s_w);
    if (threadIdx.x == 0) loss[0] = t / float(B);
}

__global__ void __launch_bounds__(256)
    k_lovasz_backward(const float* __restrict__ dl, const float* __restrict__ grad_loss, long long total, float* __restrict__ out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g < total) out[g] = grad_loss[0] * dl[g];
}

// ---------------------------------------------------------------------------------------------------------------------------------
namespace {
struct LnLovaszLayout {
    long long n0, clouds;  // points of a full cloud (<= n), clouds (>= 1)
    int nblk;              // tiles of a full cloud
    size_t keys[2], pay[2], hist, fgcnt, G, partial, cloud, bytes;
};
size_t ln_lv_align(size_t x) { return (x + 255) & ~size_t(255); }
// N rows in B clouds of at most P rows (nblk tiles each) at C classes
LnLovaszLayout ln_lv_layout_of(size_t N, size_t P, size_t B, int nblk, size_t C, bool per_cloud) {
    LnLovaszLayout L;
    const size_t S = C * B;  // segments
    L.n0 = (long long)P;
    L.clouds = (long long)B;
    L.nblk = nblk;
    size_t at = 0;
    for (int k = 0; k < 2; ++k) {
        L.keys[k] = at;
        at = ln_lv_align(at + C * N * 4);
        L.pay[k] = at;
        at = ln_lv_align(at + C * N * 4);
    }
    L.hist = at;
    at = ln_lv_align(at + S * 256 * size_t(L.nblk) * 4);
    L.fgcnt = at;
    at = ln_lv_align(at + S * size_t(L.nblk) * 4);
    L.G = at;
    at = ln_lv_align(at + S * 4);
    L.partial = at;
    at = ln_lv_align(at + S * size_t(L.nblk) * 4);
    L.cloud = at;
    if (per_cloud) at = ln_lv_align(at + B * 4);
    L.bytes = at + 256;
    return L;
}
// total: any argument gives a layout (ln_cloud_split)
LnLovaszLayout ln_lv_layout(long long n, long long points_per_cloud, int classes, bool per_cloud) {
    const LnCloudSplit split = ln_cloud_split(n, points_per_cloud);
    const size_t N = n > 0 ? size_t(n) : 0, P = size_t(split.n0);
    return ln_lv_layout_of(N, P, size_t(split.clouds), int(((N < P ? N : P) + LN_LV_TILE - 1) / LN_LV_TILE), classes > 0 ? size_t(classes) : 0,
                           per_cloud);
}
// Listed clouds (ln_loss_common.h, LnCloudsListed): tiles and strides by the longest cloud, at least one tile.  Total: n is brought into
// [0, 2^31], clouds into [1, LN_LV_MAX_CLOUDS], longest into [0, n].
LnLovaszLayout ln_lv_layout_ranges(long long n, long long clouds, long long longest, int classes) {
    const long long N = n < 0 ? 0 : (n < (1ll << 31) ? n : 1ll << 31);
    const long long P = longest < 0 ? 0 : (longest > N ? N : longest);
    const long long B = clouds < 1 ? 1 : (clouds > LN_LV_MAX_CLOUDS ? LN_LV_MAX_CLOUDS : clouds);
    const long long nblk = (P + LN_LV_TILE - 1) / LN_LV_TILE;
    return ln_lv_layout_of(size_t(N), size_t(P), size_t(B), int(nblk < 1 ? 1 : nblk), classes > 0 ? size_t(classes) : 0, true);
}

// The launches of every entry point, its arguments checked and n > 0.  cut: L.n0 (long long), or the list.  mean_form: the per-cloud entries (k_lovasz_finish writes the clouds'
// losses into the workspace and k_lovasz_cloud_mean the loss; the one-cloud entry lets k_lovasz_finish write the loss itself).
template <class CUT>
int ln_lv_launches(const char* who, bool mean_form, CUT cut, const LnLovaszLayout& L, const float* log_probs, const long long* target,
                   long long n, int classes, long long ignore_index, int reduction, void* workspace, float* loss, float* per_cloud,
                   float* per_class, float* dloss_dlogp, hipStream_t st) {
    const int B = int(L.clouds);
    char* ws = static_cast<char*>(workspace);
    uint32_t* keys[2] = {reinterpret_cast<uint32_t*>(ws + L.keys[0]), reinterpret_cast<uint32_t*>(ws + L.keys[1])};
    uint32_t* pay[2] = {reinterpret_cast<uint32_t*>(ws + L.pay[0]), reinterpret_cast<uint32_t*>(ws + L.pay[1])};
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + L.hist);
    uint32_t* fgcnt = reinterpret_cast<uint32_t*>(ws + L.fgcnt);
    int* G = reinterpret_cast<int*>(ws + L.G);
    float* partial = reinterpret_cast<float*>(ws + L.partial);
    float* cloud = reinterpret_cast<float*>(ws + L.cloud);
    const dim3 tiles(L.nblk, classes, B), segments(classes, B), thr(LN_LV_THREADS);
    const int key_blocks = ln_div_up(L.n0, LN_LV_THREADS);
    LN_LAUNCH("k_lovasz_keys", k_lovasz_keys<CUT>, dim3(key_blocks < 1 ? 1 : key_blocks, classes, B), thr, 0, st, log_probs, target, n, cut, classes,
              keys[0], pay[0]);
    for (int pass = 0; pass < LN_LV_PASSES; ++pass) {
        const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
        LN_LAUNCH("k_lovasz_hist", k_lovasz_hist<CUT>, tiles, thr, 0, st, keys[in], n, cut, classes, L.nblk, shift, hist);
        LN_LAUNCH("k_lovasz_scan", k_lovasz_scan, segments, dim3(LN_LV_SCAN_THREADS), 0, st, hist, 256ll * L.nblk, (int*)nullptr);
        LN_LAUNCH("k_lovasz_scatter", k_lovasz_scatter<CUT>, tiles, thr, 0, st, keys[in], pay[in], keys[out], pay[out], hist, n, cut, classes, L.nblk, shift);
    }
    static_assert(LN_LV_PASSES % 2 == 0, "the sorted order ends in buffer 0");
    LN_LAUNCH("k_lovasz_fg_count", k_lovasz_fg_count<CUT>, tiles, thr, 0, st, pay[0], n, cut, classes, L.nblk, fgcnt);
    LN_LAUNCH("k_lovasz_scan", k_lovasz_scan, segments, dim3(LN_LV_SCAN_THREADS), 0, st, fgcnt, (long long)L.nblk, G);
    LN_LAUNCH("k_lovasz_dot", k_lovasz_dot<CUT>, tiles, thr, 0, st, keys[0], pay[0], fgcnt, G, log_probs, n, cut, classes, L.nblk, ignore_index, reduction,
              float(B), partial, dloss_dlogp);
    LN_LAUNCH("k_lovasz_finish", k_lovasz_finish, dim3(B), thr, 0, st, partial, G, L.nblk, classes, ignore_index, reduction,
              mean_form ? cloud : loss, per_class);
    if (mean_form) LN_LAUNCH("k_lovasz_cloud_mean", k_lovasz_cloud_mean, dim3(1), thr, 0, st, cloud, (long long)B, loss, per_cloud);
    return ln_check_launch(who);
}

// Both equal-size entry points: `who` names the caller in messages; per_cloud_form: ln_lovasz_forward_clouds (the other passes
// points_per_cloud = n, one cloud).
int ln_lv_forward(const char* who, bool per_cloud_form, const float* log_probs, const long long* target, long long n,
                  long long points_per_cloud, int classes, long long ignore_index, int reduction, void* workspace, size_t workspace_bytes,
                  float* loss, float* per_cloud, float* per_class, float* dloss_dlogp, hipStream_t st) {
    LN_REQUIRE(n >= 0 && classes >= 1 && classes <= LN_LV_MAX_CLASSES, LN_ERR_ARG, "%s: bad sizes (n >= 0, 1 <= classes <= %d)", who,
               LN_LV_MAX_CLASSES);
    LN_REQUIRE(points_per_cloud >= 1 || !per_cloud_form, LN_ERR_ARG, "%s: bad sizes (points_per_cloud >= 1)", who);
    LN_REQUIRE(n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_ARG, "%s: n * classes must stay below 2^31", who);
    LN_REQUIRE(reduction == 0 || reduction == 1, LN_ERR_ARG, "%s: reduction is 0 (mean) or 1 (sum)", who);
    LN_REQUIRE(loss, LN_ERR_ARG, "%s: null buffer", who);
    const LnLovaszLayout L = ln_lv_layout(n, points_per_cloud, classes, per_cloud_form);
    LN_REQUIRE(L.clouds <= LN_LV_MAX_CLOUDS, LN_ERR_ARG, "%s: %lld clouds, at most %d (the cloud is the z coordinate of the grids)", who,
               L.clouds, LN_LV_MAX_CLOUDS);
    if (n == 0) {  // no class is present: the loss is 0 (and there is no cloud: per_cloud and the per-cloud per_class have no element)
        int rc = ln_zero_async(loss, sizeof(float), st);
        if (rc == LN_OK && per_class && !per_cloud_form) rc = ln_zero_async(per_class, size_t(classes) * sizeof(float), st);
        return rc;
    }
    LN_REQUIRE(log_probs && target && dloss_dlogp, LN_ERR_ARG, "%s: null buffer", who);
    LN_REQUIRE(workspace && workspace_bytes >= L.bytes, LN_ERR_ARG, "%s: null / small workspace (%zu bytes needed)", who, L.bytes);
    return ln_lv_launches(who, per_cloud_form, L.n0, L, log_probs, target, n, classes, ignore_index, reduction, workspace, loss,
                          per_cloud, per_class, dloss_dlogp, st);
}
}  // namespace

extern "C" size_t ln_lovasz_workspace_bytes(long long n, int classes) { return ln_lv_layout(n, n, classes, false).bytes; }
extern "C" size_t ln_lovasz_clouds_workspace_bytes(long long n, long long points_per_cloud, int classes) {
    return ln_lv_layout(n, points_per_cloud, classes, true).bytes;
}

extern "C" int ln_lovasz_forward(const float* log_probs, const long long* target, long long n, int classes, long long ignore_index,
                                 int reduction, void* workspace, size_t workspace_bytes, float* loss, float* per_class,
                                 float* dloss_dlogp, void* stream) {
    return ln_lv_forward("ln_lovasz_forward", false, log_probs, target, n, n, classes, ignore_index, reduction, workspace, workspace_bytes,
                         loss, nullptr, per_class, dloss_dlogp, (hipStream_t)stream);
}

extern "C" int ln_lovasz_forward_clouds(const float* log_probs, const long long* target, long long n, long long points_per_cloud,
                                        int classes, long long ignore_index, int reduction, void* workspace, size_t workspace_bytes,
                                        float* loss, float* per_cloud, float* per_class, float* dloss_dlogp, void* stream) {
    return ln_lv_forward("ln_lovasz_forward_clouds", true, log_probs, target, n, points_per_cloud, classes, ignore_index, reduction, workspace,
                         workspace_bytes, loss, per_cloud, per_class, dloss_dlogp, (hipStream_t)stream);
}

extern "C" int ln_lovasz_backward(const float* dloss_dlogp, const float* grad_loss, long long n, int classes, float* grad_log_probs,
                                  void* stream) {
    LN_REQUIRE(n >= 0 && classes >= 1 && classes <= LN_LV_MAX_CLASSES && n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_ARG,
               "ln_lovasz_backward: bad sizes");
    if (n == 0) return LN_OK;
    LN_REQUIRE(dloss_dlogp && grad_loss && grad_log_probs, LN_ERR_ARG, "ln_lovasz_backward: null buffer");
    LN_LAUNCH("k_lovasz_backward", k_lovasz_backward, dim3(ln_div_up(n * classes, 256)), dim3(256), 0, (hipStream_t)stream, dloss_dlogp, grad_loss,
              n * classes, grad_log_probs);
    return ln_check_launch("ln_lovasz_backward");
}

// Clouds of unequal sizes: the rows of cloud b from point_starts.  ln_lovasz_backward is the backward.
extern "C" size_t ln_lovasz_ranges_workspace_bytes(long long n, int clouds, long long longest, int classes) {
    return ln_lv_layout_ranges(n, clouds, longest, classes).bytes;
}

extern "C" int ln_lovasz_forward_ranges(const float* log_probs, const long long* target, long long n, const int* point_starts, int clouds,
                                        long long longest, int classes, long long ignore_index, int reduction, void* workspace,
                                        size_t workspace_bytes, float* loss, float* per_cloud, float* per_class, float* dloss_dlogp,
                                        void* stream) {
    const char* who = "ln_lovasz_forward_ranges";
    hipStream_t st = (hipStream_t)stream;
    LN_REQUIRE(n >= 0 && classes >= 1 && classes <= LN_LV_MAX_CLASSES, LN_ERR_ARG, "%s: bad sizes (n >= 0, 1 <= classes <= %d)", who,
               LN_LV_MAX_CLASSES);
    LN_REQUIRE(n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_ARG, "%s: n * classes must stay below 2^31", who);
    LN_REQUIRE_CLOUD_LIST(who, n, point_starts, clouds, longest, LN_LV_MAX_CLOUDS, LN_ERR_ARG);
    LN_REQUIRE(reduction == 0 || reduction == 1, LN_ERR_ARG, "%s: reduction is 0 (mean) or 1 (sum)", who);
    LN_REQUIRE(loss, LN_ERR_ARG, "%s: null buffer", who);
    if (n == 0) {  // every cloud is empty: each loss is 0, and so are their mean and every per-class row
        int rc = ln_zero_async(loss, sizeof(float), st);
        if (rc == LN_OK && per_cloud) rc = ln_zero_async(per_cloud, size_t(clouds) * sizeof(float), st);
        if (rc == LN_OK && per_class) rc = ln_zero_async(per_class, size_t(clouds) * size_t(classes) * sizeof(float), st);
        return rc;
    }
    const LnLovaszLayout L = ln_lv_layout_ranges(n, clouds, longest, classes);
    LN_REQUIRE(log_probs && target && dloss_dlogp, LN_ERR_ARG, "%s: null buffer", who);
    LN_REQUIRE(workspace && workspace_bytes >= L.bytes, LN_ERR_ARG, "%s: null / small workspace (%zu bytes needed)", who, L.bytes);
    return ln_lv_launches(who, true, LnCloudsListed{point_starts, L.n0}, L, log_probs, target, n, classes, ignore_index, reduction,
                          workspace, loss, per_cloud, per_class, dloss_dlogp, st);
}
