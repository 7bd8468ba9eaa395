// Intersection / union counts of the validation metric (callbacks/scores.py) for a batch of clouds: scores [n, C] float, labels [n]
// int64, cloud-major with n0 points per cloud (the last cloud may be shorter).  Per cloud b and class c:
//     pred_i = the LOWEST class index among the maxima of row i (torch.argmax's documented rule)
//     hit    = #{pred = label = c}  (the unclamped label: a label outside [0, C) never hits)
//     n_gt   = #{clamp(label, 0, C - 1) = c},   n_pred = #{pred = c},   in_gt = n_gt > 0 and c != unlabeled_index
//     intersection[c] += hit in_gt,   union[c] += (n_gt + n_pred - hit) in_gt        summed over the clouds
// — Scores.accumulate_scores called once per cloud.  Everything is integer: exact whatever the order of the additions.
//   k_iou_counts_clouds   grid (tiles of 256 rows of a cloud, cloud): a workgroup never spans two clouds.  One thread per row up to 64
//                         classes, one wave per row above (a thread walking a 4 KB row alone leaves every load of the wave in a
//                         line of its own).  Three LDS histograms per workgroup, their non-zero bins added to counts[cloud][3][C]
//                         in the workspace with integer atomics.
//   k_iou_finish_clouds   one thread per class walks the clouds and adds onto the two int64 accumulators (one writer per class).
// Rows that hold a NaN are not held to torch's rule (torch.argmax returns the NaN's index; here a NaN never wins a comparison).
#include "ln_loss_common.h"

#define LN_IOU_THREADS 256
#define LN_IOU_ROWS 256  // rows of a workgroup
#define LN_IOU_MAX_CLASSES 1024
#define LN_IOU_MAX_CLOUDS 65535      // grid y
#define LN_IOU_THREAD_ROW_CLASSES 64  // up to here one thread per row

// (integer additions into LDS: their order is immaterial)
__device__ __forceinline__ void ln_iou_tally(uint32_t* s_hit, uint32_t* s_gt, uint32_t* s_pred, int C, int pred, long long t) {
    const long long tc = t < 0 ? 0 : (t >= C ? C - 1 : t);
    atomicAdd(&s_pred[pred], 1u);
    atomicAdd(&s_gt[int(tc)], 1u);
    if (t == pred) atomicAdd(&s_hit[pred], 1u);
}

template <bool WAVE_ROW>
__global__ void __launch_bounds__(LN_IOU_THREADS)
    k_iou_counts_clouds(const float* __restrict__ scores, const long long* __restrict__ target, long long n, long long n0, int C,
                        uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_hit[LN_IOU_MAX_CLASSES], s_gt[LN_IOU_MAX_CLASSES], s_pred[LN_IOU_MAX_CLASSES];
    const LnCloudRange cloud = ln_cloud_range(n, n0, blockIdx.y);
    const long long first = cloud.first, len = cloud.len;
    for (int k = threadIdx.x; k < C; k += LN_IOU_THREADS) s_hit[k] = s_gt[k] = s_pred[k] = 0u;
    __syncthreads();
    if (!WAVE_ROW) {
        const long long i = (long long)blockIdx.x * LN_IOU_ROWS + threadIdx.x;
        if (i < len) {
            const float* row = scores + (first + i) * C;
            float best = row[0];
            int pred = 0;
            for (int k = 1; k < C; ++k) {
                const float v = row[k];
                if (v > best) {  // (strictly: the lowest index of equal maxima stays)
                    best = v;
                    pred = k;
                }
            }
            ln_iou_tally(s_hit, s_gt, s_pred, C, pred, target[first + i]);
        }
    } else {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int r = 0; r < 64; ++r) {
            const long long i = (long long)blockIdx.x * LN_IOU_ROWS + wave * 64 + r;  // wave-uniform
            if (i >= len) break;
            const float* row = scores + (first + i) * C;
            float best = row[lane];  // C > 64: every lane owns a class
            int pred = lane;
            for (int k = lane + 64; k < C; k += 64) {
                const float v = row[k];
                if (v > best) {
                    best = v;
                    pred = k;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const float ov = __shfl_down(best, off, 64);
                const int op = __shfl_down(pred, off, 64);
                if (ov > best || (ov == best && op < pred)) {
                    best = ov;
                    pred = op;
                }
            }
            if (lane == 0) ln_iou_tally(s_hit, s_gt, s_pred, C, pred, target[first + i]);
        }
    }
    __syncthreads();
    uint32_t* out = counts + (long long)blockIdx.y * 3 * C;
    for (int k = threadIdx.x; k < C; k += LN_IOU_THREADS) {
        if (s_hit[k]) atomicAdd(&out[k], s_hit[k]);
        if (s_gt[k]) atomicAdd(&out[C + k], s_gt[k]);
        if (s_pred[k]) atomicAdd(&out[2 * C + k], s_pred[k]);
    }
}

__global__ void __launch_bounds__(LN_IOU_THREADS)
    k_iou_finish_clouds(const uint32_t* __restrict__ counts, int clouds, int C, long long unlabeled_index, long long* __restrict__ intersection,
                        long long* __restrict__ union_) {
    const int c = blockIdx.x * LN_IOU_THREADS + threadIdx.x;
    if (c >= C) return;
    long long I = 0, U = 0;
    for (int b = 0; b < clouds; ++b) {
        const uint32_t* p = counts + (long long)b * 3 * C;
        const long long hit = p[c], gt = p[C + c], pred = p[2 * C + c];
        if (gt > 0 && c != unlabeled_index) {
            I += hit;
            U += gt + pred - hit;
        }
    }
    intersection[c] += I;
    union_[c] += U;
}

namespace {
// total: any argument gives a size (ln_cloud_split); no rows, no cloud
size_t ln_iou_clouds(long long n, long long points_per_cloud) { return n > 0 ? size_t(ln_cloud_split(n, points_per_cloud).clouds) : 0; }
size_t ln_iou_counts_bytes(long long n, long long points_per_cloud, int classes) {
    return ln_iou_clouds(n, points_per_cloud) * 3 * (classes > 0 ? size_t(classes) : 0) * sizeof(uint32_t);
}
}  // namespace

extern "C" size_t ln_iou_counts_clouds_workspace_bytes(long long n, long long points_per_cloud, int classes) {
    return ((ln_iou_counts_bytes(n, points_per_cloud, classes) + 255) & ~size_t(255)) + 256;
}

extern "C" int ln_iou_counts_clouds(const float* scores, const long long* target, long long n, long long points_per_cloud, int classes,
                                    long long unlabeled_index, void* workspace, size_t workspace_bytes, long long* intersection,
                                    long long* union_, void* stream) {
    LN_REQUIRE(n >= 0 && points_per_cloud >= 1 && classes >= 1 && classes <= LN_IOU_MAX_CLASSES, LN_ERR_ARG,
               "ln_iou_counts_clouds: bad sizes (n >= 0, points_per_cloud >= 1, 1 <= classes <= %d)", LN_IOU_MAX_CLASSES);
    LN_REQUIRE(n < (1ll << 31) && n * classes < (1ll << 31), LN_ERR_ARG, "ln_iou_counts_clouds: n * classes must stay below 2^31");
    const long long n0 = ln_cloud_split(n, points_per_cloud).n0;
    const size_t clouds = ln_iou_clouds(n, n0);
    LN_REQUIRE(clouds <= LN_IOU_MAX_CLOUDS, LN_ERR_ARG, "ln_iou_counts_clouds: %zu clouds, at most %d (the cloud is the y coordinate of the grid)",
               clouds, LN_IOU_MAX_CLOUDS);
    LN_REQUIRE(intersection && union_, LN_ERR_ARG, "ln_iou_counts_clouds: null buffer");
    if (n == 0) return LN_OK;  // nothing to add
    LN_REQUIRE(scores && target, LN_ERR_ARG, "ln_iou_counts_clouds: null buffer");
    const size_t need = ln_iou_counts_clouds_workspace_bytes(n, n0, classes);
    LN_REQUIRE(workspace && workspace_bytes >= need, LN_ERR_ARG, "ln_iou_counts_clouds: null / small workspace (%zu bytes needed)", need);
    hipStream_t st = (hipStream_t)stream;
    uint32_t* counts = static_cast<uint32_t*>(workspace);
    const int rc = ln_zero_async(counts, ln_iou_counts_bytes(n, n0, classes), st);
    if (rc != LN_OK) return rc;
    const dim3 grid(ln_div_up(n0, LN_IOU_ROWS), (unsigned)clouds), thr(LN_IOU_THREADS);
    if (classes <= LN_IOU_THREAD_ROW_CLASSES)
        LN_LAUNCH("k_iou_counts_clouds", k_iou_counts_clouds<false>, grid, thr, 0, st, scores, target, n, n0, classes, counts);
    else
        LN_LAUNCH("k_iou_counts_clouds", k_iou_counts_clouds<true>, grid, thr, 0, st, scores, target, n, n0, classes, counts);
    LN_LAUNCH("k_iou_finish_clouds", k_iou_finish_clouds, dim3(ln_div_up(classes, LN_IOU_THREADS)), thr, 0, st, counts, int(clouds), classes,
              unlabeled_index, intersection, union_);
    return ln_check_launch("ln_iou_counts_clouds");
}
