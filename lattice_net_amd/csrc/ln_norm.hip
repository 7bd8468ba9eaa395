// GroupNorm and BatchNorm (+ fused ReLU) on the native [M, C] lattice-value layout, forward and backward, in three forms: GroupNorm over
// the whole matrix, BatchNorm (GroupNorm with one channel per group, plus running statistics) and GroupNorm per row range (the clouds of
// a batch; beyond 64 ranges one workgroup owns one range: k_gn_forward_range_owner, below).  The reference runs torch.nn.GroupNorm on a transposed [1, C, M] view (lattice_modules.py:585-616), two transposed copies in
// each direction; the LNN blocks apply it before every operator, so it sits between any two lattice kernels of the U-Net.
//   statistics : per-channel partial sums over a slab of rows per workgroup (lanes run along the channels of a row: coalesced),
//                combined across workgroups with one fp64 atomic per (workgroup, channel) into LN_GN_REPLICAS accumulator copies
//   apply      : every workgroup rebuilds the per-channel scale/shift from the C channel sums in LDS, then one float4 pass over its rows
// Backward uses the same two shapes: per-channel sums of gy*x and gy, then dx = gy*gamma*rstd + x*c2[g] + c3[g].
// Every step has ONE device body, and a kernel is a shell that resolves its rows and its slabs and calls them: ln_gn_stats_rows (the
// sums; ln_gn_thread_sums is the part of one thread, ln_gn_range_sums the sums of a range by one workgroup), ln_gn_replica_sums,
// ln_gn_channel_affine (ln_gn_affine_of_sums behind the replica loads), ln_gn_affine_rows (y), ln_gn_masked (the ReLU mask), ln_gn_backward_rows (c2 / c3 and
// dx; ln_gn_backward_of_sums behind the replica loads), ln_gn_live_rows / ln_gn_zero_next / ln_gn_zero_tail (the prologue).  A change to a formula is made in one place for every form.
// Every fp32 sum that involves x is a sum of x - p over the LN_GN_PASSES rows of ONE thread, with the pivot p the first of these
// rows: sum (x-p)^2 and sum gy*(x-p) have the size of the spread of those rows, not of their offset from zero, and a pivot that is an
// outlier spoils 16 rows' worth of a sum it is itself a term of, never the whole statistic.  Each thread then puts its pivot back in
// fp64 (sum x = S1 + n p, sum x^2 = S2 + 2 p S1 + n p^2, sum gy x = S + p sum gy): everything from there on, the fold of the
// workgroup, the atomics and E[x^2] - mean^2, is fp64, where the cancellation costs 2^-53, not 2^-24.
#include "ln_common.h"

#define LN_GN_MAX_C 1024
#define LN_GN_PASSES 16
#define LN_GN_REPLICAS 32  // accumulator copies: memory-side atomics serialise per cache line, so spread the workgroups
#define LN_BN_SUM_BATCH 8  // replica loads in flight in the BatchNorm kernels (ln_gn_replica_sums)
#define LN_GN_MAX_SEGMENTS LN_CLOUDS_MAX  // row ranges of one call in the slab form: a 2-D grid and an accumulator slab per range
#define LN_GN_MANY_MAX_SEGMENTS LN_CLOUDS_MANY_MAX  // row ranges of one call (the clouds of a batch: Lattice.set_cloud_batch); beyond
                                                    // LN_GN_MAX_SEGMENTS the range-owner form, one workgroup per range

// The rows that count, 0 <= live <= m (static-rows mode: the tensors are taller than the lattice, *rows_dev rows of them are its rows;
// the rows behind them are excluded from the statistics and written as zeros).  With no live row the forms differ, on purpose: the
// whole-matrix kernels take their statistics with a count of 1 (all sums are zero) and publish them, the per-range kernels leave
// mean_rstd / scale_shift of an empty range untouched.
__device__ __forceinline__ int ln_gn_live_rows(int m, const int* __restrict__ rows_dev) { return max(0, rows_dev ? min(m, *rows_dev) : m); }

// the accumulators of the NEXT call (nobody is using them now: stream order), one share per blockIdx.y, zeroed by its first workgroup
__device__ __forceinline__ void ln_gn_zero_next(double* __restrict__ zero_next, int zero_count) {
    if (!zero_next || blockIdx.x != 0) return;
    const int share = (zero_count + (int)gridDim.y - 1) / (int)gridDim.y;
    const int end = min(zero_count, ((int)blockIdx.y + 1) * share);
    for (int i = (int)blockIdx.y * share + threadIdx.x; i < end; i += 256) zero_next[i] = 0.0;
}

// The storage type T of the [M, C] matrices (x, y, grad_y, grad_x): float or _Float16.  Every body below reaches a matrix through these two
// and nowhere else: the 4 channels of one thread are one 16-byte (fp32) or one 8-byte (fp16) access, `i` counting such quads from `base`.
// An fp16 element is converted to fp32 as it is loaded (exact) and rounded to nearest-even once as it is stored; every operation in
// between is the fp32 / fp64 one of the fp32 instance on the same numbers, in the same order (same rows per thread, same slabs, same
// grids).  The parameters, the statistics and the workspace are fp32 / fp64 for either T.
typedef _Float16 ln_gn_half4 __attribute__((ext_vector_type(4)));

template <typename I>
__device__ __forceinline__ const float4& ln_gn_load4(const float* base, I i) { return reinterpret_cast<const float4*>(base)[i]; }
template <typename I>
__device__ __forceinline__ float4 ln_gn_load4(const _Float16* base, I i) {
    const ln_gn_half4 h = reinterpret_cast<const ln_gn_half4*>(base)[i];
    return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
}
__device__ __forceinline__ void ln_gn_store4(float* base, long long i, float4 v) { reinterpret_cast<float4*>(base)[i] = v; }
__device__ __forceinline__ void ln_gn_store4(_Float16* base, long long i, float4 v) {
    ln_gn_half4 h;
    h.x = (_Float16)v.x;
    h.y = (_Float16)v.y;
    h.z = (_Float16)v.z;
    h.w = (_Float16)v.w;
    reinterpret_cast<ln_gn_half4*>(base)[i] = h;
}

// zeros in the rows of `out` from `live` to m_tensor, spread over the linear_blocks workgroups of the grid
template <typename T>
__device__ __forceinline__ void ln_gn_zero_tail(T* __restrict__ out, int live, int m_tensor, int c, long long linear_block, long long linear_blocks) {
    const long long tensor4 = (long long)m_tensor * c / 4;  // c % 4 == 0 checked by the host
    for (long long i = (long long)live * c / 4 + linear_block * 256 + threadIdx.x; i < tensor4; i += linear_blocks * 256)
        ln_gn_store4(out, i, make_float4(0.f, 0.f, 0.f, 0.f));
}

// gy' of the fused ReLU: the incoming gradient where the forward output x * a + b is positive, zero elsewhere (a NaN output included).
// The mask is decided on this fp32 value for either storage type, never on the rounded fp16 y: a positive x * a + b below half the
// smallest fp16 subnormal is stored as y = 0 and still passes its gradient, as the fp32 instance does on the same x.
__device__ __forceinline__ float ln_gn_masked(float g, float x, float a, float b) { return x * a + b > 0.f ? g : 0.f; }

__device__ __forceinline__ void ln_gn_masked_grad(float4& g, const float4& xv, const float* s_a, const float* s_b, int col) {
    g.x = ln_gn_masked(g.x, xv.x, s_a[col], s_b[col]);
    g.y = ln_gn_masked(g.y, xv.y, s_a[col + 1], s_b[col + 1]);
    g.z = ln_gn_masked(g.z, xv.z, s_a[col + 2], s_b[col + 2]);
    g.w = ln_gn_masked(g.w, xv.w, s_a[col + 3], s_b[col + 3]);
}

// The two sums of ONE thread over its LN_GN_PASSES rows of the slab of rows_per_pass * LN_GN_PASSES rows that starts at row r0, pivot put
// back: pd[j] = sum_rows p(row, 4 qi + j), qd[j] = sum_rows q(row, 4 qi + j)
//   forward  (gy == nullptr): p = x,  q = x*x
//   backward               : p = gy' * x, q = gy'   with gy' = gy masked by (x*a[c] + b[c] > 0) when relu
// A thread owns one float4 (4 channels) of a row; 256 / (c/4) rows are read per pass and LN_GN_PASSES independent
// passes are in flight per thread.  Rows from m on count nowhere; a thread with rp >= rows_per_pass has no row (zeros).
template <typename T>
__device__ __forceinline__ void ln_gn_thread_sums(const T* __restrict__ x, const T* __restrict__ gy, const float* __restrict__ scale_shift,
                                                  int relu, long long r0, int m, int c, double (&pd)[4], double (&qd)[4]) {
    const int tid = threadIdx.x;
    const int quads = c >> 2;                 // c % 4 == 0, c <= 1024  ->  quads <= 256
    const int rows_per_pass = 256 / quads;
    const int rp = tid / quads;
    const int qi = tid - rp * quads;
    const bool live = rp < rows_per_pass;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), q = p;
#pragma unroll
    for (int j = 0; j < 4; ++j) pd[j] = qd[j] = 0.0;
    if (live) {
        float4 a = p, b = p;
        // pivots: this thread's first row (with no row of its own all its terms are zero)
        const float4 pv = r0 + rp < m ? ln_gn_load4(x + (r0 + rp) * c, qi) : p;
        int n = 0;
        if (gy && relu) {
            a = reinterpret_cast<const float4*>(scale_shift)[qi];
            b = reinterpret_cast<const float4*>(scale_shift + c)[qi];
        }
        float4 xv[LN_GN_PASSES], gv[LN_GN_PASSES];
#pragma unroll
        for (int k = 0; k < LN_GN_PASSES; ++k) {
            const long long row = r0 + (long long)k * rows_per_pass + rp;
            const bool ok = row < m;
            n += ok;
            xv[k] = ok ? ln_gn_load4(x + row * c, qi) : pv;  // (x - p = 0 beyond the last row)
            if (gy) gv[k] = ok ? ln_gn_load4(gy + row * c, qi) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < LN_GN_PASSES; ++k) {
            if (gy) {
                float4 g = gv[k];
                if (relu) {
                    g.x = ln_gn_masked(g.x, xv[k].x, a.x, b.x);
                    g.y = ln_gn_masked(g.y, xv[k].y, a.y, b.y);
                    g.z = ln_gn_masked(g.z, xv[k].z, a.z, b.z);
                    g.w = ln_gn_masked(g.w, xv[k].w, a.w, b.w);
                }
                p.x += g.x * (xv[k].x - pv.x); p.y += g.y * (xv[k].y - pv.y); p.z += g.z * (xv[k].z - pv.z); p.w += g.w * (xv[k].w - pv.w);
                q.x += g.x; q.y += g.y; q.z += g.z; q.w += g.w;
            } else {
                const float4 d = make_float4(xv[k].x - pv.x, xv[k].y - pv.y, xv[k].z - pv.z, xv[k].w - pv.w);
                p.x += d.x; p.y += d.y; p.z += d.z; p.w += d.w;
                q.x += d.x * d.x; q.y += d.y * d.y; q.z += d.z * d.z; q.w += d.w * d.w;
            }
        }
        // the pivot goes back in, in fp64
        const float ps[4] = {p.x, p.y, p.z, p.w}, qs[4] = {q.x, q.y, q.z, q.w}, pvs[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double s1 = ps[j], s2 = qs[j], pj = pvs[j];
            pd[j] = gy ? s1 + pj * s2 : s1 + n * pj;
            qd[j] = gy ? s2 : s2 + 2.0 * pj * s1 + n * pj * pj;
        }
    }
}

// acc[c*2 + 0] += sum_rows p(row, c), acc[c*2 + 1] += sum_rows q(row, c), p and q those of ln_gn_thread_sums.  The rows are
// [row_begin, m); workgroup `block` takes the slab of rows_per_pass * LN_GN_PASSES rows that starts that many * block rows behind
// row_begin (k_gn_stats: the whole matrix; k_gn_stats_segments: one row range of it).
template <typename T>
__device__ __forceinline__ void ln_gn_stats_rows(const T* __restrict__ x, const T* __restrict__ gy, const float* __restrict__ scale_shift,
                                                 int relu, int row_begin, int m, int c, double* __restrict__ acc, int block) {
    __shared__ double s_p[256][4], s_q[256][4];
    const int tid = threadIdx.x;
    const int quads = c >> 2;
    const int rows_per_pass = 256 / quads;
    const int rp = tid / quads;
    const int qi = tid - rp * quads;
    const bool live = rp < rows_per_pass;
    double pd[4], qd[4];
    ln_gn_thread_sums(x, gy, scale_shift, relu, row_begin + (long long)block * rows_per_pass * LN_GN_PASSES, m, c, pd, qd);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_p[tid][j] = pd[j];
        s_q[tid][j] = qd[j];
    }
    __syncthreads();
    if (live && rp == 0) {  // fold the threads that share a channel quad, then one fp64 atomic per channel sum
        for (int r = 1; r < rows_per_pass; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pd[j] += s_p[r * quads + qi][j];
                qd[j] += s_q[r * quads + qi][j];
            }
        double* dst = acc + (size_t)(block % LN_GN_REPLICAS) * 2 * c + 8 * qi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            atomicAdd(dst + 2 * j, pd[j]);
            atomicAdd(dst + 2 * j + 1, qd[j]);
        }
    }
}

// The same sums over the rows [lo, hi) taken by ONE workgroup, left in LDS: s_sum[col] = sum p, s_sq[col] = sum q (the range-owner
// kernels: many short ranges, no accumulator slab and no atomic).  The slabs are those of ln_gn_stats_rows, blocked from lo, so every
// fp32 rounding is the one of the other forms; a thread adds its slabs in fp64 in row order, then the threads of a channel quad are
// folded in thread order: one fixed order, the same bits on every run.  All 256 threads call it; it ends with a barrier.
__device__ __forceinline__ void ln_gn_range_sums(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ scale_shift,
                                                 int relu, int lo, int hi, int c, double* s_sum, double* s_sq) {
    __shared__ double s_p[256][4], s_q[256][4];
    const int tid = threadIdx.x;
    const int quads = c >> 2;
    const int rows_per_pass = 256 / quads;
    const int rp = tid / quads;
    const int qi = tid - rp * quads;
    double pd[4] = {0.0, 0.0, 0.0, 0.0}, qd[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (long long r0 = lo; r0 < hi; r0 += rows_per_pass * LN_GN_PASSES) {  // (one trip for a range of up to 16 passes; a long range loops)
        long long slab = r0;
        asm volatile("" : "+s"(slab));  // (opaque: the 32 row addresses are formed per trip as in k_gn_stats, not carried round the loop in 64 VGPRs:
                                        // 276 -> 184 VGPRs in the backward kernel with AMD clang 22.0.0git of ROCm 7.2.0; drop it if a later compiler no longer needs it)
        double p1[4], q1[4];
        ln_gn_thread_sums(x, gy, scale_shift, relu, slab, hi, c, p1, q1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pd[j] += p1[j];
            qd[j] += q1[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_p[tid][j] = pd[j];
        s_q[tid][j] = qd[j];
    }
    __syncthreads();
    if (rp == 0) {
        for (int r = 1; r < rows_per_pass; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pd[j] += s_p[r * quads + qi][j];
                qd[j] += s_q[r * quads + qi][j];
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s_sum[4 * qi + j] = pd[j];
            s_sq[4 * qi + j] = qd[j];
        }
    }
    __syncthreads();
}

// The two fp64 sums of channel `col` over the accumulator replicas, added in replica order, BATCH loads of each in flight at a time.  The
// GroupNorm bodies take all LN_GN_REPLICAS at once (one round trip in the prologue of every workgroup; the registers are free again at the
// barrier that follows).  k_bn_apply and k_bn_backward_eval use the sums in the loop that loads them, where 64 loads in flight cost 156
// VGPRs and with them the occupancy of the float4 pass (8 -> 3 waves, 7.5 -> 9.3 us at [120000, 32] on an MI355X): LN_BN_SUM_BATCH there.
template <int BATCH>
__device__ __forceinline__ void ln_gn_replica_sums(const double* __restrict__ acc, int c, int col, double& s0, double& s1) {
    s0 = 0.0;
    s1 = 0.0;
    for (int r0 = 0; r0 < LN_GN_REPLICAS; r0 += BATCH) {
        double v0[BATCH], v1[BATCH];
#pragma unroll
        for (int r = 0; r < BATCH; ++r) {
            v0[r] = acc[(size_t)(r0 + r) * 2 * c + 2 * col];
            v1[r] = acc[(size_t)(r0 + r) * 2 * c + 2 * col + 1];
        }
#pragma unroll
        for (int r = 0; r < BATCH; ++r) {
            s0 += v0[r];
            s1 += v1[r];
        }
    }
}

// per-channel scale a[c] = gamma*rstd[g], shift b[c] = beta - mean[g]*a[c] from the channel sums over m rows in LDS (s_sum, s_sq: complete
// behind a barrier); block 0 also publishes mean/rstd per group and scale/shift per channel for the backward pass
__device__ __forceinline__ void ln_gn_affine_of_sums(const double* s_sum, const double* s_sq, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int m, int c, int groups, float eps, float* s_a,
                                                     float* s_b, float* __restrict__ mean_rstd, float* __restrict__ scale_shift) {
    if (m < 1) m = 1;  // (an empty lattice under a static row bound: all sums are zero)
    const int cg = c / groups;
    for (int col = threadIdx.x; col < c; col += 256) {
        const int g = col / cg;
        double s = 0.0, ss = 0.0;
        for (int k = 0; k < cg; ++k) {
            s += s_sum[g * cg + k];
            ss += s_sq[g * cg + k];
        }
        const double cnt = (double)m * cg;
        const double mean = s / cnt;
        double var = ss / cnt - mean * mean;  // (fp64 sums of fp32 data: the cancellation costs 2^-53 mean^2 / var)
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const float a = (gamma ? gamma[col] : 1.f) * rstd;
        const float b = (float)((beta ? (double)beta[col] : 0.0) - mean * (double)a);
        s_a[col] = a;
        s_b[col] = b;
        if (blockIdx.x == 0) {
            scale_shift[col] = a;
            scale_shift[c + col] = b;
            if (col == g * cg) {
                mean_rstd[g] = (float)mean;
                mean_rstd[groups + g] = rstd;
            }
        }
    }
}

// ln_gn_affine_of_sums on the channel sums of the accumulator replicas
__device__ __forceinline__ void ln_gn_channel_affine(const double* __restrict__ acc, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int m, int c, int groups, float eps, float* s_a,
                                                     float* s_b, float* __restrict__ mean_rstd, float* __restrict__ scale_shift) {
    __shared__ double s_sum[LN_GN_MAX_C], s_sq[LN_GN_MAX_C];
    for (int col = threadIdx.x; col < c; col += 256) {
        double a0, a1;
        ln_gn_replica_sums<LN_GN_REPLICAS>(acc, c, col, a0, a1);
        s_sum[col] = a0;
        s_sq[col] = a1;
    }
    __syncthreads();
    ln_gn_affine_of_sums(s_sum, s_sq, gamma, beta, m, c, groups, eps, s_a, s_b, mean_rstd, scale_shift);
}

// y = act(x * a[c] + b[c]) over the float4 [first4, last4) of the matrix, the workgroups of blockIdx.y side by side
template <typename T>
__device__ __forceinline__ void ln_gn_affine_rows(const T* __restrict__ x, const float* s_a, const float* s_b, long long first4, long long last4,
                                                  int c, int relu, T* __restrict__ y) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = first4 + (long long)blockIdx.x * 256 + threadIdx.x; i < last4; i += stride) {
        const int col = int((i * 4) % c);
        float4 v = ln_gn_load4(x, i);
        v.x = v.x * s_a[col] + s_b[col];
        v.y = v.y * s_a[col + 1] + s_b[col + 1];
        v.z = v.z * s_a[col + 2] + s_b[col + 2];
        v.w = v.w * s_a[col + 3] + s_b[col + 3];
        if (relu) {
            v.x = fmaxf(v.x, 0.f);
            v.y = fmaxf(v.y, 0.f);
            v.z = fmaxf(v.z, 0.f);
            v.w = fmaxf(v.w, 0.f);
        }
        ln_gn_store4(y, i, v);
    }
}

// dx = gy' * gamma * rstd + x * c2[g] + c3[g] over the float4 [first4, last4) of the matrix, from the channel sums of ln_gn_stats_rows /
// ln_gn_range_sums over `count` rows in LDS (s_ds, s_db: complete behind a barrier; mean_rstd, scale_shift: those of the rows in question).  The first workgroup of the rows also leaves the terms
// of the parameter gradients in LDS, in fp64: term_gamma[col] = (ds - db*mean)*rstd, term_beta[col] = db, each written by the thread that
// owns `col` in a loop `col = threadIdx.x; col < c; col += 256` (which may read them back without a barrier).
template <typename T>
__device__ __forceinline__ void ln_gn_backward_of_sums(const T* __restrict__ x, const T* __restrict__ gy, double* s_ds, double* s_db,
                                                       const float* __restrict__ gamma, const float* __restrict__ mean_rstd,
                                                       const float* __restrict__ scale_shift, int count, long long first4, long long last4, int c,
                                                       int groups, int relu, T* __restrict__ dx, double*& term_gamma, double*& term_beta) {
    __shared__ float s_gr[LN_GN_MAX_C], s_c2[LN_GN_MAX_C], s_c3[LN_GN_MAX_C], s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int cg = c / groups;
    for (int col = threadIdx.x; col < c; col += 256) {
        const int g = col / cg;
        const float mean = mean_rstd[g], rstd = mean_rstd[groups + g];
        double sum1 = 0.0, sum2 = 0.0;  // sum over the group's channels of ds*gamma, db*gamma
        for (int k = 0; k < cg; ++k) {
            const int cc = g * cg + k;
            const double gm = gamma ? (double)gamma[cc] : 1.0;
            sum1 += s_ds[cc] * gm;
            sum2 += s_db[cc] * gm;
        }
        const double cnt = (double)count * cg;
        const double c2 = (sum2 * mean - sum1) * (double)rstd * rstd * rstd / cnt;
        const double c3 = -c2 * mean - sum2 * (double)rstd / cnt;
        s_gr[col] = (gamma ? gamma[col] : 1.f) * rstd;
        s_c2[col] = (float)c2;
        s_c3[col] = (float)c3;
        s_a[col] = scale_shift[col];
        s_b[col] = scale_shift[c + col];
    }
    __syncthreads();
    if (blockIdx.x == 0)  // (behind the barrier: nobody reads another channel's sum any more)
        for (int col = threadIdx.x; col < c; col += 256) {
            const float mean = mean_rstd[col / cg], rstd = mean_rstd[groups + col / cg];
            s_ds[col] = (s_ds[col] - s_db[col] * mean) * rstd;
        }
    term_gamma = s_ds;
    term_beta = s_db;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = first4 + (long long)blockIdx.x * 256 + threadIdx.x; i < last4; i += stride) {
        const int col = int((i * 4) % c);
        const float4 xv = ln_gn_load4(x, i);
        float4 g = ln_gn_load4(gy, i);
        if (relu) ln_gn_masked_grad(g, xv, s_a, s_b, col);
        float4 o;
        o.x = g.x * s_gr[col] + xv.x * s_c2[col] + s_c3[col];
        o.y = g.y * s_gr[col + 1] + xv.y * s_c2[col + 1] + s_c3[col + 1];
        o.z = g.z * s_gr[col + 2] + xv.z * s_c2[col + 2] + s_c3[col + 2];
        o.w = g.w * s_gr[col + 3] + xv.w * s_c2[col + 3] + s_c3[col + 3];
        ln_gn_store4(dx, i, o);
    }
}

// ln_gn_backward_of_sums on the channel sums of the accumulator replicas
template <typename T>
__device__ __forceinline__ void ln_gn_backward_rows(const T* __restrict__ x, const T* __restrict__ gy, const double* __restrict__ acc,
                                                    const float* __restrict__ gamma, const float* __restrict__ mean_rstd,
                                                    const float* __restrict__ scale_shift, int count, long long first4, long long last4, int c,
                                                    int groups, int relu, T* __restrict__ dx, double*& term_gamma, double*& term_beta) {
    __shared__ double s_ds[LN_GN_MAX_C], s_db[LN_GN_MAX_C];
    for (int col = threadIdx.x; col < c; col += 256) {
        double ds, db;
        ln_gn_replica_sums<LN_GN_REPLICAS>(acc, c, col, ds, db);
        s_ds[col] = ds;
        s_db[col] = db;
    }
    __syncthreads();
    ln_gn_backward_of_sums(x, gy, s_ds, s_db, gamma, mean_rstd, scale_shift, count, first4, last4, c, groups, relu, dx, term_gamma, term_beta);
}

__global__ void __launch_bounds__(256)
    k_gn_stats(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ scale_shift, int relu, int m, int c,
               double* __restrict__ acc, const int* __restrict__ rows_dev) {
    ln_gn_stats_rows(x, gy, scale_shift, relu, 0, ln_gn_live_rows(m, rows_dev), c, acc, blockIdx.x);
}

__global__ void __launch_bounds__(256)
    k_gn_apply(const float* __restrict__ x, const double* __restrict__ acc, const float* __restrict__ gamma, const float* __restrict__ beta,
               int m, int c, int groups, float eps, int relu, float* __restrict__ y, float* __restrict__ mean_rstd,
               float* __restrict__ scale_shift, double* __restrict__ zero_next, int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int live = ln_gn_live_rows(m, rows_dev);
    ln_gn_zero_next(zero_next, zero_count);
    ln_gn_channel_affine(acc, gamma, beta, live, c, groups, eps, s_a, s_b, mean_rstd, scale_shift);
    __syncthreads();
    ln_gn_zero_tail(y, live, m, c, blockIdx.x, gridDim.x);
    ln_gn_affine_rows(x, s_a, s_b, 0, (long long)live * c / 4, c, relu, y);
}

// block 0 rounds the terms of ln_gn_backward_rows to dgamma, dbeta
__global__ void __launch_bounds__(256)
    k_gn_backward_apply(const float* __restrict__ x, const float* __restrict__ gy, const double* __restrict__ acc,
                        const float* __restrict__ gamma, const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift, int m,
                        int c, int groups, int relu, float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                        double* __restrict__ zero_next, int zero_count, const int* __restrict__ rows_dev) {
    const int live = ln_gn_live_rows(m, rows_dev);
    ln_gn_zero_next(zero_next, zero_count);
    ln_gn_zero_tail(dx, live, m, c, blockIdx.x, gridDim.x);
    double *term_gamma, *term_beta;
    ln_gn_backward_rows(x, gy, acc, gamma, mean_rstd, scale_shift, max(live, 1), 0, (long long)live * c / 4, c, groups, relu, dx, term_gamma,
                        term_beta);
    if (blockIdx.x == 0)
        for (int col = threadIdx.x; col < c; col += 256) {
            if (dgamma) dgamma[col] = (float)term_gamma[col];
            if (dbeta) dbeta[col] = (float)term_beta[col];
        }
}

// ---- BatchNorm: GroupNorm with one channel per group, plus running statistics --------------------------------------------------------
// Training: k_gn_stats gives the fp64 channel sums exactly as for GroupNorm (same summation, same bounds), k_bn_apply turns them into
// scale / shift and moves the running statistics on the device; the backward is k_gn_backward_apply at groups == channels.
// Evaluation: the statistics are the running ones, constants of the step: one launch forward; backward dx = gy' * a, and the
// parameter gradients from the same k_gn_stats sums.

// Training forward.  Every workgroup rebuilds a = gamma * rstd, b = beta - mean * a from the fp64 channel sums (biased variance, clamped
// at 0; n = live rows); block 0 publishes mean_rstd / scale_shift and, with n >= 2, moves the running statistics (unbiased variance),
// each formed in fp64 and rounded once.  With n < 2 the running statistics keep their bits.
__global__ void __launch_bounds__(256)
    k_bn_apply(const float* __restrict__ x, const double* __restrict__ acc, const float* __restrict__ gamma, const float* __restrict__ beta,
               float* __restrict__ running_mean, float* __restrict__ running_var, int m, int c, float eps, double momentum, int relu,
               float* __restrict__ y, float* __restrict__ mean_rstd, float* __restrict__ scale_shift, double* __restrict__ zero_next,
               int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int live = ln_gn_live_rows(m, rows_dev);
    ln_gn_zero_next(zero_next, zero_count);
    const double cnt = live < 1 ? 1.0 : (double)live;  // (an empty lattice under a static row bound: all sums are zero)
    for (int col = threadIdx.x; col < c; col += 256) {
        double s, ss;
        ln_gn_replica_sums<LN_BN_SUM_BATCH>(acc, c, col, s, ss);
        const double mean = s / cnt;
        double var = ss / cnt - mean * mean;  // (fp64 sums of fp32 data: the cancellation costs 2^-53 mean^2 / var)
        if (var < 0.0) var = 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        const float a = (gamma ? gamma[col] : 1.f) * rstd;
        const float b = (float)((beta ? (double)beta[col] : 0.0) - mean * (double)a);
        s_a[col] = a;
        s_b[col] = b;
        if (blockIdx.x == 0) {
            mean_rstd[col] = (float)mean;
            mean_rstd[c + col] = rstd;
            scale_shift[col] = a;
            scale_shift[c + col] = b;
            if (running_mean && live >= 2) {  // (one row has no unbiased variance: nothing moves)
                running_mean[col] = (float)((1.0 - momentum) * (double)running_mean[col] + momentum * mean);
                running_var[col] = (float)((1.0 - momentum) * (double)running_var[col] + momentum * (var * (cnt / (cnt - 1.0))));
            }
        }
    }
    __syncthreads();
    ln_gn_zero_tail(y, live, m, c, blockIdx.x, gridDim.x);
    ln_gn_affine_rows(x, s_a, s_b, 0, (long long)live * c / 4, c, relu, y);
}

// Evaluation forward: a = gamma / sqrt(running_var + eps) (rstd formed in fp64, rounded once), b = beta - running_mean * a (fp64, rounded
// once).  Reads the running statistics, never writes them.
__global__ void __launch_bounds__(256)
    k_bn_apply_eval(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                    const float* __restrict__ running_mean, const float* __restrict__ running_var, int m, int c, float eps, int relu,
                    float* __restrict__ y, float* __restrict__ mean_rstd, float* __restrict__ scale_shift, double* __restrict__ zero_next,
                    int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int live = ln_gn_live_rows(m, rows_dev);
    ln_gn_zero_next(zero_next, zero_count);
    for (int col = threadIdx.x; col < c; col += 256) {
        const float mean = running_mean[col];
        const float rstd = (float)(1.0 / sqrt((double)running_var[col] + (double)eps));
        const float a = (gamma ? gamma[col] : 1.f) * rstd;
        const float b = (float)((beta ? (double)beta[col] : 0.0) - (double)mean * (double)a);
        s_a[col] = a;
        s_b[col] = b;
        if (blockIdx.x == 0) {
            mean_rstd[col] = mean;
            mean_rstd[c + col] = rstd;
            scale_shift[col] = a;
            scale_shift[c + col] = b;
        }
    }
    __syncthreads();
    ln_gn_zero_tail(y, live, m, c, blockIdx.x, gridDim.x);
    ln_gn_affine_rows(x, s_a, s_b, 0, (long long)live * c / 4, c, relu, y);
}

// Evaluation backward: dx = gy' * a (its own loop: no c2 / c3, and x is read only for the mask);  block 0 writes
// dgamma = (ds - db * running_mean) * rstd, dbeta = db in fp64 from the k_gn_stats sums (acc == nullptr: no parameter gradient is wanted
// and no sums were taken).
__global__ void __launch_bounds__(256)
    k_bn_backward_eval(const float* __restrict__ x, const float* __restrict__ gy, const double* __restrict__ acc,
                       const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift, int m, int c, int relu,
                       float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta, double* __restrict__ zero_next,
                       int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int live = ln_gn_live_rows(m, rows_dev);
    ln_gn_zero_next(zero_next, zero_count);
    for (int col = threadIdx.x; col < c; col += 256) {
        s_a[col] = scale_shift[col];
        s_b[col] = scale_shift[c + col];
        if (acc && blockIdx.x == 0) {
            double ds, db;
            ln_gn_replica_sums<LN_BN_SUM_BATCH>(acc, c, col, ds, db);
            if (dgamma) dgamma[col] = (float)((ds - db * (double)mean_rstd[col]) * (double)mean_rstd[c + col]);
            if (dbeta) dbeta[col] = (float)db;
        }
    }
    __syncthreads();
    ln_gn_zero_tail(dx, live, m, c, blockIdx.x, gridDim.x);
    const long long total4 = (long long)live * c / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
        const int col = int((i * 4) % c);
        float4 g = reinterpret_cast<const float4*>(gy)[i];
        if (relu) ln_gn_masked_grad(g, reinterpret_cast<const float4*>(x)[i], s_a, s_b, col);
        reinterpret_cast<float4*>(dx)[i] = make_float4(g.x * s_a[col], g.y * s_a[col + 1], g.z * s_a[col + 2], g.w * s_a[col + 3]);
    }
}

// ---- GroupNorm per row range: a batch of clouds in one table (LnTable.batch_points) ------------------------------------------------
// In first-occurrence row order the vertices of cloud s are the rows [row_starts[s], row_starts[s + 1]) of the value matrix (the points
// of a batch are cloud-major and clouds share no vertex), so per-cloud GroupNorm is the GroupNorm above over B row ranges: blockIdx.y is
// the range, its workgroups block the rows from the START of the range (the pivot of a thread is a row of its own range, the summation
// inside a range is the one of k_gn_stats over that many rows), and range s owns accumulator slab s (LN_GN_REPLICAS x 2 x C doubles).
// The rows from row_starts[B] (clamped by *rows_dev and the tensor height) to the tensor height are written as zeros and count nowhere.

// One thread per row: a row whose cloud differs from its predecessor's is where the clouds in between start.  The cloud of a row is read
// from the first coordinate of its key: cloud s is shifted by s * batch_key_step and stays within half a step of the origin, at every
// level (a coarser level halves both the keys and the step).  flag (zeroed in front of the launch): set when a row's cloud is smaller
// than its predecessor's, i.e. the rows are not cloud-major and row_starts is not usable.
__global__ void __launch_bounds__(256) k_cloud_row_starts(LnTable t, int rows_upper, int clouds, int* __restrict__ row_starts, int* __restrict__ flag) {
    int m = min(*t.nr_filled, rows_upper);
    if (t.row_limit > 0) m = min(m, t.row_limit);  // (a build leaves vertices beyond the limit un-inserted: no keys[] row)
    m = max(m, 0);
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > m) return;
    const long long step = t.batch_key_step, half = step >> 1;
    int prev = -1, cur = clouds;  // (row -1 belongs to no cloud; row m closes every cloud that is left)
    if (r > 0) {
        const long long k = (long long)t.keys[(size_t)(r - 1) * t.pos_dim] + half;
        prev = int(min(max((k >= 0 ? k : k - step + 1) / step, 0ll), (long long)clouds - 1));
    }
    if (r < m) {
        const long long k = (long long)t.keys[(size_t)r * t.pos_dim] + half;
        cur = int(min(max((k >= 0 ? k : k - step + 1) / step, 0ll), (long long)clouds - 1));
    }
    if (cur < prev) *flag = 1;
    for (int s = prev + 1; s <= cur; ++s) row_starts[s] = r;  // (clouds without a vertex start where the next one does)
}

// rows [lo, hi) of range s, clamped to 0 <= lo <= hi <= live whatever row_starts holds (nothing is indexed outside the tensors); live = the rows that count
__device__ __forceinline__ void ln_gn_segment(const int* __restrict__ row_starts, int segments, int s, int m, const int* __restrict__ rows_dev,
                                              int& live, int& lo, int& hi) {
    live = ln_gn_live_rows(min(m, row_starts[segments]), rows_dev);
    lo = min(max(row_starts[s], 0), live);
    hi = min(max(row_starts[s + 1], lo), live);
}

__global__ void __launch_bounds__(256)
    k_gn_stats_segments(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ scale_shift, int relu, int m, int c,
                        double* __restrict__ acc, const int* __restrict__ rows_dev, const int* __restrict__ row_starts, int segments) {
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    // (the grid covers a range of m rows: the workgroups behind the end of this range, all of them for an empty one, have nothing to add)
    if ((long long)blockIdx.x * (256 / (c >> 2)) * LN_GN_PASSES >= hi - lo) return;
    ln_gn_stats_rows(x, gy, scale_shift ? scale_shift + (size_t)s * 2 * c : nullptr, relu, lo, hi, c, acc + (size_t)s * LN_GN_REPLICAS * 2 * c,
                     blockIdx.x);
}

__global__ void __launch_bounds__(256)
    k_gn_stats_segments_f16(const _Float16* __restrict__ x, const _Float16* __restrict__ gy, const float* __restrict__ scale_shift, int relu, int m,
                            int c, double* __restrict__ acc, const int* __restrict__ rows_dev, const int* __restrict__ row_starts, int segments) {
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    // (the grid covers a range of m rows: the workgroups behind the end of this range, all of them for an empty one, have nothing to add)
    if ((long long)blockIdx.x * (256 / (c >> 2)) * LN_GN_PASSES >= hi - lo) return;
    ln_gn_stats_rows(x, gy, scale_shift ? scale_shift + (size_t)s * 2 * c : nullptr, relu, lo, hi, c, acc + (size_t)s * LN_GN_REPLICAS * 2 * c,
                     blockIdx.x);
}

// the prologue of the two apply kernels: the next call's accumulators, and zeros in the rows behind the last range (all workgroups of the 2-D grid)
template <typename T>
__device__ __forceinline__ void ln_gn_segments_housekeeping(double* __restrict__ zero_next, int zero_count, int live, int m, int c,
                                                            T* __restrict__ out) {
    ln_gn_zero_next(zero_next, zero_count);
    ln_gn_zero_tail(out, live, m, c, (long long)blockIdx.y * gridDim.x + blockIdx.x, (long long)gridDim.x * gridDim.y);
}

__global__ void __launch_bounds__(256)
    k_gn_apply_segments(const float* __restrict__ x, const double* __restrict__ acc, const float* __restrict__ gamma, const float* __restrict__ beta,
                        int m, int c, int groups, float eps, int relu, float* __restrict__ y, float* __restrict__ mean_rstd,
                        float* __restrict__ scale_shift, double* __restrict__ zero_next, int zero_count, const int* __restrict__ rows_dev,
                        const int* __restrict__ row_starts, int segments) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    ln_gn_segments_housekeeping(zero_next, zero_count, live, m, c, y);
    if (hi == lo) return;  // an empty range: no statistics, no rows
    ln_gn_channel_affine(acc + (size_t)s * LN_GN_REPLICAS * 2 * c, gamma, beta, hi - lo, c, groups, eps, s_a, s_b, mean_rstd + (size_t)s * 2 * groups,
                         scale_shift + (size_t)s * 2 * c);
    __syncthreads();
    ln_gn_affine_rows(x, s_a, s_b, (long long)lo * c / 4, (long long)hi * c / 4, c, relu, y);
}

__global__ void __launch_bounds__(256)
    k_gn_apply_segments_f16(const _Float16* __restrict__ x, const double* __restrict__ acc, const float* __restrict__ gamma,
                            const float* __restrict__ beta, int m, int c, int groups, float eps, int relu, _Float16* __restrict__ y,
                            float* __restrict__ mean_rstd, float* __restrict__ scale_shift, double* __restrict__ zero_next, int zero_count,
                            const int* __restrict__ rows_dev, const int* __restrict__ row_starts, int segments) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    ln_gn_segments_housekeeping(zero_next, zero_count, live, m, c, y);
    if (hi == lo) return;  // an empty range: no statistics, no rows
    ln_gn_channel_affine(acc + (size_t)s * LN_GN_REPLICAS * 2 * c, gamma, beta, hi - lo, c, groups, eps, s_a, s_b, mean_rstd + (size_t)s * 2 * groups,
                         scale_shift + (size_t)s * 2 * c);
    __syncthreads();
    ln_gn_affine_rows(x, s_a, s_b, (long long)lo * c / 4, (long long)hi * c / 4, c, relu, y);
}

// ln_gn_backward_rows over range blockIdx.y.  The parameter gradients are sums over the ranges: the first workgroup of range s leaves its
// terms in parts[s * 2 C ...], in fp64 (zeros for an empty range); k_gn_param_grads_segments adds them.
__global__ void __launch_bounds__(256)
    k_gn_backward_apply_segments(const float* __restrict__ x, const float* __restrict__ gy, const double* __restrict__ acc,
                                 const float* __restrict__ gamma, const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift, int m,
                                 int c, int groups, int relu, float* __restrict__ dx, double* __restrict__ parts, double* __restrict__ zero_next,
                                 int zero_count, const int* __restrict__ rows_dev, const int* __restrict__ row_starts, int segments) {
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    ln_gn_segments_housekeeping(zero_next, zero_count, live, m, c, dx);
    parts += (size_t)s * 2 * c;
    if (hi == lo) {
        if (blockIdx.x == 0)
            for (int i = threadIdx.x; i < 2 * c; i += 256) parts[i] = 0.0;
        return;
    }
    double *term_gamma, *term_beta;
    ln_gn_backward_rows(x, gy, acc + (size_t)s * LN_GN_REPLICAS * 2 * c, gamma, mean_rstd + (size_t)s * 2 * groups, scale_shift + (size_t)s * 2 * c,
                        hi - lo, (long long)lo * c / 4, (long long)hi * c / 4, c, groups, relu, dx, term_gamma, term_beta);
    if (blockIdx.x == 0)
        for (int col = threadIdx.x; col < c; col += 256) {
            parts[col] = term_gamma[col];
            parts[c + col] = term_beta[col];
        }
}

__global__ void __launch_bounds__(256)
    k_gn_backward_apply_segments_f16(const _Float16* __restrict__ x, const _Float16* __restrict__ gy, const double* __restrict__ acc,
                                     const float* __restrict__ gamma, const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift,
                                     int m, int c, int groups, int relu, _Float16* __restrict__ dx, double* __restrict__ parts,
                                     double* __restrict__ zero_next, int zero_count, const int* __restrict__ rows_dev,
                                     const int* __restrict__ row_starts, int segments) {
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    ln_gn_segments_housekeeping(zero_next, zero_count, live, m, c, dx);
    parts += (size_t)s * 2 * c;
    if (hi == lo) {
        if (blockIdx.x == 0)
            for (int i = threadIdx.x; i < 2 * c; i += 256) parts[i] = 0.0;
        return;
    }
    double *term_gamma, *term_beta;
    ln_gn_backward_rows(x, gy, acc + (size_t)s * LN_GN_REPLICAS * 2 * c, gamma, mean_rstd + (size_t)s * 2 * groups, scale_shift + (size_t)s * 2 * c,
                        hi - lo, (long long)lo * c / 4, (long long)hi * c / 4, c, groups, relu, dx, term_gamma, term_beta);
    if (blockIdx.x == 0)
        for (int col = threadIdx.x; col < c; col += 256) {
            parts[col] = term_gamma[col];
            parts[c + col] = term_beta[col];
        }
}

// dgamma[col] = sum_s parts[s][col], dbeta[col] = sum_s parts[s][C + col]: fp64, ranges added in order, one rounding to fp32
__global__ void __launch_bounds__(256)
    k_gn_param_grads_segments(const double* __restrict__ parts, int segments, int c, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // < 2 C: the first C are dgamma
    if (i >= 2 * c) return;
    double sum = 0.0;
    for (int s0 = 0; s0 < segments; s0 += 8) {  // eight loads in flight
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = s0 + k < segments ? parts[(size_t)(s0 + k) * 2 * c + i] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += v[k];
    }
    float* out = i < c ? dgamma : dbeta;
    if (out) out[i < c ? i : i - c] = (float)sum;
}

// ---- GroupNorm per row range, many short ranges (LN_GN_MAX_SEGMENTS < B <= LN_GN_MANY_MAX_SEGMENTS): one workgroup owns one range ----
// A grid sized for the whole matrix once per range, and an accumulator slab per range that has to be zero, are what the kernels above
// cost per range; at 1024 ranges of a few dozen rows that is a thousand times the useful workgroups and 32 MB of zero fill per call.
// Here the grid is (1, B): workgroup blockIdx.y takes the sums of its range alone (ln_gn_range_sums: LDS, fixed order, no slab, no
// atomic), and behind a barrier walks the range a second time (from L2: a range of 40 rows x 64 channels is 10 KB) to write y, or dx.
// The grid is (1, B) and not (B, 1) because the shared bodies stride their rows by gridDim.x and publish from blockIdx.x == 0: with one
// workgroup in x they are the owner's loop as they stand, and ln_gn_zero_next gives every owner a share of the next call's accumulators.
// A range of any length is correct, the owner loops over it, but it is walked by ONE workgroup of the chip's 256 CUs: a 100 000-row
// range among 200 short ones takes as long as that range alone on one CU.  The host takes this form only beyond LN_GN_MAX_SEGMENTS
// ranges, where the ranges of a batch that fits one table are short.
__global__ void __launch_bounds__(256)
    k_gn_forward_range_owner(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, int m, int c, int groups,
                             float eps, int relu, float* __restrict__ y, float* __restrict__ mean_rstd, float* __restrict__ scale_shift,
                             double* __restrict__ zero_next, int zero_count, const int* __restrict__ rows_dev,
                             const int* __restrict__ row_starts, int segments) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    __shared__ double s_sum[LN_GN_MAX_C], s_sq[LN_GN_MAX_C];
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    ln_gn_segments_housekeeping(zero_next, zero_count, live, m, c, y);
    if (hi == lo) return;  // an empty range: no statistics, no rows
    ln_gn_range_sums(x, nullptr, nullptr, 0, lo, hi, c, s_sum, s_sq);
    ln_gn_affine_of_sums(s_sum, s_sq, gamma, beta, hi - lo, c, groups, eps, s_a, s_b, mean_rstd + (size_t)s * 2 * groups,
                         scale_shift + (size_t)s * 2 * c);
    __syncthreads();
    ln_gn_affine_rows(x, s_a, s_b, (long long)lo * c / 4, (long long)hi * c / 4, c, relu, y);
}

// The owner of range s takes the sums of gy' x and gy' over its range, writes dx and leaves its terms of the parameter gradients in
// parts[s * 2 C ...] (zeros for an empty range) for k_gn_param_grads_segments.
__global__ void __launch_bounds__(256)
    k_gn_backward_range_owner(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ gamma,
                              const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift, int m, int c, int groups, int relu,
                              float* __restrict__ dx, double* __restrict__ parts, double* __restrict__ zero_next, int zero_count,
                              const int* __restrict__ rows_dev, const int* __restrict__ row_starts, int segments) {
    __shared__ double s_ds[LN_GN_MAX_C], s_db[LN_GN_MAX_C];
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    ln_gn_segments_housekeeping(zero_next, zero_count, live, m, c, dx);
    parts += (size_t)s * 2 * c;
    if (hi == lo) {
        for (int i = threadIdx.x; i < 2 * c; i += 256) parts[i] = 0.0;
        return;
    }
    scale_shift += (size_t)s * 2 * c;
    ln_gn_range_sums(x, gy, scale_shift, relu, lo, hi, c, s_ds, s_db);
    double *term_gamma, *term_beta;
    ln_gn_backward_of_sums(x, gy, s_ds, s_db, gamma, mean_rstd + (size_t)s * 2 * groups, scale_shift, hi - lo, (long long)lo * c / 4,
                           (long long)hi * c / 4, c, groups, relu, dx, term_gamma, term_beta);
    for (int col = threadIdx.x; col < c; col += 256) {
        parts[col] = term_gamma[col];
        parts[c + col] = term_beta[col];
    }
}

static int ln_gn_check(const char* who, int m, int c, int groups) {
    LN_REQUIRE(m >= 1 && c >= 4 && c <= LN_GN_MAX_C && c % 4 == 0, LN_ERR_UNSUPPORTED, "%s: need 1 <= rows, channels %% 4 == 0 and <= %d (got %d x %d)",
               who, LN_GN_MAX_C, m, c);
    LN_REQUIRE(groups >= 1 && c % groups == 0, LN_ERR_ARG, "%s: %d groups do not divide %d channels", who, groups, c);
    return LN_OK;
}

// The storage type of the [M, C] matrices of a call, by its element size: what the host function behind an fp32 / fp16 pair of entry
// points is told, and what it picks the kernel instances by.
enum LnGnStorage { LN_GN_F16 = 2, LN_GN_F32 = 4 };

// The buffers of a call: its [M, C] matrices (x, y forward; x, grad_y, grad_x backward) non-null and aligned to the 4 elements a thread
// accesses at once (16 bytes in fp32, 8 in fp16), mean_rstd / scale_shift non-null, `workspace` non-null with at least `need` bytes
// (need == 0: a call that takes no sums and leaves `workspace` alone), both workspaces 8-byte aligned.
static int ln_norm_check_buffers(const char* who, const void* x, const void* grad_y, const void* out, const void* mean_rstd, const void* scale_shift,
                                 const void* workspace, size_t workspace_bytes, size_t need, const void* next_workspace, bool backward,
                                 LnGnStorage storage = LN_GN_F32) {
    LN_REQUIRE(x && out && mean_rstd && scale_shift && (grad_y || !backward), LN_ERR_ARG, "%s: null buffer", who);
    LN_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), LN_ERR_ARG, "%s: null workspace, or smaller than %zu bytes", who, need);
    const uintptr_t align = 4 * (uintptr_t)storage;
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(grad_y) | reinterpret_cast<uintptr_t>(out)) & (align - 1)) == 0, LN_ERR_ARG,
               "%s: the [rows, channels] matrices must be %d-byte aligned", who, (int)align);
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(next_workspace)) & 7) == 0, LN_ERR_ARG,
               "%s: the workspaces must be 8-byte aligned", who);
    return LN_OK;
}

static int ln_gn_stats_grid(int m, int c) {
    const int rows_per_pass = 256 / (c / 4);
    return ln_div_up(m, rows_per_pass * LN_GN_PASSES);
}

static int ln_gn_apply_grid(int m, int c) {
    const long long total4 = (long long)m * c / 4;
    int grid = ln_div_up(total4, 256 * 4);
    if (grid > 2048) grid = 2048;
    return grid < 1 ? 1 : grid;
}

extern "C" size_t ln_group_norm_workspace_bytes(int channels) { return (size_t)LN_GN_REPLICAS * 2 * channels * sizeof(double); }

extern "C" int ln_group_norm_forward_rows(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                          int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                          void* next_workspace, size_t next_workspace_bytes, const int* rows_device, void* stream) {
    int rc = ln_gn_check("ln_group_norm_forward", m, channels, groups);
    if (rc) return rc;
    rc = ln_norm_check_buffers("ln_group_norm_forward", x, nullptr, y, mean_rstd, scale_shift, workspace, workspace_bytes,
                               ln_group_norm_workspace_bytes(channels), next_workspace, false);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* acc = static_cast<double*>(workspace);
    // next_workspace != NULL: the caller alternates two workspaces and promises `workspace` is zero (it was `next_workspace` of
    // the previous call on this stream, or freshly zeroed); this call zero-fills `next_workspace` on its way out.
    if (!next_workspace && ln_zero_async(acc, ln_group_norm_workspace_bytes(channels), st) != LN_OK)
        return ln_check_launch("ln_group_norm_forward(memset)");
    LN_LAUNCH("k_gn_stats", k_gn_stats, dim3(ln_gn_stats_grid(m, channels)), dim3(256), 0, st, x, (const float*)nullptr, (const float*)nullptr, 0, m,
              channels, acc, rows_device);
    LN_LAUNCH("k_gn_apply", k_gn_apply, dim3(ln_gn_apply_grid(m, channels)), dim3(256), 0, st, x, acc, gamma, beta, m, channels, groups, eps, relu, y,
              mean_rstd, scale_shift, static_cast<double*>(next_workspace), int(next_workspace_bytes / sizeof(double)), rows_device);
    return ln_check_launch("ln_group_norm_forward");
}

extern "C" int ln_group_norm_forward(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                     int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                     void* next_workspace, size_t next_workspace_bytes, void* stream) {
    return ln_group_norm_forward_rows(x, gamma, beta, m, channels, groups, eps, relu, y, mean_rstd, scale_shift, workspace, workspace_bytes,
                                      next_workspace, next_workspace_bytes, nullptr, stream);
}

extern "C" int ln_group_norm_backward_rows(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                           const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                           float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace,
                                           size_t next_workspace_bytes, const int* rows_device, void* stream) {
    int rc = ln_gn_check("ln_group_norm_backward", m, channels, groups);
    if (rc) return rc;
    rc = ln_norm_check_buffers("ln_group_norm_backward", x, grad_y, grad_x, mean_rstd, scale_shift, workspace, workspace_bytes,
                               ln_group_norm_workspace_bytes(channels), next_workspace, true);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* acc = static_cast<double*>(workspace);
    if (!next_workspace && ln_zero_async(acc, ln_group_norm_workspace_bytes(channels), st) != LN_OK)
        return ln_check_launch("ln_group_norm_backward(memset)");
    LN_LAUNCH("k_gn_stats", k_gn_stats, dim3(ln_gn_stats_grid(m, channels)), dim3(256), 0, st, x, grad_y, scale_shift, relu, m, channels, acc, rows_device);
    LN_LAUNCH("k_gn_backward_apply", k_gn_backward_apply, dim3(ln_gn_apply_grid(m, channels)), dim3(256), 0, st, x, grad_y, acc, gamma, mean_rstd,
              scale_shift, m, channels, groups, relu, grad_x, grad_gamma, grad_beta, static_cast<double*>(next_workspace),
              int(next_workspace_bytes / sizeof(double)), rows_device);
    return ln_check_launch("ln_group_norm_backward");
}

extern "C" int ln_group_norm_backward(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                      const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                      float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, void* stream) {
    return ln_group_norm_backward_rows(x, grad_y, gamma, mean_rstd, scale_shift, m, channels, groups, relu, grad_x, grad_gamma, grad_beta, workspace,
                                       workspace_bytes, next_workspace, next_workspace_bytes, nullptr, stream);
}

extern "C" size_t ln_batch_norm_workspace_bytes(int channels) { return ln_group_norm_workspace_bytes(channels); }

extern "C" int ln_batch_norm_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, int m,
                                     int channels, float eps, double momentum, int training, int relu, float* y, float* mean_rstd,
                                     float* scale_shift, void* workspace, size_t workspace_bytes, void* next_workspace,
                                     size_t next_workspace_bytes, const int* rows_device, void* stream) {
    int rc = ln_gn_check("ln_batch_norm_forward", m, channels, channels);
    if (rc) return rc;
    LN_REQUIRE(!running_mean == !running_var, LN_ERR_ARG, "ln_batch_norm_forward: running_mean and running_var come together or not at all");
    LN_REQUIRE(training || running_mean, LN_ERR_ARG, "ln_batch_norm_forward: evaluation mode needs the running statistics");
    rc = ln_norm_check_buffers("ln_batch_norm_forward", x, nullptr, y, mean_rstd, scale_shift, workspace, workspace_bytes,
                               training ? ln_batch_norm_workspace_bytes(channels) : 0, next_workspace, false);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* zero_next = static_cast<double*>(next_workspace);
    const int zero_count = int(next_workspace_bytes / sizeof(double));
    if (!training) {  // the running statistics are the statistics: no sums, `workspace` is not touched
        LN_LAUNCH("k_bn_apply_eval", k_bn_apply_eval, dim3(ln_gn_apply_grid(m, channels)), dim3(256), 0, st, x, gamma, beta,
                  (const float*)running_mean, (const float*)running_var, m, channels, eps, relu, y, mean_rstd, scale_shift, zero_next, zero_count,
                  rows_device);
        return ln_check_launch("ln_batch_norm_forward");
    }
    double* acc = static_cast<double*>(workspace);
    if (!next_workspace && ln_zero_async(acc, ln_batch_norm_workspace_bytes(channels), st) != LN_OK)
        return ln_check_launch("ln_batch_norm_forward(memset)");
    LN_LAUNCH("k_gn_stats", k_gn_stats, dim3(ln_gn_stats_grid(m, channels)), dim3(256), 0, st, x, (const float*)nullptr, (const float*)nullptr, 0, m,
              channels, acc, rows_device);
    LN_LAUNCH("k_bn_apply", k_bn_apply, dim3(ln_gn_apply_grid(m, channels)), dim3(256), 0, st, x, (const double*)acc, gamma, beta, running_mean,
              running_var, m, channels, eps, momentum, relu, y, mean_rstd, scale_shift, zero_next, zero_count, rows_device);
    return ln_check_launch("ln_batch_norm_forward");
}

extern "C" int ln_batch_norm_backward(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd, const float* scale_shift,
                                      int m, int channels, int training, int relu, float* grad_x, float* grad_gamma, float* grad_beta,
                                      void* workspace, size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes,
                                      const int* rows_device, void* stream) {
    int rc = ln_gn_check("ln_batch_norm_backward", m, channels, channels);
    if (rc) return rc;
    rc = ln_norm_check_buffers("ln_batch_norm_backward", x, grad_y, grad_x, mean_rstd, scale_shift, workspace, workspace_bytes,
                               ln_batch_norm_workspace_bytes(channels), next_workspace, true);
    if (rc) return rc;
    if (training)  // GroupNorm with one channel per group: the same sums, the same formula (the arguments were checked above)
        return ln_group_norm_backward_rows(x, grad_y, gamma, mean_rstd, scale_shift, m, channels, channels, relu, grad_x, grad_gamma, grad_beta,
                                           workspace, workspace_bytes, next_workspace, next_workspace_bytes, rows_device, stream);
    hipStream_t st = (hipStream_t)stream;
    double* acc = static_cast<double*>(workspace);
    const bool sums = grad_gamma || grad_beta;  // (without parameter gradients dx = gy' * a needs no sum: `workspace` stays as it is)
    if (sums) {
        if (!next_workspace && ln_zero_async(acc, ln_batch_norm_workspace_bytes(channels), st) != LN_OK)
            return ln_check_launch("ln_batch_norm_backward(memset)");
        LN_LAUNCH("k_gn_stats", k_gn_stats, dim3(ln_gn_stats_grid(m, channels)), dim3(256), 0, st, x, grad_y, scale_shift, relu, m, channels, acc,
                  rows_device);
    }
    LN_LAUNCH("k_bn_backward_eval", k_bn_backward_eval, dim3(ln_gn_apply_grid(m, channels)), dim3(256), 0, st, x, grad_y,
              sums ? (const double*)acc : (const double*)nullptr, mean_rstd, scale_shift, m, channels, relu, grad_x, grad_gamma, grad_beta,
              static_cast<double*>(next_workspace), int(next_workspace_bytes / sizeof(double)), rows_device);
    return ln_check_launch("ln_batch_norm_backward");
}

static int ln_cloud_row_starts_run(const char* who, const LnTable* t, int rows_upper, int clouds, int max_clouds, int* row_starts, int* order_flag, void* stream) {
    LN_REQUIRE(t && t->keys && t->nr_filled && t->pos_dim >= 1 && t->pos_dim <= LN_MAX_POS_DIM, LN_ERR_ARG, "%s: null table", who);
    LN_REQUIRE((t->batch_points > 0 || t->batch_points == LN_BATCH_POINT_STARTS) && t->batch_key_step >= 2, LN_ERR_ARG,
               "%s: the table holds no batch of clouds", who);
    LN_REQUIRE(clouds >= 1 && clouds <= max_clouds, LN_ERR_UNSUPPORTED, "%s: 1 <= clouds <= %d (got %d)", who, max_clouds, clouds);
    LN_REQUIRE(rows_upper >= 0 && row_starts && order_flag, LN_ERR_ARG, "%s: null output or negative rows_upper", who);
    hipStream_t st = (hipStream_t)stream;
    if (ln_zero_async(order_flag, sizeof(int), st) != LN_OK) return ln_check_launch(who);
    LN_LAUNCH("k_cloud_row_starts", k_cloud_row_starts, dim3(ln_div_up((long long)rows_upper + 1, 256)), dim3(256), 0, st, *t, rows_upper, clouds,
              row_starts, order_flag);
    return ln_check_launch(who);
}

// (k_cloud_row_starts writes any number of starts: the two entry points differ in the limit they check)
extern "C" int ln_cloud_row_starts(const LnTable* t, int rows_upper, int clouds, int* row_starts, int* order_flag, void* stream) {
    return ln_cloud_row_starts_run("ln_cloud_row_starts", t, rows_upper, clouds, LN_CLOUDS_MAX, row_starts, order_flag, stream);
}

extern "C" int ln_cloud_row_starts_many(const LnTable* t, int rows_upper, int clouds, int* row_starts, int* order_flag, void* stream) {
    return ln_cloud_row_starts_run("ln_cloud_row_starts_many", t, rows_upper, clouds, LN_CLOUDS_MANY_MAX, row_starts, order_flag, stream);
}

// Up to LN_GN_MAX_SEGMENTS ranges: B accumulator slabs, then the B x 2 C parameter-gradient terms of the backward call.  Beyond (the
// range-owner form): the B x 2 C terms alone, written before they are read, so that nothing in this workspace has to be zero.
extern "C" size_t ln_group_norm_segments_workspace_bytes(int channels, int segments) {
    const size_t parts = 2 * (size_t)channels * sizeof(double);
    if (segments > LN_GN_MAX_SEGMENTS) return (size_t)segments * parts;
    return (size_t)segments * (ln_group_norm_workspace_bytes(channels) + parts);
}

static int ln_gn_segments_check(const char* who, int m, int c, int groups, int segments, int max_segments, const int* row_starts) {
    int rc = ln_gn_check(who, m, c, groups);
    if (rc) return rc;
    LN_REQUIRE(segments >= 1 && segments <= max_segments, LN_ERR_UNSUPPORTED, "%s: 1 <= row ranges <= %d (got %d)", who, max_segments, segments);
    LN_REQUIRE(row_starts, LN_ERR_ARG, "%s: null row_starts", who);
    return LN_OK;
}

// apply grid of one range: sized for twice the mean range (the loops are grid-stride: any range is covered)
static int ln_gn_segments_apply_grid(int m, int c, int segments) { return ln_gn_apply_grid(2 * ln_div_up(m, segments), c); }

// The fp32 and fp16 entry points over row ranges share one host function: `storage` says what x / y (grad_y / grad_x) point at; the
// checks, the grids and the workspace are the same, and the kernel instance is picked at the launch.  (The fp16 entry points come with
// max_segments = LN_GN_MAX_SEGMENTS and are refused before the range-owner branch, which has no fp16 instance.)
static int ln_gn_forward_segments_run(const char* who, int max_segments, LnGnStorage storage, const void* x, const float* gamma, const float* beta, int m,
                                      int channels, int groups, float eps, int relu, void* y, float* mean_rstd, float* scale_shift, void* workspace,
                                      size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, const int* rows_device,
                                      const int* row_starts, int segments, void* stream) {
    int rc = ln_gn_segments_check(who, m, channels, groups, segments, max_segments, row_starts);
    if (rc) return rc;
    rc = ln_norm_check_buffers(who, x, nullptr, y, mean_rstd, scale_shift, workspace, workspace_bytes,
                               ln_group_norm_segments_workspace_bytes(channels, segments), next_workspace, false, storage);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* zero_next = static_cast<double*>(next_workspace);
    const int zero_count = int(next_workspace_bytes / sizeof(double));
    if (segments > LN_GN_MAX_SEGMENTS) {  // many short ranges: one owner per range, `workspace` is not touched
        LN_LAUNCH("k_gn_forward_range_owner", k_gn_forward_range_owner, dim3(1, segments), dim3(256), 0, st, static_cast<const float*>(x), gamma, beta, m,
                  channels, groups, eps, relu, static_cast<float*>(y), mean_rstd, scale_shift, zero_next, zero_count, rows_device, row_starts, segments);
        return ln_check_launch(who);
    }
    double* acc = static_cast<double*>(workspace);
    if (!next_workspace && ln_zero_async(acc, (size_t)segments * ln_group_norm_workspace_bytes(channels), st) != LN_OK)
        return ln_check_launch(who);
    const dim3 stats_grid(ln_gn_stats_grid(m, channels), segments), apply_grid(ln_gn_segments_apply_grid(m, channels, segments), segments);
    if (storage == LN_GN_F16) {
        const _Float16* xh = static_cast<const _Float16*>(x);
        LN_LAUNCH("k_gn_stats_segments_f16", k_gn_stats_segments_f16, stats_grid, dim3(256), 0, st, xh, (const _Float16*)nullptr, (const float*)nullptr,
                  0, m, channels, acc, rows_device, row_starts, segments);
        LN_LAUNCH("k_gn_apply_segments_f16", k_gn_apply_segments_f16, apply_grid, dim3(256), 0, st, xh, (const double*)acc, gamma, beta, m, channels,
                  groups, eps, relu, static_cast<_Float16*>(y), mean_rstd, scale_shift, zero_next, zero_count, rows_device, row_starts, segments);
        return ln_check_launch(who);
    }
    const float* xf = static_cast<const float*>(x);
    LN_LAUNCH("k_gn_stats_segments", k_gn_stats_segments, stats_grid, dim3(256), 0, st, xf, (const float*)nullptr, (const float*)nullptr, 0, m, channels,
              acc, rows_device, row_starts, segments);
    LN_LAUNCH("k_gn_apply_segments", k_gn_apply_segments, apply_grid, dim3(256), 0, st, xf, (const double*)acc, gamma, beta, m, channels, groups, eps,
              relu, static_cast<float*>(y), mean_rstd, scale_shift, zero_next, zero_count, rows_device, row_starts, segments);
    return ln_check_launch(who);
}

// The entry points over row ranges.  ln_group_norm_forward_segments / _backward_segments take up to LN_GN_MAX_SEGMENTS ranges, as they always
// did; ln_group_norm_forward_many_segments / _backward_many_segments take up to LN_GN_MANY_MAX_SEGMENTS and, beyond LN_GN_MAX_SEGMENTS, the
// range-owner kernels (up to there they are the first pair, launch for launch).
extern "C" int ln_group_norm_forward_segments(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                              int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                              void* next_workspace, size_t next_workspace_bytes, const int* rows_device, const int* row_starts,
                                              int segments, void* stream) {
    return ln_gn_forward_segments_run("ln_group_norm_forward_segments", LN_GN_MAX_SEGMENTS, LN_GN_F32, x, gamma, beta, m, channels, groups, eps, relu, y, mean_rstd, scale_shift, workspace,
                                      workspace_bytes, next_workspace, next_workspace_bytes, rows_device, row_starts, segments, stream);
}

extern "C" int ln_group_norm_forward_many_segments(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                                   int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace,
                                                   size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes,
                                                   const int* rows_device, const int* row_starts, int segments, void* stream) {
    return ln_gn_forward_segments_run("ln_group_norm_forward_many_segments", LN_GN_MANY_MAX_SEGMENTS, LN_GN_F32, x, gamma, beta, m, channels, groups, eps, relu, y, mean_rstd, scale_shift, workspace,
                                      workspace_bytes, next_workspace, next_workspace_bytes, rows_device, row_starts, segments, stream);
}

extern "C" int ln_group_norm_forward_segments_f16(const void* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                                  int relu, void* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                                  void* next_workspace, size_t next_workspace_bytes, const int* rows_device, const int* row_starts,
                                                  int segments, void* stream) {
    return ln_gn_forward_segments_run("ln_group_norm_forward_segments_f16", LN_GN_MAX_SEGMENTS, LN_GN_F16, x, gamma, beta, m, channels, groups, eps, relu,
                                      y, mean_rstd, scale_shift, workspace, workspace_bytes, next_workspace, next_workspace_bytes, rows_device,
                                      row_starts, segments, stream);
}

static int ln_gn_backward_segments_run(const char* who, int max_segments, LnGnStorage storage, const void* x, const void* grad_y, const float* gamma,
                                       const float* mean_rstd, const float* scale_shift, int m, int channels, int groups, int relu, void* grad_x, float* grad_gamma,
                                       float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace,
                                       size_t next_workspace_bytes, const int* rows_device, const int* row_starts, int segments, void* stream) {
    int rc = ln_gn_segments_check(who, m, channels, groups, segments, max_segments, row_starts);
    if (rc) return rc;
    rc = ln_norm_check_buffers(who, x, grad_y, grad_x, mean_rstd, scale_shift, workspace, workspace_bytes,
                               ln_group_norm_segments_workspace_bytes(channels, segments), next_workspace, true, storage);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* acc = static_cast<double*>(workspace);
    double* zero_next = static_cast<double*>(next_workspace);
    const int zero_count = int(next_workspace_bytes / sizeof(double));
    if (segments > LN_GN_MAX_SEGMENTS) {  // many short ranges: one owner per range, the workspace is the B x 2 C terms
        LN_LAUNCH("k_gn_backward_range_owner", k_gn_backward_range_owner, dim3(1, segments), dim3(256), 0, st, static_cast<const float*>(x),
                  static_cast<const float*>(grad_y), gamma, mean_rstd, scale_shift, m, channels, groups, relu, static_cast<float*>(grad_x), acc, zero_next,
                  zero_count, rows_device, row_starts, segments);
        if (grad_gamma || grad_beta)
            LN_LAUNCH("k_gn_param_grads_segments", k_gn_param_grads_segments, dim3(ln_div_up(2 * channels, 256)), dim3(256), 0, st,
                      (const double*)acc, segments, channels, grad_gamma, grad_beta);
        return ln_check_launch(who);
    }
    const size_t slabs = (size_t)segments * ln_group_norm_workspace_bytes(channels);
    double* parts = acc + slabs / sizeof(double);
    if (!next_workspace && ln_zero_async(acc, slabs, st) != LN_OK) return ln_check_launch(who);
    const dim3 stats_grid(ln_gn_stats_grid(m, channels), segments), apply_grid(ln_gn_segments_apply_grid(m, channels, segments), segments);
    if (storage == LN_GN_F16) {
        const _Float16 *xh = static_cast<const _Float16*>(x), *gh = static_cast<const _Float16*>(grad_y);
        LN_LAUNCH("k_gn_stats_segments_f16", k_gn_stats_segments_f16, stats_grid, dim3(256), 0, st, xh, gh, scale_shift, relu, m, channels, acc,
                  rows_device, row_starts, segments);
        LN_LAUNCH("k_gn_backward_apply_segments_f16", k_gn_backward_apply_segments_f16, apply_grid, dim3(256), 0, st, xh, gh, (const double*)acc, gamma,
                  mean_rstd, scale_shift, m, channels, groups, relu, static_cast<_Float16*>(grad_x), parts, zero_next, zero_count, rows_device,
                  row_starts, segments);
    } else {
        const float *xf = static_cast<const float*>(x), *gf = static_cast<const float*>(grad_y);
        LN_LAUNCH("k_gn_stats_segments", k_gn_stats_segments, stats_grid, dim3(256), 0, st, xf, gf, scale_shift, relu, m, channels, acc, rows_device,
                  row_starts, segments);
        LN_LAUNCH("k_gn_backward_apply_segments", k_gn_backward_apply_segments, apply_grid, dim3(256), 0, st, xf, gf, (const double*)acc, gamma,
                  mean_rstd, scale_shift, m, channels, groups, relu, static_cast<float*>(grad_x), parts, zero_next, zero_count, rows_device, row_starts,
                  segments);
    }
    if (grad_gamma || grad_beta)
        LN_LAUNCH("k_gn_param_grads_segments", k_gn_param_grads_segments, dim3(ln_div_up(2 * channels, 256)), dim3(256), 0, st, (const double*)parts,
                  segments, channels, grad_gamma, grad_beta);
    return ln_check_launch(who);
}

extern "C" int ln_group_norm_backward_segments(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                               const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                               float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace,
                                               size_t next_workspace_bytes, const int* rows_device, const int* row_starts, int segments, void* stream) {
    return ln_gn_backward_segments_run("ln_group_norm_backward_segments", LN_GN_MAX_SEGMENTS, LN_GN_F32, x, grad_y, gamma, mean_rstd, scale_shift, m, channels, groups, relu, grad_x, grad_gamma,
                                       grad_beta, workspace, workspace_bytes, next_workspace, next_workspace_bytes, rows_device, row_starts, segments,
                                       stream);
}

extern "C" int ln_group_norm_backward_many_segments(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                                    const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x,
                                                    float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes,
                                                    void* next_workspace, size_t next_workspace_bytes, const int* rows_device,
                                                    const int* row_starts, int segments, void* stream) {
    return ln_gn_backward_segments_run("ln_group_norm_backward_many_segments", LN_GN_MANY_MAX_SEGMENTS, LN_GN_F32, x, grad_y, gamma, mean_rstd, scale_shift, m, channels, groups, relu, grad_x,
                                       grad_gamma, grad_beta, workspace, workspace_bytes, next_workspace, next_workspace_bytes, rows_device,
                                       row_starts, segments, stream);
}

extern "C" int ln_group_norm_backward_segments_f16(const void* x, const void* grad_y, const float* gamma, const float* mean_rstd,
                                                   const float* scale_shift, int m, int channels, int groups, int relu, void* grad_x,
                                                   float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes,
                                                   void* next_workspace, size_t next_workspace_bytes, const int* rows_device,
                                                   const int* row_starts, int segments, void* stream) {
    return ln_gn_backward_segments_run("ln_group_norm_backward_segments_f16", LN_GN_MAX_SEGMENTS, LN_GN_F16, x, grad_y, gamma, mean_rstd, scale_shift, m,
                                       channels, groups, relu, grad_x, grad_gamma, grad_beta, workspace, workspace_bytes, next_workspace,
                                       next_workspace_bytes, rows_device, row_starts, segments, stream);
}
