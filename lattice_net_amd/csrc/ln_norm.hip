// GroupNorm (+ fused ReLU) on the native [M, C] lattice-value layout, forward and backward.
// The reference runs torch.nn.GroupNorm on a transposed [1, C, M] view (lattice_modules.py:585-616), which on a
// row-major value matrix costs two transposed copies in each direction; the LNN blocks (GnRelu1x1, GnReluConv,
// GnReluFinefy, ...) apply it before every operator, so it sits between any two lattice kernels of the U-Net.
//   statistics : per-channel partial sums over a slab of rows per workgroup (lanes run along the channels of a row:
//                coalesced), combined across workgroups with one fp64 atomic per (workgroup, channel)
//   apply      : every workgroup rebuilds the per-channel scale/shift from the C channel sums in LDS, then one
//                float4 pass over its slab
// Backward uses the same two shapes: per-channel sums of gy*x and gy, then dx = gy*gamma*rstd + x*c2[g] + c3[g].
// Every fp32 sum that involves x is a sum of x - p over the LN_GN_PASSES rows of ONE thread, with the pivot p the first of these
// rows: sum (x-p)^2 and sum gy*(x-p) have the size of the spread of those rows, not of their offset from zero, and a pivot that is an
// outlier spoils 16 rows' worth of a sum it is itself a term of, never the whole statistic.  Each thread then puts its pivot back in
// fp64 (sum x = S1 + n p, sum x^2 = S2 + 2 p S1 + n p^2, sum gy x = S + p sum gy): everything from there on, the fold of the
// workgroup, the atomics and E[x^2] - mean^2, is fp64, where the cancellation costs 2^-53, not 2^-24.
#include "ln_common.h"

#define LN_GN_MAX_C 1024
#define LN_GN_PASSES 16
#define LN_GN_REPLICAS 32  // accumulator copies: memory-side atomics serialise per cache line, so spread the workgroups
#define LN_GN_MAX_SEGMENTS 64  // row ranges of one call (the clouds of a batch: Lattice.set_cloud_batch)

// acc[c*2 + 0] += sum_rows p(row, c), acc[c*2 + 1] += sum_rows q(row, c)
//   forward  (gy == nullptr): p = x,  q = x*x
//   backward               : p = gy' * x, q = gy'   with gy' = gy masked by (x*a[c] + b[c] > 0) when relu
// A thread owns one float4 (4 channels) of a row; 256 / (c/4) rows are read per pass and LN_GN_PASSES independent
// passes are in flight per thread.  The rows are [row_begin, m); workgroup `block` takes the slab of rows_per_pass * LN_GN_PASSES rows
// that starts that many * block rows behind row_begin (k_gn_stats: the whole matrix; k_gn_stats_segments: one row range of it).
__device__ __forceinline__ void ln_gn_stats_rows(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ scale_shift,
                                                 int relu, int row_begin, int m, int c, double* __restrict__ acc, int block) {
    __shared__ double s_p[256][4], s_q[256][4];
    const int tid = threadIdx.x;
    const int quads = c >> 2;                 // c % 4 == 0, c <= 1024  ->  quads <= 256
    const int rows_per_pass = 256 / quads;
    const int rp = tid / quads;
    const int qi = tid - rp * quads;
    const bool live = rp < rows_per_pass;
    const long long r0 = row_begin + (long long)block * rows_per_pass * LN_GN_PASSES;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), q = p;
    double pd[4] = {0.0, 0.0, 0.0, 0.0}, qd[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
        float4 a = p, b = p;
        // pivots: this thread's first row (with no row of its own all its terms are zero)
        const float4 pv = r0 + rp < m ? reinterpret_cast<const float4*>(x + (r0 + rp) * c)[qi] : p;
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
            xv[k] = ok ? reinterpret_cast<const float4*>(x + row * c)[qi] : pv;  // (x - p = 0 beyond the last row)
            if (gy) gv[k] = ok ? reinterpret_cast<const float4*>(gy + row * c)[qi] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < LN_GN_PASSES; ++k) {
            if (gy) {
                float4 g = gv[k];
                if (relu) {
                    if (!(xv[k].x * a.x + b.x > 0.f)) g.x = 0.f;
                    if (!(xv[k].y * a.y + b.y > 0.f)) g.y = 0.f;
                    if (!(xv[k].z * a.z + b.z > 0.f)) g.z = 0.f;
                    if (!(xv[k].w * a.w + b.w > 0.f)) g.w = 0.f;
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

__global__ void __launch_bounds__(256)
    k_gn_stats(const float* __restrict__ x, const float* __restrict__ gy, const float* __restrict__ scale_shift, int relu, int m, int c,
               double* __restrict__ acc, const int* __restrict__ rows_dev) {
    if (rows_dev) m = min(m, *rows_dev);  // static-rows mode: the tensors are taller than the lattice, only its rows count
    ln_gn_stats_rows(x, gy, scale_shift, relu, 0, m, c, acc, blockIdx.x);
}

// per-channel scale a[c] = gamma*rstd[g], shift b[c] = beta - mean[g]*a[c] from the channel sums; block 0 also
// publishes mean/rstd per group and scale/shift per channel for the backward pass
__device__ __forceinline__ void ln_gn_channel_affine(const double* __restrict__ acc, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int m, int c, int groups, float eps, float* s_a,
                                                     float* s_b, float* __restrict__ mean_rstd, float* __restrict__ scale_shift) {
    if (m < 1) m = 1;  // (an empty lattice under a static row bound: all sums are zero)
    const int cg = c / groups;
    __shared__ double s_sum[LN_GN_MAX_C], s_sq[LN_GN_MAX_C];
    for (int col = threadIdx.x; col < c; col += 256) {  // channel sums over the accumulator replicas
        double v0[LN_GN_REPLICAS], v1[LN_GN_REPLICAS];
#pragma unroll
        for (int r = 0; r < LN_GN_REPLICAS; ++r) {
            v0[r] = acc[(size_t)r * 2 * c + 2 * col];
            v1[r] = acc[(size_t)r * 2 * c + 2 * col + 1];
        }
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int r = 0; r < LN_GN_REPLICAS; ++r) {
            a0 += v0[r];
            a1 += v1[r];
        }
        s_sum[col] = a0;
        s_sq[col] = a1;
    }
    __syncthreads();
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

__global__ void __launch_bounds__(256)
    k_gn_apply(const float* __restrict__ x, const double* __restrict__ acc, const float* __restrict__ gamma, const float* __restrict__ beta,
               int m, int c, int groups, float eps, int relu, float* __restrict__ y, float* __restrict__ mean_rstd,
               float* __restrict__ scale_shift, double* __restrict__ zero_next, int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int m_tensor = m;
    if (rows_dev) m = min(m, *rows_dev);  // rows beyond the lattice: excluded from the statistics, written as zeros
    if (zero_next && blockIdx.x == 0)  // the accumulators of the NEXT call (nobody is using them now: stream order)
        for (int i = threadIdx.x; i < zero_count; i += 256) zero_next[i] = 0.0;
    ln_gn_channel_affine(acc, gamma, beta, m, c, groups, eps, s_a, s_b, mean_rstd, scale_shift);
    __syncthreads();
    const long long total4 = (long long)m * c / 4;  // c % 4 == 0 checked by the host
    const long long tensor4 = (long long)m_tensor * c / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = total4 + (long long)blockIdx.x * 256 + threadIdx.x; i < tensor4; i += stride)
        reinterpret_cast<float4*>(y)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
        const int col = int((i * 4) % c);
        float4 v = reinterpret_cast<const float4*>(x)[i];
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
        reinterpret_cast<float4*>(y)[i] = v;
    }
}

// dx = gy' * gamma * rstd + x * c2[g] + c3[g];   block 0 writes dgamma = (ds - db*mean)*rstd, dbeta = db   (all of it in fp64)
__global__ void __launch_bounds__(256)
    k_gn_backward_apply(const float* __restrict__ x, const float* __restrict__ gy, const double* __restrict__ acc,
                        const float* __restrict__ gamma, const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift, int m,
                        int c, int groups, int relu, float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                        double* __restrict__ zero_next, int zero_count, const int* __restrict__ rows_dev) {
    const int m_tensor = m;
    if (rows_dev) m = min(m, *rows_dev);
    if (m < 1) m = 1;
    if (zero_next && blockIdx.x == 0)
        for (int i = threadIdx.x; i < zero_count; i += 256) zero_next[i] = 0.0;
    __shared__ float s_gr[LN_GN_MAX_C], s_c2[LN_GN_MAX_C], s_c3[LN_GN_MAX_C], s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int cg = c / groups;
    __shared__ double s_ds[LN_GN_MAX_C], s_db[LN_GN_MAX_C];
    for (int col = threadIdx.x; col < c; col += 256) {  // channel sums over the accumulator replicas
        double v0[LN_GN_REPLICAS], v1[LN_GN_REPLICAS];
#pragma unroll
        for (int r = 0; r < LN_GN_REPLICAS; ++r) {
            v0[r] = acc[(size_t)r * 2 * c + 2 * col];
            v1[r] = acc[(size_t)r * 2 * c + 2 * col + 1];
        }
        double ds = 0.0, db = 0.0;
#pragma unroll
        for (int r = 0; r < LN_GN_REPLICAS; ++r) {
            ds += v0[r];
            db += v1[r];
        }
        s_ds[col] = ds;
        s_db[col] = db;
    }
    __syncthreads();
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
        const double cnt = (double)m * cg;
        const double c2 = (sum2 * mean - sum1) * (double)rstd * rstd * rstd / cnt;
        const double c3 = -c2 * mean - sum2 * (double)rstd / cnt;
        s_gr[col] = (gamma ? gamma[col] : 1.f) * rstd;
        s_c2[col] = (float)c2;
        s_c3[col] = (float)c3;
        s_a[col] = scale_shift[col];
        s_b[col] = scale_shift[c + col];
        if (blockIdx.x == 0) {
            if (dgamma) dgamma[col] = (float)((s_ds[col] - s_db[col] * mean) * rstd);
            if (dbeta) dbeta[col] = (float)s_db[col];
        }
    }
    __syncthreads();
    const long long total4 = (rows_dev ? (long long)min(m_tensor, *rows_dev) : (long long)m) * c / 4;
    const long long tensor4 = (long long)m_tensor * c / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = total4 + (long long)blockIdx.x * 256 + threadIdx.x; i < tensor4; i += stride)
        reinterpret_cast<float4*>(dx)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
        const int col = int((i * 4) % c);
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        float4 g = reinterpret_cast<const float4*>(gy)[i];
        if (relu) {
            if (!(xv.x * s_a[col] + s_b[col] > 0.f)) g.x = 0.f;
            if (!(xv.y * s_a[col + 1] + s_b[col + 1] > 0.f)) g.y = 0.f;
            if (!(xv.z * s_a[col + 2] + s_b[col + 2] > 0.f)) g.z = 0.f;
            if (!(xv.w * s_a[col + 3] + s_b[col + 3] > 0.f)) g.w = 0.f;
        }
        float4 o;
        o.x = g.x * s_gr[col] + xv.x * s_c2[col] + s_c3[col];
        o.y = g.y * s_gr[col + 1] + xv.y * s_c2[col + 1] + s_c3[col + 1];
        o.z = g.z * s_gr[col + 2] + xv.z * s_c2[col + 2] + s_c3[col + 2];
        o.w = g.w * s_gr[col + 3] + xv.w * s_c2[col + 3] + s_c3[col + 3];
        reinterpret_cast<float4*>(dx)[i] = o;
    }
}

static int ln_gn_check(const char* who, int m, int c, int groups) {
    LN_REQUIRE(m >= 1 && c >= 4 && c <= LN_GN_MAX_C && c % 4 == 0, LN_ERR_UNSUPPORTED, "%s: need 1 <= rows, channels %% 4 == 0 and <= %d (got %d x %d)",
               who, LN_GN_MAX_C, m, c);
    LN_REQUIRE(groups >= 1 && c % groups == 0, LN_ERR_ARG, "%s: %d groups do not divide %d channels", who, groups, c);
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
                                          void* next_workspace, size_t next_workspace_bytes, const int* rows_device, void* stream);
extern "C" int ln_group_norm_forward(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                     int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                     void* next_workspace, size_t next_workspace_bytes, void* stream) {
    return ln_group_norm_forward_rows(x, gamma, beta, m, channels, groups, eps, relu, y, mean_rstd, scale_shift, workspace, workspace_bytes,
                                      next_workspace, next_workspace_bytes, nullptr, stream);
}
extern "C" int ln_group_norm_forward_rows(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                          int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                          void* next_workspace, size_t next_workspace_bytes, const int* rows_device, void* stream) {
    int rc = ln_gn_check("ln_group_norm_forward", m, channels, groups);
    if (rc) return rc;
    LN_REQUIRE(x && y && mean_rstd && scale_shift && workspace && workspace_bytes >= ln_group_norm_workspace_bytes(channels), LN_ERR_ARG,
               "ln_group_norm_forward: null buffer or workspace too small");
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               LN_ERR_ARG, "ln_group_norm_forward: x / y must be 16-byte aligned");
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

extern "C" int ln_group_norm_backward_rows(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                           const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                           float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace,
                                           size_t next_workspace_bytes, const int* rows_device, void* stream);
extern "C" int ln_group_norm_backward(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                      const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                      float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace, size_t next_workspace_bytes, void* stream) {
    return ln_group_norm_backward_rows(x, grad_y, gamma, mean_rstd, scale_shift, m, channels, groups, relu, grad_x, grad_gamma, grad_beta, workspace,
                                       workspace_bytes, next_workspace, next_workspace_bytes, nullptr, stream);
}
extern "C" int ln_group_norm_backward_rows(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                           const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                           float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace,
                                           size_t next_workspace_bytes, const int* rows_device, void* stream) {
    int rc = ln_gn_check("ln_group_norm_backward", m, channels, groups);
    if (rc) return rc;
    LN_REQUIRE(x && grad_y && mean_rstd && scale_shift && grad_x && workspace && workspace_bytes >= ln_group_norm_workspace_bytes(channels),
               LN_ERR_ARG, "ln_group_norm_backward: null buffer or workspace too small");
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(grad_y) | reinterpret_cast<uintptr_t>(grad_x)) & 15) == 0, LN_ERR_ARG,
               "ln_group_norm_backward: x / grad_y / grad_x must be 16-byte aligned");
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

// ---- BatchNorm (+ fused ReLU) over the same [M, C] layout: GroupNorm with one channel per group, plus running statistics ----------
// Training: k_gn_stats gives the fp64 channel sums exactly as for GroupNorm (same summation, same bounds), k_bn_apply turns them into
// scale / shift and moves the running statistics on the device; the backward is k_gn_backward_apply at groups == channels.
// Evaluation: the statistics are the running ones, constants of the step: one launch forward; backward dx = gy' * a, and the
// parameter gradients from the same k_gn_stats sums.

// the two fp64 sums of channel `col` over the accumulator replicas, added in replica order (the order of ln_gn_channel_affine), eight
// loads in flight at a time
__device__ __forceinline__ void ln_bn_channel_sums(const double* __restrict__ acc, int c, int col, double& s0, double& s1) {
    s0 = 0.0;
    s1 = 0.0;
    for (int r0 = 0; r0 < LN_GN_REPLICAS; r0 += 8) {
        double v0[8], v1[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            v0[r] = acc[(size_t)(r0 + r) * 2 * c + 2 * col];
            v1[r] = acc[(size_t)(r0 + r) * 2 * c + 2 * col + 1];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            s0 += v0[r];
            s1 += v1[r];
        }
    }
}

// y = act(x * a[c] + b[c]) over the first m rows, zeros in the rows from m to m_tensor
__device__ __forceinline__ void ln_bn_apply_rows(const float* __restrict__ x, const float* s_a, const float* s_b, int m, int m_tensor, int c,
                                                 int relu, float* __restrict__ y) {
    const long long total4 = (long long)m * c / 4;  // c % 4 == 0 checked by the host
    const long long tensor4 = (long long)m_tensor * c / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = total4 + (long long)blockIdx.x * 256 + threadIdx.x; i < tensor4; i += stride)
        reinterpret_cast<float4*>(y)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
        const int col = int((i * 4) % c);
        float4 v = reinterpret_cast<const float4*>(x)[i];
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
        reinterpret_cast<float4*>(y)[i] = v;
    }
}

// Training forward.  Every workgroup rebuilds a = gamma * rstd, b = beta - mean * a from the fp64 channel sums (biased variance, clamped
// at 0; n = live rows); block 0 publishes mean_rstd / scale_shift and, with n >= 2, moves the running statistics (unbiased variance),
// each formed in fp64 and rounded once.  With n < 2 the running statistics keep their bits.
__global__ void __launch_bounds__(256)
    k_bn_apply(const float* __restrict__ x, const double* __restrict__ acc, const float* __restrict__ gamma, const float* __restrict__ beta,
               float* __restrict__ running_mean, float* __restrict__ running_var, int m, int c, float eps, double momentum, int relu,
               float* __restrict__ y, float* __restrict__ mean_rstd, float* __restrict__ scale_shift, double* __restrict__ zero_next,
               int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int m_tensor = m;
    if (rows_dev) m = max(0, min(m, *rows_dev));  // rows beyond the lattice: excluded from the statistics, written as zeros
    if (zero_next && blockIdx.x == 0)  // the accumulators of the NEXT call (nobody is using them now: stream order)
        for (int i = threadIdx.x; i < zero_count; i += 256) zero_next[i] = 0.0;
    const double cnt = m < 1 ? 1.0 : (double)m;  // (an empty lattice under a static row bound: all sums are zero)
    for (int col = threadIdx.x; col < c; col += 256) {
        double s, ss;
        ln_bn_channel_sums(acc, c, col, s, ss);
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
            if (running_mean && m >= 2) {  // (one row has no unbiased variance: nothing moves)
                running_mean[col] = (float)((1.0 - momentum) * (double)running_mean[col] + momentum * mean);
                running_var[col] = (float)((1.0 - momentum) * (double)running_var[col] + momentum * (var * (cnt / (cnt - 1.0))));
            }
        }
    }
    __syncthreads();
    ln_bn_apply_rows(x, s_a, s_b, m, m_tensor, c, relu, y);
}

// Evaluation forward: a = gamma / sqrt(running_var + eps) (rstd formed in fp64, rounded once), b = beta - running_mean * a (fp64, rounded
// once).  Reads the running statistics, never writes them.
__global__ void __launch_bounds__(256)
    k_bn_apply_eval(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                    const float* __restrict__ running_mean, const float* __restrict__ running_var, int m, int c, float eps, int relu,
                    float* __restrict__ y, float* __restrict__ mean_rstd, float* __restrict__ scale_shift, double* __restrict__ zero_next,
                    int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int m_tensor = m;
    if (rows_dev) m = max(0, min(m, *rows_dev));
    if (zero_next && blockIdx.x == 0)
        for (int i = threadIdx.x; i < zero_count; i += 256) zero_next[i] = 0.0;
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
    ln_bn_apply_rows(x, s_a, s_b, m, m_tensor, c, relu, y);
}

// Evaluation backward: dx = gy' * a;  block 0 writes dgamma = (ds - db * running_mean) * rstd, dbeta = db in fp64 from the k_gn_stats
// sums (acc == nullptr: no parameter gradient is wanted and no sums were taken).
__global__ void __launch_bounds__(256)
    k_bn_backward_eval(const float* __restrict__ x, const float* __restrict__ gy, const double* __restrict__ acc,
                       const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift, int m, int c, int relu,
                       float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta, double* __restrict__ zero_next,
                       int zero_count, const int* __restrict__ rows_dev) {
    __shared__ float s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int m_tensor = m;
    if (rows_dev) m = max(0, min(m, *rows_dev));
    if (zero_next && blockIdx.x == 0)
        for (int i = threadIdx.x; i < zero_count; i += 256) zero_next[i] = 0.0;
    for (int col = threadIdx.x; col < c; col += 256) {
        s_a[col] = scale_shift[col];
        s_b[col] = scale_shift[c + col];
        if (acc && blockIdx.x == 0) {
            double ds, db;
            ln_bn_channel_sums(acc, c, col, ds, db);
            if (dgamma) dgamma[col] = (float)((ds - db * (double)mean_rstd[col]) * (double)mean_rstd[c + col]);
            if (dbeta) dbeta[col] = (float)db;
        }
    }
    __syncthreads();
    const long long total4 = (long long)m * c / 4;
    const long long tensor4 = (long long)m_tensor * c / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = total4 + (long long)blockIdx.x * 256 + threadIdx.x; i < tensor4; i += stride)
        reinterpret_cast<float4*>(dx)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += stride) {
        const int col = int((i * 4) % c);
        float4 g = reinterpret_cast<const float4*>(gy)[i];
        if (relu) {
            const float4 xv = reinterpret_cast<const float4*>(x)[i];
            if (!(xv.x * s_a[col] + s_b[col] > 0.f)) g.x = 0.f;
            if (!(xv.y * s_a[col + 1] + s_b[col + 1] > 0.f)) g.y = 0.f;
            if (!(xv.z * s_a[col + 2] + s_b[col + 2] > 0.f)) g.z = 0.f;
            if (!(xv.w * s_a[col + 3] + s_b[col + 3] > 0.f)) g.w = 0.f;
        }
        reinterpret_cast<float4*>(dx)[i] = make_float4(g.x * s_a[col], g.y * s_a[col + 1], g.z * s_a[col + 2], g.w * s_a[col + 3]);
    }
}

extern "C" size_t ln_batch_norm_workspace_bytes(int channels) { return ln_group_norm_workspace_bytes(channels); }

extern "C" int ln_batch_norm_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, int m,
                                     int channels, float eps, double momentum, int training, int relu, float* y, float* mean_rstd,
                                     float* scale_shift, void* workspace, size_t workspace_bytes, void* next_workspace,
                                     size_t next_workspace_bytes, const int* rows_device, void* stream) {
    int rc = ln_gn_check("ln_batch_norm_forward", m, channels, channels);
    if (rc) return rc;
    LN_REQUIRE(x && y && mean_rstd && scale_shift, LN_ERR_ARG, "ln_batch_norm_forward: null buffer");
    LN_REQUIRE(!running_mean == !running_var, LN_ERR_ARG, "ln_batch_norm_forward: running_mean and running_var come together or not at all");
    LN_REQUIRE(training || running_mean, LN_ERR_ARG, "ln_batch_norm_forward: evaluation mode needs the running statistics");
    LN_REQUIRE(!training || (workspace && workspace_bytes >= ln_batch_norm_workspace_bytes(channels)), LN_ERR_ARG,
               "ln_batch_norm_forward: null or too small workspace");
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(next_workspace) & 7) == 0,
               LN_ERR_ARG, "ln_batch_norm_forward: x / y must be 16-byte aligned");
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
    LN_REQUIRE(x && grad_y && mean_rstd && scale_shift && grad_x && workspace && workspace_bytes >= ln_batch_norm_workspace_bytes(channels),
               LN_ERR_ARG, "ln_batch_norm_backward: null buffer or workspace too small");
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(grad_y) | reinterpret_cast<uintptr_t>(grad_x)) & 15) == 0 &&
                   ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(next_workspace)) & 7) == 0,
               LN_ERR_ARG, "ln_batch_norm_backward: x / grad_y / grad_x must be 16-byte aligned");
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

extern "C" int ln_cloud_row_starts(const LnTable* t, int rows_upper, int clouds, int* row_starts, int* order_flag, void* stream) {
    LN_REQUIRE(t && t->keys && t->nr_filled && t->pos_dim >= 1 && t->pos_dim <= LN_MAX_POS_DIM, LN_ERR_ARG, "ln_cloud_row_starts: null table");
    LN_REQUIRE((t->batch_points > 0 || t->batch_points == LN_BATCH_POINT_STARTS) && t->batch_key_step >= 2, LN_ERR_ARG,
               "ln_cloud_row_starts: the table holds no batch of clouds");
    LN_REQUIRE(clouds >= 1 && clouds <= LN_GN_MAX_SEGMENTS, LN_ERR_UNSUPPORTED, "ln_cloud_row_starts: 1 <= clouds <= %d (got %d)",
               LN_GN_MAX_SEGMENTS, clouds);
    LN_REQUIRE(rows_upper >= 0 && row_starts && order_flag, LN_ERR_ARG, "ln_cloud_row_starts: null output or negative rows_upper");
    hipStream_t st = (hipStream_t)stream;
    if (ln_zero_async(order_flag, sizeof(int), st) != LN_OK) return ln_check_launch("ln_cloud_row_starts(memset)");
    LN_LAUNCH("k_cloud_row_starts", k_cloud_row_starts, dim3(ln_div_up((long long)rows_upper + 1, 256)), dim3(256), 0, st, *t, rows_upper, clouds,
              row_starts, order_flag);
    return ln_check_launch("ln_cloud_row_starts");
}

// rows [lo, hi) of range s, clamped to 0 <= lo <= hi <= live whatever row_starts holds (nothing is indexed outside the tensors); live = the rows that count
__device__ __forceinline__ void ln_gn_segment(const int* __restrict__ row_starts, int segments, int s, int m, const int* __restrict__ rows_dev,
                                              int& live, int& lo, int& hi) {
    live = min(m, row_starts[segments]);
    if (rows_dev) live = min(live, *rows_dev);
    live = max(live, 0);
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

// the accumulators of the NEXT call, one share per range (the first workgroup of every range), and zeros in the rows behind the last range
__device__ __forceinline__ void ln_gn_segments_housekeeping(double* __restrict__ zero_next, int zero_count, int segments, int live, int m, int c,
                                                            float* __restrict__ out) {
    if (zero_next && blockIdx.x == 0) {
        const int share = (zero_count + segments - 1) / segments;
        const int end = min(zero_count, ((int)blockIdx.y + 1) * share);
        for (int i = (int)blockIdx.y * share + threadIdx.x; i < end; i += 256) zero_next[i] = 0.0;
    }
    const long long total4 = (long long)live * c / 4, tensor4 = (long long)m * c / 4;
    const long long stride = (long long)gridDim.x * gridDim.y * 256;
    for (long long i = total4 + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < tensor4; i += stride)
        reinterpret_cast<float4*>(out)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
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
    ln_gn_segments_housekeeping(zero_next, zero_count, segments, live, m, c, y);
    if (hi == lo) return;  // an empty range: no statistics, no rows
    ln_gn_channel_affine(acc + (size_t)s * LN_GN_REPLICAS * 2 * c, gamma, beta, hi - lo, c, groups, eps, s_a, s_b, mean_rstd + (size_t)s * 2 * groups,
                         scale_shift + (size_t)s * 2 * c);
    __syncthreads();
    const long long last4 = (long long)hi * c / 4;  // c % 4 == 0 checked by the host
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)lo * c / 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < last4; i += stride) {
        const int col = int((i * 4) % c);
        float4 v = reinterpret_cast<const float4*>(x)[i];
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
        reinterpret_cast<float4*>(y)[i] = v;
    }
}

// k_gn_backward_apply over range blockIdx.y.  The parameter gradients are sums over the ranges: the first workgroup of range s leaves its
// terms, (ds - db mean_s) rstd_s and db in fp64, in parts[s * 2 C ...] (zeros for an empty range); k_gn_param_grads_segments adds them.
__global__ void __launch_bounds__(256)
    k_gn_backward_apply_segments(const float* __restrict__ x, const float* __restrict__ gy, const double* __restrict__ acc,
                                 const float* __restrict__ gamma, const float* __restrict__ mean_rstd, const float* __restrict__ scale_shift, int m,
                                 int c, int groups, int relu, float* __restrict__ dx, double* __restrict__ parts, double* __restrict__ zero_next,
                                 int zero_count, const int* __restrict__ rows_dev, const int* __restrict__ row_starts, int segments) {
    const int s = blockIdx.y;
    int live, lo, hi;
    ln_gn_segment(row_starts, segments, s, m, rows_dev, live, lo, hi);
    ln_gn_segments_housekeeping(zero_next, zero_count, segments, live, m, c, dx);
    parts += (size_t)s * 2 * c;
    if (hi == lo) {
        if (blockIdx.x == 0)
            for (int i = threadIdx.x; i < 2 * c; i += 256) parts[i] = 0.0;
        return;
    }
    acc += (size_t)s * LN_GN_REPLICAS * 2 * c;
    mean_rstd += (size_t)s * 2 * groups;
    scale_shift += (size_t)s * 2 * c;
    __shared__ float s_gr[LN_GN_MAX_C], s_c2[LN_GN_MAX_C], s_c3[LN_GN_MAX_C], s_a[LN_GN_MAX_C], s_b[LN_GN_MAX_C];
    const int cg = c / groups;
    __shared__ double s_ds[LN_GN_MAX_C], s_db[LN_GN_MAX_C];
    for (int col = threadIdx.x; col < c; col += 256) {  // channel sums over the accumulator replicas, in replica order
        double ds, db;
        ln_bn_channel_sums(acc, c, col, ds, db);
        s_ds[col] = ds;
        s_db[col] = db;
    }
    __syncthreads();
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
        const double cnt = (double)(hi - lo) * cg;
        const double c2 = (sum2 * mean - sum1) * (double)rstd * rstd * rstd / cnt;
        const double c3 = -c2 * mean - sum2 * (double)rstd / cnt;
        s_gr[col] = (gamma ? gamma[col] : 1.f) * rstd;
        s_c2[col] = (float)c2;
        s_c3[col] = (float)c3;
        s_a[col] = scale_shift[col];
        s_b[col] = scale_shift[c + col];
        if (blockIdx.x == 0) {
            parts[col] = (s_ds[col] - s_db[col] * mean) * rstd;
            parts[c + col] = s_db[col];
        }
    }
    __syncthreads();
    const long long last4 = (long long)hi * c / 4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)lo * c / 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < last4; i += stride) {
        const int col = int((i * 4) % c);
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        float4 g = reinterpret_cast<const float4*>(gy)[i];
        if (relu) {
            if (!(xv.x * s_a[col] + s_b[col] > 0.f)) g.x = 0.f;
            if (!(xv.y * s_a[col + 1] + s_b[col + 1] > 0.f)) g.y = 0.f;
            if (!(xv.z * s_a[col + 2] + s_b[col + 2] > 0.f)) g.z = 0.f;
            if (!(xv.w * s_a[col + 3] + s_b[col + 3] > 0.f)) g.w = 0.f;
        }
        float4 o;
        o.x = g.x * s_gr[col] + xv.x * s_c2[col] + s_c3[col];
        o.y = g.y * s_gr[col + 1] + xv.y * s_c2[col + 1] + s_c3[col + 1];
        o.z = g.z * s_gr[col + 2] + xv.z * s_c2[col + 2] + s_c3[col + 2];
        o.w = g.w * s_gr[col + 3] + xv.w * s_c2[col + 3] + s_c3[col + 3];
        reinterpret_cast<float4*>(dx)[i] = o;
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

// B accumulator slabs, then the B x 2 C parameter-gradient terms of the backward call
extern "C" size_t ln_group_norm_segments_workspace_bytes(int channels, int segments) {
    return (size_t)segments * (ln_group_norm_workspace_bytes(channels) + 2 * (size_t)channels * sizeof(double));
}

static int ln_gn_segments_check(const char* who, int m, int c, int groups, int segments, const int* row_starts, void* workspace, size_t workspace_bytes,
                                void* next_workspace) {
    int rc = ln_gn_check(who, m, c, groups);
    if (rc) return rc;
    LN_REQUIRE(segments >= 1 && segments <= LN_GN_MAX_SEGMENTS, LN_ERR_UNSUPPORTED, "%s: 1 <= row ranges <= %d (got %d)", who, LN_GN_MAX_SEGMENTS,
               segments);
    LN_REQUIRE(row_starts && workspace && workspace_bytes >= ln_group_norm_segments_workspace_bytes(c, segments), LN_ERR_ARG,
               "%s: null row_starts or workspace too small", who);
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(next_workspace)) & 7) == 0, LN_ERR_ARG,
               "%s: workspaces must be 8-byte aligned", who);
    return LN_OK;
}

// apply grid of one range: sized for twice the mean range (the loops are grid-stride: any range is covered)
static int ln_gn_segments_apply_grid(int m, int c, int segments) { return ln_gn_apply_grid(2 * ln_div_up(m, segments), c); }

extern "C" int ln_group_norm_forward_segments(const float* x, const float* gamma, const float* beta, int m, int channels, int groups, float eps,
                                              int relu, float* y, float* mean_rstd, float* scale_shift, void* workspace, size_t workspace_bytes,
                                              void* next_workspace, size_t next_workspace_bytes, const int* rows_device, const int* row_starts,
                                              int segments, void* stream) {
    int rc = ln_gn_segments_check("ln_group_norm_forward_segments", m, channels, groups, segments, row_starts, workspace, workspace_bytes, next_workspace);
    if (rc) return rc;
    LN_REQUIRE(x && y && mean_rstd && scale_shift, LN_ERR_ARG, "ln_group_norm_forward_segments: null buffer");
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0, LN_ERR_ARG,
               "ln_group_norm_forward_segments: x / y must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* acc = static_cast<double*>(workspace);
    if (!next_workspace && ln_zero_async(acc, (size_t)segments * ln_group_norm_workspace_bytes(channels), st) != LN_OK)
        return ln_check_launch("ln_group_norm_forward_segments(memset)");
    LN_LAUNCH("k_gn_stats_segments", k_gn_stats_segments, dim3(ln_gn_stats_grid(m, channels), segments), dim3(256), 0, st, x, (const float*)nullptr,
              (const float*)nullptr, 0, m, channels, acc, rows_device, row_starts, segments);
    LN_LAUNCH("k_gn_apply_segments", k_gn_apply_segments, dim3(ln_gn_segments_apply_grid(m, channels, segments), segments), dim3(256), 0, st, x,
              (const double*)acc, gamma, beta, m, channels, groups, eps, relu, y, mean_rstd, scale_shift, static_cast<double*>(next_workspace),
              int(next_workspace_bytes / sizeof(double)), rows_device, row_starts, segments);
    return ln_check_launch("ln_group_norm_forward_segments");
}

extern "C" int ln_group_norm_backward_segments(const float* x, const float* grad_y, const float* gamma, const float* mean_rstd,
                                               const float* scale_shift, int m, int channels, int groups, int relu, float* grad_x, float* grad_gamma,
                                               float* grad_beta, void* workspace, size_t workspace_bytes, void* next_workspace,
                                               size_t next_workspace_bytes, const int* rows_device, const int* row_starts, int segments, void* stream) {
    int rc = ln_gn_segments_check("ln_group_norm_backward_segments", m, channels, groups, segments, row_starts, workspace, workspace_bytes, next_workspace);
    if (rc) return rc;
    LN_REQUIRE(x && grad_y && mean_rstd && scale_shift && grad_x, LN_ERR_ARG, "ln_group_norm_backward_segments: null buffer");
    LN_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(grad_y) | reinterpret_cast<uintptr_t>(grad_x)) & 15) == 0, LN_ERR_ARG,
               "ln_group_norm_backward_segments: x / grad_y / grad_x must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* acc = static_cast<double*>(workspace);
    const size_t slabs = (size_t)segments * ln_group_norm_workspace_bytes(channels);
    double* parts = acc + slabs / sizeof(double);
    if (!next_workspace && ln_zero_async(acc, slabs, st) != LN_OK) return ln_check_launch("ln_group_norm_backward_segments(memset)");
    LN_LAUNCH("k_gn_stats_segments", k_gn_stats_segments, dim3(ln_gn_stats_grid(m, channels), segments), dim3(256), 0, st, x, grad_y, scale_shift, relu,
              m, channels, acc, rows_device, row_starts, segments);
    LN_LAUNCH("k_gn_backward_apply_segments", k_gn_backward_apply_segments, dim3(ln_gn_segments_apply_grid(m, channels, segments), segments), dim3(256),
              0, st, x, grad_y, (const double*)acc, gamma, mean_rstd, scale_shift, m, channels, groups, relu, grad_x, parts,
              static_cast<double*>(next_workspace), int(next_workspace_bytes / sizeof(double)), rows_device, row_starts, segments);
    if (grad_gamma || grad_beta)
        LN_LAUNCH("k_gn_param_grads_segments", k_gn_param_grads_segments, dim3(ln_div_up(2 * channels, 256)), dim3(256), 0, st, (const double*)parts,
                  segments, channels, grad_gamma, grad_beta);
    return ln_check_launch("ln_group_norm_backward_segments");
}
