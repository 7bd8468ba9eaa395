// DeformSlice head on fp16 lattice values: gather and the fused slice + linear classifier, forward and backward.
//
// The lattice values are IEEE fp16 (`_Float16`) and are widened on load; everything else — delta_w, w, the classifier, grad_logits,
// every output and every accumulator — is fp32.  fp16 -> fp32 is exact, and each kernel here keeps the tiles, the grids, the slab
// layout and, per element, the operations and their order of its fp32 counterpart (k_slice_classify_forward_wave /
// k_slice_classify_backward_wave of ln_classify.hip, k_slice_classify_forward_v4 / k_slice_classify_backward_v4 and k_gather_forward
// of ln_rows.hip): every output equals, bit for bit, what the fp32 entry point gives on the same values widened to fp32.  The text
// is duplicated, not shared through a storage-type template: the fp32 kernels stay the compiler's output they were.
//
// Memory access: a lane that read a float4 (16 bytes) of a vertex row reads the same four channels as 8 bytes.  In the wave kernels
// the eight lanes of a point then cover a 64-byte half line per row and 32-channel chunk; the other half of the line is the next
// chunk of the same wave (forward: the next `ch` step; backward: u + 1 of the same lane, issued together), so lines are still
// fetched whole into L2 / the vector cache and no lane computes a second row address.  Raw fp16 words are kept in registers while
// the gathers are in flight (half the registers of the fp32 form) and widened where they are consumed.
//
// Only the wave-tiled and the float4 forms exist here: a shape at which the fp32 entry point would take a scalar form, V % 4 != 0
// or a misaligned pointer is LN_ERR_UNSUPPORTED with nothing written.
#include "ln_common.h"

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));

int ln_sc_backward_wave_grid(int n);  // ln_classify.hip

__device__ __forceinline__ void ln_wave_sync_h() {
    // LDS operations of one wave execute in program order; this only stops the compiler from moving them across
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int CTRL>
__device__ __forceinline__ float ln_dpp_h(float v) {  // the value of another lane of the row (DPP control CTRL), no LDS round trip
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// four channels of a row: one 8-byte load, widened where it is used
__device__ __forceinline__ halfx4 ln_ld_h4(const _Float16* p) { return *reinterpret_cast<const halfx4*>(p); }
__device__ __forceinline__ float4 ln_widen(halfx4 v) { return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w); }

#define LN_SCH_FWD_WAVES 3  // as LN_SCW_FWD_WAVES / LN_SCW_BWD_WAVES of ln_classify.hip
#define LN_SCH_BWD_WAVES 2
#define LN_SCH_SH 33        // row stride of the forward's h tile (floats)
#define LN_SCH_FWD_MAX_CPT 16  // as LN_SC_FWD_MAX_CPT / LN_SC_BLOCKS of ln_rows.hip
#define LN_SCH_BLOCKS 3

// ------------------------------------------------------------------------------------------
// gather: out[p, r, :] = (values[idx[p, r], :] * w[p, r], w[p, r]), absent vertices 0 (k_gather_forward)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    k_gather_forward_f16(const _Float16* __restrict__ values, const int* __restrict__ idx, const float* __restrict__ w, long long work,
                         int V, float* __restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= work) return;
    const long long pr = g / (V + 1);  // p*(d+1)+r
    const int j = int(g - pr * (V + 1));
    const int row = idx[pr];
    float o = 0.0f;
    if (row >= 0) {
        const float wt = w[pr];
        o = (j < V) ? (float)values[(size_t)row * V + j] * wt : wt;
    }
    out[g] = o;
}

extern "C" int ln_gather_forward_f16(const void* values_f16, const int* idx, const float* w, int n, int pos_dim, int val_dim, float* out,
                                     void* stream) {
    LN_REQUIRE(n >= 0 && pos_dim >= 1 && pos_dim <= LN_MAX_POS_DIM && val_dim >= 1, LN_ERR_ARG, "ln_gather_forward_f16: bad sizes n=%d d=%d V=%d",
               n, pos_dim, val_dim);
    LN_REQUIRE(n == 0 || (values_f16 && idx && w && out), LN_ERR_ARG, "ln_gather_forward_f16: null buffer");
    if (n == 0) return LN_OK;
    const long long work = (long long)n * (pos_dim + 1) * (val_dim + 1);
    LN_LAUNCH("k_gather_forward_f16", k_gather_forward_f16, dim3(ln_div_up(work, 256)), dim3(256), 0, (hipStream_t)stream,
              static_cast<const _Float16*>(values_f16), idx, w, work, val_dim, out);
    return ln_check_launch("ln_gather_forward_f16");
}

// ------------------------------------------------------------------------------------------
// forward, wave-tiled (k_slice_classify_forward_wave): tile = 64 points per wave, channels in chunks of 32
// ------------------------------------------------------------------------------------------
template <int DP1, int CT>
__global__ void __launch_bounds__(256, LN_SCH_FWD_WAVES)
    k_slice_classify_forward_wave_f16(const _Float16* __restrict__ values, const float* __restrict__ delta_w, const float* __restrict__ lin_w,
                                      const float* __restrict__ lin_b, const int* __restrict__ idx, const float* __restrict__ w, int n,
                                      int V, int C, float* __restrict__ logits) {
    __shared__ float s_h_all[4][64 * LN_SCH_SH];
    __shared__ float s_we_all[4][64 * DP1];
    __shared__ int s_idx_all[4][64 * DP1];
    extern __shared__ __attribute__((aligned(16))) float s_w[];  // [C][V] classifier weights
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* s_h = s_h_all[wave];
    float* s_we = s_we_all[wave];
    int* s_idx = s_idx_all[wave];
    const int tiles = (n + 63) >> 6;
    const int chunks = V >> 5;
    const int s = lane & 7;
    for (int e = threadIdx.x; e < C * V; e += 256) s_w[e] = lin_w[e];
    __syncthreads();
    // one batch = 2 points per 8-lane group x (d+1) vertex rows: 2 (d+1) half-line reads per lane; two batches in flight
    auto issue = [&](int ch, int bt, halfx4 (&x)[2][DP1], int (&rows)[2][DP1]) {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int lp = (bt * 2 + ps) * 8 + (lane >> 3);
#pragma unroll
            for (int r = 0; r < DP1; ++r) {
                rows[ps][r] = s_idx[lp * DP1 + r];
                x[ps][r] = ln_ld_h4(values + (size_t)(rows[ps][r] >= 0 ? rows[ps][r] : 0) * V + ch * 32 + s * 4);
            }
        }
    };
    auto finish = [&](int bt, const halfx4 (&x)[2][DP1], const int (&rows)[2][DP1]) {
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int lp = (bt * 2 + ps) * 8 + (lane >> 3);
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int r = 0; r < DP1; ++r) {
                // rows r ascending, an absent vertex is a zero row (h + 0 * w == h bit for bit)
                const bool ok = rows[ps][r] >= 0;
                const float wt = s_we[lp * DP1 + r];
                const float4 xv = ln_widen(x[ps][r]);
                h.x = h.x + (ok ? xv.x : 0.0f) * wt; h.y = h.y + (ok ? xv.y : 0.0f) * wt;
                h.z = h.z + (ok ? xv.z : 0.0f) * wt; h.w = h.w + (ok ? xv.w : 0.0f) * wt;
            }
            float* d = s_h + lp * LN_SCH_SH + s * 4;
            d[0] = h.x; d[1] = h.y; d[2] = h.z; d[3] = h.w;
        }
    };
    for (int tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
        const long long p0 = (long long)tile * 64;
        const long long tok_end = (long long)n * DP1;
#pragma unroll
        for (int k = 0; k < DP1; ++k) {
            const int i = lane + 64 * k;
            const long long t = p0 * DP1 + i;
            const bool ok = t < tok_end;
            s_idx[i] = ok ? idx[t] : -1;
            s_we[i] = ok ? w[t] + delta_w[t] : 0.0f;
        }
        ln_wave_sync_h();
        float acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = 0.0f;
        for (int ch = 0; ch < chunks; ++ch) {
            {
                halfx4 xa[2][DP1], xb[2][DP1];
                int ra[2][DP1], rb[2][DP1];
                issue(ch, 0, xa, ra);
                issue(ch, 1, xb, rb);
                finish(0, xa, ra);
                issue(ch, 2, xa, ra);
                finish(1, xb, rb);
                issue(ch, 3, xb, rb);
                finish(2, xa, ra);
                finish(3, xb, rb);
            }
            ln_wave_sync_h();
            float hv[32];
#pragma unroll
            for (int v = 0; v < 32; ++v) hv[v] = s_h[lane * LN_SCH_SH + v];
            // wave-uniform classifier weights broadcast from LDS, four classes' chains interleaved; padding classes recompute class
            // C - 1 and are dropped at the store
            const float* wch = s_w + ch * 32;
#pragma unroll
            for (int c0 = 0; c0 < CT; c0 += 4) {
                const float* wc[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) wc[k] = wch + (c0 + k < C ? c0 + k : C - 1) * V;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float4 w4[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) w4[k] = *reinterpret_cast<const float4*>(wc[k] + 4 * j);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[c0 + k] = acc[c0 + k] + w4[k].x * hv[4 * j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[c0 + k] = acc[c0 + k] + w4[k].y * hv[4 * j + 1];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[c0 + k] = acc[c0 + k] + w4[k].z * hv[4 * j + 2];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[c0 + k] = acc[c0 + k] + w4[k].w * hv[4 * j + 3];
                }
            }
            ln_wave_sync_h();  // the next chunk overwrites s_h
        }
        // logits of the tile are contiguous in HBM: stage [64][C] in LDS, store lane-linear
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) s_h[lane * C + c] = acc[c] + lin_b[c];
        ln_wave_sync_h();
        const long long left = (long long)n - p0;
        const int cnt = int(left < 64 ? left : 64) * C;
        float* out = logits + p0 * C;
        for (int i = lane; i < cnt; i += 64) out[i] = s_h[i];
        ln_wave_sync_h();
    }
}

// ------------------------------------------------------------------------------------------
// forward, float4 form (k_slice_classify_forward_v4)
// ------------------------------------------------------------------------------------------
template <int PB>
__global__ void __launch_bounds__(256)
    k_slice_classify_forward_v4_f16(const _Float16* __restrict__ values, const float* __restrict__ delta_w, const float* __restrict__ lin_w,
                                    const float* __restrict__ lin_b, const int* __restrict__ idx, const float* __restrict__ w, int n,
                                    int dp1, int V, int C, float* __restrict__ logits) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int SH = V + 1;                // row stride of W and h
    float* s_w = smem;                   // [C, V+1]
    float* s_h = s_w + C * SH;           // [PB, V+1]
    float* s_we = s_h + PB * SH;         // [PB, dp1]  w + delta_w
    int* s_idx = reinterpret_cast<int*>(s_we + PB * dp1);  // [PB, dp1]
    constexpr int TPP = 256 / PB;        // threads per point in the classifier phase
    const int tid = threadIdx.x;
    const int V4 = V >> 2;
    for (int i = tid; i < C * V; i += 256) {
        const int c = i / V;
        s_w[c * SH + (i - c * V)] = lin_w[i];
    }
    const int tiles = (n + PB - 1) / PB;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = (long long)tile * PB;
        __syncthreads();  // s_w staged / previous tile consumed
        for (int i = tid; i < PB * dp1; i += 256) {
            const long long t = p0 * dp1 + i;
            const bool ok = t < (long long)n * dp1;
            s_idx[i] = ok ? idx[t] : -1;
            s_we[i] = ok ? w[t] + delta_w[t] : 0.0f;
        }
        __syncthreads();
        for (int i = tid; i < PB * V4; i += 256) {
            const int lp = i / V4, v4 = i - lp * V4;
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            // all d+1 row gathers in flight before the first use; summation order and skips as in the fp32 kernel
            int rows[LN_MAX_POS_DIM + 1];
            halfx4 x[LN_MAX_POS_DIM + 1];
#pragma unroll
            for (int r = 0; r <= LN_MAX_POS_DIM; ++r) {
                rows[r] = -1;
                x[r] = halfx4{0, 0, 0, 0};
                if (r < dp1) {  // wave-uniform
                    rows[r] = s_idx[lp * dp1 + r];
                    x[r] = ln_ld_h4(values + (size_t)(rows[r] >= 0 ? rows[r] : 0) * V + v4 * 4);
                }
            }
#pragma unroll
            for (int r = 0; r <= LN_MAX_POS_DIM; ++r) {
                if (rows[r] >= 0) {
                    const float wt = s_we[lp * dp1 + r];
                    const float4 xv = ln_widen(x[r]);
                    h.x = h.x + xv.x * wt; h.y = h.y + xv.y * wt; h.z = h.z + xv.z * wt; h.w = h.w + xv.w * wt;
                }
            }
            float* d = s_h + lp * SH + v4 * 4;
            d[0] = h.x; d[1] = h.y; d[2] = h.z; d[3] = h.w;
        }
        __syncthreads();
        {
            const int lp = tid / TPP, q = tid - lp * TPP;
            const long long p = p0 + lp;
            if (p < n) {
                float acc[LN_SCH_FWD_MAX_CPT];
#pragma unroll
                for (int k = 0; k < LN_SCH_FWD_MAX_CPT; ++k) acc[k] = 0.0f;
                const float* hw = s_h + lp * SH;
                for (int v = 0; v < V; ++v) {
                    const float hv = hw[v];
#pragma unroll
                    for (int k = 0; k < LN_SCH_FWD_MAX_CPT; ++k) {
                        const int c = q + k * TPP;
                        if (c < C) acc[k] = acc[k] + s_w[c * SH + v] * hv;
                    }
                }
#pragma unroll
                for (int k = 0; k < LN_SCH_FWD_MAX_CPT; ++k) {
                    const int c = q + k * TPP;
                    if (c < C) logits[p * C + c] = acc[k] + lin_b[c];
                }
            }
        }
    }
}

// Form of a forward shape: 1 = wave-tiled, 2 = float4 with *pb points per tile, 0 = none here (fp32 takes a scalar kernel or refuses).
// The conditions are those of ln_sc_forward_wave and ln_slice_classify_forward with every alignment clause taken as met.
static int ln_sc_forward_form_f16(int pos_dim, int val_dim, int nr_classes, int* pb_out, size_t* lds_out) {
    if (val_dim % 32 == 0 && nr_classes <= 32 && (pos_dim == 2 || pos_dim == 3) &&
        sizeof(float) * (size_t)nr_classes * val_dim <= 16 * 1024) {
        *pb_out = 64;
        *lds_out = sizeof(float) * (size_t)nr_classes * val_dim;
        return 1;
    }
    if (val_dim % 4 == 0) {
        for (int pb = 64; pb >= 16; pb >>= 1) {
            const size_t lds4 = sizeof(float) * ((size_t)(nr_classes + pb) * (val_dim + 1) + 2 * (size_t)pb * (pos_dim + 1));
            const int cpt = ln_div_up(nr_classes, 256 / pb);
            if (lds4 > 64 * 1024 || cpt > LN_SCH_FWD_MAX_CPT) continue;
            *pb_out = pb;
            *lds_out = lds4;
            return 2;
        }
    }
    return 0;
}

extern "C" int ln_slice_classify_forward_f16(const void* values_f16, const float* delta_w, const float* lin_w, const float* lin_b,
                                             const int* idx, const float* w, int n, int pos_dim, int val_dim, int nr_classes,
                                             float* logits, void* stream) {
    LN_REQUIRE(n >= 0 && pos_dim >= 1 && pos_dim <= LN_MAX_POS_DIM && val_dim >= 1 && nr_classes >= 1, LN_ERR_ARG,
               "ln_slice_classify_forward_f16: bad sizes n=%d d=%d V=%d C=%d", n, pos_dim, val_dim, nr_classes);
    LN_REQUIRE(n == 0 || (values_f16 && delta_w && lin_w && lin_b && idx && w && logits), LN_ERR_ARG,
               "ln_slice_classify_forward_f16: null buffer");
    if (n == 0) return LN_OK;
    int pb = 0;
    size_t lds = 0;
    const int form = ln_sc_forward_form_f16(pos_dim, val_dim, nr_classes, &pb, &lds);
    LN_REQUIRE(form != 0, LN_ERR_UNSUPPORTED,
               "ln_slice_classify_forward_f16: V=%d C=%d d=%d has no wave-tiled or 4-channel form (V %% 4 == 0 and tiles within 64 KiB of LDS)",
               val_dim, nr_classes, pos_dim);
    LN_REQUIRE((reinterpret_cast<uintptr_t>(values_f16) & 7) == 0, LN_ERR_UNSUPPORTED,
               "ln_slice_classify_forward_f16: V=%d C=%d d=%d: values must be 8-byte aligned", val_dim, nr_classes, pos_dim);
    hipStream_t st = (hipStream_t)stream;
    const _Float16* values = static_cast<const _Float16*>(values_f16);
    if (form == 1) {
        const int grid = ln_div_up(ln_div_up(n, 64), 4);
#define LN_SCH_FWD(DP1, CT)                                                                                                                  \
    LN_LAUNCH("k_slice_classify_forward_f16", (k_slice_classify_forward_wave_f16<DP1, CT>), dim3(grid), dim3(256), lds, st, values, delta_w, \
              lin_w, lin_b, idx, w, n, val_dim, nr_classes, logits)
#define LN_SCH_FWD_C(DP1)                            \
    switch ((nr_classes + 3) / 4) {                  \
        case 1: LN_SCH_FWD(DP1, 4); break;           \
        case 2: LN_SCH_FWD(DP1, 8); break;           \
        case 3: LN_SCH_FWD(DP1, 12); break;          \
        case 4: LN_SCH_FWD(DP1, 16); break;          \
        case 5: LN_SCH_FWD(DP1, 20); break;          \
        case 6: LN_SCH_FWD(DP1, 24); break;          \
        case 7: LN_SCH_FWD(DP1, 28); break;          \
        default: LN_SCH_FWD(DP1, 32); break;         \
    }
        if (pos_dim == 3) {
            LN_SCH_FWD_C(4);
        } else {
            LN_SCH_FWD_C(3);
        }
#undef LN_SCH_FWD_C
#undef LN_SCH_FWD
        return ln_check_launch("ln_slice_classify_forward_f16");
    }
    int grid4 = ln_div_up(n, pb);
    if (grid4 > 2048) grid4 = 2048;
#define LN_SCH_FWD4(P)                                                                                                                  \
    if (pb == P)                                                                                                                        \
        LN_LAUNCH("k_slice_classify_forward_f16", k_slice_classify_forward_v4_f16<P>, dim3(grid4), dim3(256), lds, st, values, delta_w, \
                  lin_w, lin_b, idx, w, n, pos_dim + 1, val_dim, nr_classes, logits);
    LN_SCH_FWD4(64) LN_SCH_FWD4(32) LN_SCH_FWD4(16)
#undef LN_SCH_FWD4
    return ln_check_launch("ln_slice_classify_forward_f16");
}

// ------------------------------------------------------------------------------------------
// backward, wave-tiled (k_slice_classify_backward_wave): tile = 16 points per wave, both dense products on v_mfma_f32_16x16x4_f32
// ------------------------------------------------------------------------------------------
template <int DP1, int U, int CTL>
__global__ void __launch_bounds__(256, LN_SCH_BWD_WAVES)
    k_slice_classify_backward_wave_f16(const float* __restrict__ grad_logits, const _Float16* __restrict__ values,
                                       const float* __restrict__ delta_w, const float* __restrict__ lin_w, const int* __restrict__ idx,
                                       const float* __restrict__ w, int n, int C, float* __restrict__ g_delta_w,
                                       float* __restrict__ grad_sliced, float* __restrict__ w_eff, float* __restrict__ slabs) {
    constexpr int V = 32 * U;
    constexpr int NT = 2 * U;
    constexpr int KSMAX = 8;     // C <= 32
    // one tile buffer per wave: gh = g @ W in D-fragment order, overwritten in place by the sliced features h (stride V + 4)
    constexpr int SG = V + 4;
    constexpr int WAVE_LDS = 16 * SG;  // floats
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int KS = (C + 3) >> 2;  // K steps of gh = g @ W
    float* s_wb = smem;                                   // [KS][NT][64]  classifier in B-fragment order
    float* s_wave = s_wb + KS * NT * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* s_gh = s_wave + wave * WAVE_LDS;               // [16][SG]
    __shared__ float s_we_all[4][16 * DP1];
    __shared__ int s_idx_all[4][16 * DP1];
    __shared__ float s_dw_all[4][16 * DP1];
    float* s_we = s_we_all[wave];
    int* s_idx = s_idx_all[wave];
    float* s_dw = s_dw_all[wave];
    const int i = lane & 15, q = lane >> 4;
    for (int e = threadIdx.x; e < KS * NT * 64; e += 256) {
        const int l = e & 63, f = e >> 6;
        const int ks = f / NT, nt = f - ks * NT;
        const int c = ks * 4 + (l >> 4), v = nt * 16 + (l & 15);
        s_wb[e] = c < C ? lin_w[(size_t)c * V + v] : 0.0f;
    }
    __syncthreads();
    floatx4 acc_w[CTL][NT];
    floatx4 acc_b[CTL];
#pragma unroll
    for (int ct = 0; ct < CTL; ++ct) {
        acc_b[ct] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc_w[ct][nt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    const int tiles = (n + 15) >> 4;
    const long long tok_end = (long long)n * DP1;
    static_assert(16 * DP1 <= 64, "one token per lane");
    // what a tile needs from HBM before its first LDS access, fetched one tile ahead
    int t_idx = -1;
    float t_we = 0.0f, t_gdw = 0.0f;
    float a1[KSMAX];        // A fragments of gh = g @ W:    A[i = point][k = class]
    float a3[4][CTL];       // A fragments of gW += g^T h:   A[i = class][k = point]
    auto fetch = [&](int tile) {
        const long long p0 = (long long)tile * 16;
        const long long t = p0 * DP1 + lane;
        const bool ok = lane < 16 * DP1 && t < tok_end && tile < tiles;
        t_idx = ok ? idx[t] : -1;
        t_we = ok ? w[t] + delta_w[t] : 0.0f;
        t_gdw = ok ? g_delta_w[t] : 0.0f;
        const bool prow = p0 + i < n && tile < tiles;
        const float* grow = grad_logits + (p0 + i) * C;
#pragma unroll
        for (int ks = 0; ks < KSMAX; ++ks) {
            const int c = ks * 4 + q;
            a1[ks] = (prow && c < C) ? grow[c] : 0.0f;
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const long long p = p0 + ks * 4 + q;
#pragma unroll
            for (int ct = 0; ct < CTL; ++ct) {
                const int c = ct * 16 + i;
                a3[ks][ct] = (p < n && c < C && tile < tiles) ? grad_logits[p * C + c] : 0.0f;
            }
        }
    };
    const int stride = gridDim.x * 4;
    int tile = blockIdx.x * 4 + wave;
    fetch(tile);
    for (; tile < tiles; tile += stride) {
        const long long p0 = (long long)tile * 16;
        const float t_gdw_cur = t_gdw;
        if (lane < 16 * DP1) {
            s_idx[lane] = t_idx;
            s_we[lane] = t_we;
            if (p0 * DP1 + lane < tok_end) w_eff[p0 * DP1 + lane] = t_we;
        }
        // (1) gh = g @ W
        {
            floatx4 gh[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) gh[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KSMAX; ++ks) {
                if (ks < KS) {  // wave-uniform
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        gh[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[ks], s_wb[(ks * NT + nt) * 64 + lane], gh[nt], 0, 0, 0);
                }
            }
            // D: column = lane & 15 (channel), row = q * 4 + reg (point)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s_gh[(q * 4 + r) * SG + nt * 16 + i] = gh[nt][r];
        }
        float b3[4][CTL];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int ct = 0; ct < CTL; ++ct) b3[ks][ct] = a3[ks][ct];
        ln_wave_sync_h();
        // (2) gather: 8 lanes per point, U 8-byte words per lane and vertex row; two passes of 8 points
        {
            const int s = lane & 7;
            int rows[2][DP1];
            halfx4 x[2][DP1][U];
            auto issue = [&](int ps) {
                const int lp = ps * 8 + (lane >> 3);
#pragma unroll
                for (int r = 0; r < DP1; ++r) {
                    rows[ps][r] = s_idx[lp * DP1 + r];
                    const _Float16* src = values + (size_t)(rows[ps][r] >= 0 ? rows[ps][r] : 0) * V;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        x[ps][r][u] = ln_ld_h4(src + 4 * (s + 8 * u));
                    }
                }
            };
            auto finish = [&](int ps) {
                const int lp = ps * 8 + (lane >> 3);
                const long long p = p0 + lp;
                float dot[DP1];
#pragma unroll
                for (int r = 0; r < DP1; ++r) dot[r] = 0.0f;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float* cell = s_gh + lp * SG + 4 * (s + 8 * u);
                    const float4 g4 = *reinterpret_cast<const float4*>(cell);
                    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int r = 0; r < DP1; ++r) {
                        const bool ok = rows[ps][r] >= 0;
                        const float wt = s_we[lp * DP1 + r];
                        float4 xv = ln_widen(x[ps][r][u]);
                        xv.x = ok ? xv.x : 0.0f; xv.y = ok ? xv.y : 0.0f; xv.z = ok ? xv.z : 0.0f; xv.w = ok ? xv.w : 0.0f;
                        h.x = h.x + xv.x * wt; h.y = h.y + xv.y * wt; h.z = h.z + xv.z * wt; h.w = h.w + xv.w * wt;
                        dot[r] = dot[r] + (xv.x * g4.x + xv.y * g4.y + xv.z * g4.z + xv.w * g4.w);
                    }
                    *reinterpret_cast<float4*>(cell) = h;  // in place: gh of this cell has been read by this lane only
                    if (p < n) reinterpret_cast<float4*>(grad_sliced + (size_t)p * V)[s + 8 * u] = g4;
                }
#pragma unroll
                for (int r = 0; r < DP1; ++r) {  // sum over the 8 lanes of the point: DPP within the quad, then across the two quads
                    float d = dot[r];
                    d += ln_dpp_h<0xB1>(d);   // quad_perm [1,0,3,2]
                    d += ln_dpp_h<0x4E>(d);   // quad_perm [2,3,0,1]
                    d += ln_dpp_h<0x141>(d);  // row_half_mirror: lane i <-> 7 - i of each group of 8
                    if (s == r) s_dw[lp * DP1 + r] = rows[ps][r] >= 0 ? d : 0.0f;
                }
            };
            issue(0);
            if (U <= 2) issue(1);
            fetch(tile + stride);  // (behind this tile's row reads; past the last tile: zeros, nothing is loaded)
            finish(0);
            if (U > 2) issue(1);
            finish(1);
        }
        ln_wave_sync_h();
        // accumulated into: old value fetched with the tile's tokens, one lane-linear store
        if (lane < 16 * DP1 && p0 * DP1 + lane < tok_end) g_delta_w[p0 * DP1 + lane] = t_gdw_cur + s_dw[lane];
        // (3) gW += g^T @ [h | 1]: A[i = class][k = point], B[k = point][j = channel]
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float b = s_gh[(ks * 4 + q) * SG + nt * 16 + i];
#pragma unroll
                for (int ct = 0; ct < CTL; ++ct) acc_w[ct][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(b3[ks][ct], b, acc_w[ct][nt], 0, 0, 0);
            }
#pragma unroll
            for (int ct = 0; ct < CTL; ++ct) acc_b[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(b3[ks][ct], 1.0f, acc_b[ct], 0, 0, 0);
        }
        ln_wave_sync_h();  // the next tile overwrites s_gh / the token arrays
    }
    // one slab per workgroup: the four waves' accumulators summed through LDS (wave w adds after wave w - 1)
    __syncthreads();
    float* s_slab = s_wave;  // [C * V + C] floats <= 4 * WAVE_LDS = 64 (V + 4) (C <= 32)
    const int CV = C * V;
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int ct = 0; ct < CTL; ++ct) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = ct * 16 + q * 4 + r;
                    if (c < C) {
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) {
                            float* d = s_slab + c * V + nt * 16 + i;
                            *d = (wv ? *d : 0.0f) + acc_w[ct][nt][r];
                        }
                        if (i == 0) s_slab[CV + c] = (wv ? s_slab[CV + c] : 0.0f) + acc_b[ct][r];
                    }
                }
            }
        }
        __syncthreads();
    }
    float* slab = slabs + (size_t)blockIdx.x * (CV + C);
    for (int e = threadIdx.x; e < CV + C; e += 256) slab[e] = s_slab[e];
}

// ------------------------------------------------------------------------------------------
// backward, float4 form (k_slice_classify_backward_v4)
// ------------------------------------------------------------------------------------------
template <int PB>
__global__ void __launch_bounds__(256)
    k_slice_classify_backward_v4_f16(const float* __restrict__ grad_logits, const _Float16* __restrict__ values,
                                     const float* __restrict__ delta_w, const float* __restrict__ lin_w, const int* __restrict__ idx,
                                     const float* __restrict__ w, int n, int dp1, int V, int C, float* __restrict__ g_delta_w,
                                     float* __restrict__ grad_sliced, float* __restrict__ w_eff, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int CP = (C + 3) & ~3;
    float* s_h = smem;                  // [PB, V]
    float* s_gh = s_h + PB * V;         // [PB, V]
    float* s_g = s_gh + PB * V;         // [PB, CP]
    float* s_w = s_g + PB * CP;         // [C, V]
    float* s_we = s_w + C * V;          // [PB, dp1]  w + delta_w
    int* s_idx = reinterpret_cast<int*>(s_we + PB * dp1);  // [PB, dp1]
    const int tid = threadIdx.x;
    const int CV = C * V;
    const int V4 = V >> 2;
    for (int i = tid; i < CV; i += 256) s_w[i] = lin_w[i];
    const int cblocks = CP >> 2;
    const int nblocks = cblocks * V4;   // 4x4 blocks of (class, channel)
    float acc[LN_SCH_BLOCKS][16];
#pragma unroll
    for (int k = 0; k < LN_SCH_BLOCKS; ++k)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[k][j] = 0.0f;
    float acc_b = 0.0f;
    const int tiles = (n + PB - 1) / PB;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long p0 = (long long)tile * PB;
        __syncthreads();
        for (int i = tid; i < PB * CP; i += 256) {
            const int lp = i / CP, c = i - lp * CP;
            const long long p = p0 + lp;
            s_g[i] = (p < n && c < C) ? grad_logits[p * C + c] : 0.0f;
        }
        for (int i = tid; i < PB * dp1; i += 256) {  // the tile's row indices and effective weights, once
            const long long t = p0 * dp1 + i;
            const bool ok = t < (long long)n * dp1;
            const float we = ok ? w[t] + delta_w[t] : 0.0f;
            s_idx[i] = ok ? idx[t] : -1;
            s_we[i] = we;
            if (ok) w_eff[t] = we;
        }
        __syncthreads();
        for (int i = tid; i < PB * V4; i += 256) {
            const int lp = i / V4, v4 = i - lp * V4;
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            int rows[LN_MAX_POS_DIM + 1];
            halfx4 x[LN_MAX_POS_DIM + 1];
#pragma unroll
            for (int r = 0; r <= LN_MAX_POS_DIM; ++r) {
                rows[r] = -1;
                x[r] = halfx4{0, 0, 0, 0};
                if (r < dp1) {  // wave-uniform
                    rows[r] = s_idx[lp * dp1 + r];
                    x[r] = ln_ld_h4(values + (size_t)(rows[r] >= 0 ? rows[r] : 0) * V + v4 * 4);
                }
            }
#pragma unroll
            for (int r = 0; r <= LN_MAX_POS_DIM; ++r) {
                if (rows[r] >= 0) {
                    const float wt = s_we[lp * dp1 + r];
                    const float4 xv = ln_widen(x[r]);
                    h.x = h.x + xv.x * wt; h.y = h.y + xv.y * wt; h.z = h.z + xv.z * wt; h.w = h.w + xv.w * wt;
                }
            }
            reinterpret_cast<float4*>(s_h)[i] = h;
        }
        __syncthreads();
        for (int i = tid; i < PB * V4; i += 256) {  // gh = g @ W
            const int lp = i / V4, v4 = i - lp * V4;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            const float* gr = s_g + lp * CP;
            for (int c = 0; c < C; ++c) {
                const float g = gr[c];
                const float4 w4 = reinterpret_cast<const float4*>(s_w + c * V)[v4];
                a.x = fmaf(g, w4.x, a.x); a.y = fmaf(g, w4.y, a.y); a.z = fmaf(g, w4.z, a.z); a.w = fmaf(g, w4.w, a.w);
            }
            reinterpret_cast<float4*>(s_gh)[i] = a;
            if (p0 + lp < n) reinterpret_cast<float4*>(grad_sliced + (size_t)(p0 + lp) * V)[v4] = a;
        }
        __syncthreads();
        for (int i = tid; i < PB * dp1; i += 256) {  // delta-weight gradients
            const int lp = i / dp1, r = i - lp * dp1;
            const long long p = p0 + lp;
            if (p >= n) continue;
            const int row = s_idx[i];
            if (row < 0) continue;
            const _Float16* vr = values + (size_t)row * V;
            const float4* gh = reinterpret_cast<const float4*>(s_gh + lp * V);
            float dot = 0.0f;
            for (int v4 = 0; v4 < V4; ++v4) {
                const float4 a = ln_widen(ln_ld_h4(vr + 4 * v4)), b = gh[v4];
                dot = fmaf(a.x, b.x, dot); dot = fmaf(a.y, b.y, dot); dot = fmaf(a.z, b.z, dot); dot = fmaf(a.w, b.w, dot);
            }
            g_delta_w[p * dp1 + r] += dot;
        }
#pragma unroll
        for (int k = 0; k < LN_SCH_BLOCKS; ++k) {  // classifier weight gradient, 4 classes x 4 channels per block
            const int blk = tid + k * 256;
            if (blk < nblocks) {
                const int cb = blk / V4, vb = blk - cb * V4;
                const float* pg = s_g + cb * 4;
                const float* ph = s_h + vb * 4;
#pragma unroll 4
                for (int lp = 0; lp < PB; ++lp) {
                    const float4 g4 = *reinterpret_cast<const float4*>(pg + lp * CP);
                    const float4 h4 = *reinterpret_cast<const float4*>(ph + lp * V);
                    const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
                    const float hh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[k][a * 4 + b] = fmaf(gg[a], hh[b], acc[k][a * 4 + b]);
                }
            }
        }
        if (tid < C)
            for (int lp = 0; lp < PB; ++lp) acc_b = acc_b + s_g[lp * CP + tid];
    }
    float* slab = slabs + (size_t)blockIdx.x * (CV + C);
#pragma unroll
    for (int k = 0; k < LN_SCH_BLOCKS; ++k) {
        const int blk = tid + k * 256;
        if (blk < nblocks) {
            const int cb = blk / V4, vb = blk - cb * V4;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (cb * 4 + a < C)
#pragma unroll
                    for (int b = 0; b < 4; ++b) slab[(cb * 4 + a) * V + vb * 4 + b] = acc[k][a * 4 + b];
        }
    }
    if (tid < C) slab[CV + tid] = acc_b;
}

// Form of a backward shape: 1 = wave-tiled, 2 = float4 with *pb points per tile, 0 = none here.  The conditions are those of
// ln_sc_backward_wave and ln_slice_classify_backward with every alignment clause taken as met.
static int ln_sc_backward_form_f16(int pos_dim, int val_dim, int nr_classes, int* pb_out, size_t* lds_out) {
    if (val_dim % 32 == 0 && val_dim <= 128 && nr_classes <= 32 && (pos_dim == 2 || pos_dim == 3)) {
        const int ks = (nr_classes + 3) / 4, nt = val_dim / 16;
        *pb_out = 16;
        *lds_out = sizeof(float) * ((size_t)ks * nt * 64 + 4 * (size_t)(16 * (val_dim + 4)));
        return 1;
    }
    const int cp = (nr_classes + 3) & ~3;
    if (val_dim % 4 == 0 && (long long)cp * val_dim <= 256 * LN_SCH_BLOCKS * 16) {
        for (int cand = 64; cand >= 8; cand >>= 1) {
            const size_t lds = sizeof(float) * ((size_t)cand * (2 * val_dim + cp + 2 * (pos_dim + 1)) + (size_t)nr_classes * val_dim);
            if (lds <= 64 * 1024) {
                *pb_out = cand;
                *lds_out = lds;
                return 2;
            }
        }
    }
    return 0;
}

extern "C" size_t ln_slice_classify_backward_f16_workspace_bytes(int n, int pos_dim, int val_dim, int nr_classes) {
    (void)n;
    (void)pos_dim;
    return (size_t)LN_SC_MAX_SLABS * ((size_t)nr_classes * val_dim + nr_classes) * sizeof(float) + 256;
}

extern "C" int ln_slice_classify_backward_f16(const float* grad_logits, const void* values_f16, const float* delta_w, const float* lin_w,
                                              const int* idx, const float* w, int n, int pos_dim, int val_dim, int nr_classes,
                                              float* g_values, float* g_delta_w, float* g_lin_w, float* g_lin_b, float* grad_sliced,
                                              float* w_eff, void* workspace, size_t workspace_bytes, void* stream) {
    LN_REQUIRE(n >= 0 && pos_dim >= 1 && pos_dim <= LN_MAX_POS_DIM && val_dim >= 1 && nr_classes >= 1, LN_ERR_ARG,
               "ln_slice_classify_backward_f16: bad sizes n=%d d=%d V=%d C=%d", n, pos_dim, val_dim, nr_classes);
    LN_REQUIRE(g_values == nullptr, LN_ERR_ARG,
               "ln_slice_classify_backward_f16: g_values must be NULL (reduce grad_sliced with w_eff onto the vertices instead)");
    LN_REQUIRE(n == 0 || (grad_logits && values_f16 && idx && delta_w && lin_w && w && g_delta_w && g_lin_w && g_lin_b && grad_sliced && w_eff),
               LN_ERR_ARG, "ln_slice_classify_backward_f16: null buffer");
    if (n == 0) return LN_OK;
    int pb = 0;
    size_t lds = 0;
    const int form = ln_sc_backward_form_f16(pos_dim, val_dim, nr_classes, &pb, &lds);
    LN_REQUIRE(form != 0, LN_ERR_UNSUPPORTED,
               "ln_slice_classify_backward_f16: V=%d C=%d d=%d has no wave-tiled or 4-channel form (V %% 4 == 0, C V within %d, tiles within 64 KiB "
               "of LDS)", val_dim, nr_classes, pos_dim, 256 * LN_SCH_BLOCKS * 16);
    LN_REQUIRE((reinterpret_cast<uintptr_t>(values_f16) & 7) == 0 && (reinterpret_cast<uintptr_t>(grad_sliced) & 15) == 0, LN_ERR_UNSUPPORTED,
               "ln_slice_classify_backward_f16: V=%d C=%d d=%d: values must be 8-byte aligned and grad_sliced 16-byte aligned", val_dim,
               nr_classes, pos_dim);
    LN_REQUIRE(workspace && workspace_bytes >= ln_slice_classify_backward_f16_workspace_bytes(n, pos_dim, val_dim, nr_classes), LN_ERR_WORKSPACE,
               "ln_slice_classify_backward_f16: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const _Float16* values = static_cast<const _Float16*>(values_f16);
    const int dp1 = pos_dim + 1;
    float* slabs = static_cast<float*>(workspace);
    const int cv = nr_classes * val_dim;
    int grid = 0;
    if (form == 1) {
        grid = ln_sc_backward_wave_grid(n);
#define LN_SCH_BWD(DP1, U, CTL)                                                                                                                \
    LN_LAUNCH("k_slice_classify_backward_f16", (k_slice_classify_backward_wave_f16<DP1, U, CTL>), dim3(grid), dim3(256), lds, st, grad_logits, \
              values, delta_w, lin_w, idx, w, n, nr_classes, g_delta_w, grad_sliced, w_eff, slabs)
#define LN_SCH_BWD_U(DP1, CTL)                    \
    switch (val_dim / 32) {                       \
        case 1: LN_SCH_BWD(DP1, 1, CTL); break;   \
        case 2: LN_SCH_BWD(DP1, 2, CTL); break;   \
        case 3: LN_SCH_BWD(DP1, 3, CTL); break;   \
        default: LN_SCH_BWD(DP1, 4, CTL); break;  \
    }
        if (pos_dim == 3) {
            if (nr_classes > 16) { LN_SCH_BWD_U(4, 2) } else { LN_SCH_BWD_U(4, 1) }
        } else {
            if (nr_classes > 16) { LN_SCH_BWD_U(3, 2) } else { LN_SCH_BWD_U(3, 1) }
        }
#undef LN_SCH_BWD_U
#undef LN_SCH_BWD
    } else {
        grid = ln_div_up(n, pb);
        if (grid > 512) grid = 512;
#define LN_SCH_BWD4(P)                                                                                                                       \
    if (pb == P)                                                                                                                             \
        LN_LAUNCH("k_slice_classify_backward_f16", k_slice_classify_backward_v4_f16<P>, dim3(grid), dim3(256), lds, st, grad_logits, values, \
                  delta_w, lin_w, idx, w, n, dp1, val_dim, nr_classes, g_delta_w, grad_sliced, w_eff, slabs);
        LN_SCH_BWD4(64) LN_SCH_BWD4(32) LN_SCH_BWD4(16) LN_SCH_BWD4(8)
#undef LN_SCH_BWD4
    }
    // the gradient tensors are accumulated into; slabs added as by the fp32 call
    LN_LAUNCH("k_sc_reduce_slabs", ln_k_sum_slabs2<true>, dim3(ln_div_up(cv + nr_classes, 16)), dim3(256), 0, st, slabs, grid,
              (long long)(cv + nr_classes), cv + nr_classes, g_lin_w, g_lin_b, cv);
    return ln_check_launch("ln_slice_classify_backward_f16");
}
