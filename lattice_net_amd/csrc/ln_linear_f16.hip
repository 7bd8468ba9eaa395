// Per-vertex linear layer on fp16 lattice values (the 1 x 1 layers of GnRelu1x1 / BottleneckBlock / Conv1x1 on the half-precision feature
// path): a dense tall-and-skinny GEMM on gfx950's v_mfma_f32_16x16x32_f16 with no neighbour list and no identity indirection.  fp16
// rows, fp32 master weights (rounded to fp16, to nearest-even, once, when a workgroup stages its bank), fp32 accumulation, an optional
// bias and an optional residual row added in fp32 in the epilogue, one rounding on store.
//
// Product  out[r, c] = sum_k in[r, k] B[k, c]  (ln_linear_f16_plan.h: forward B[k, c] = h(w[c, k]); input gradient B[k, c] = h(w[k, c]))
//   * the matrix instruction computes the TRANSPOSE of a 16-row tile: the weights are its A operand (lane (i, q) holds the 8 halfs
//     B[32 s + 8 q + j, 16 nt + i], j = 0..7), the rows its B operand (lane (i, q) loads the 16 bytes in[m0 + i, 32 s + 8 q ..] — a
//     wave reads 16 rows x 64 contiguous bytes per step), so that a lane ends with FOUR CONSECUTIVE COLUMNS 16 nt + 4 q .. + 3 of row
//     m0 + i: bias, residual and the store are 8-byte (16-byte for the bias) vector accesses.  A row never meets another row's values:
//     a NaN in one row of `in` stays in that row of `out`, and the rows of a partial tile read a clamped index and select zero.
//   * the bank (chunk) is staged once per workgroup in fragment order, 16 bytes per lane and (step, nt), lane-linear: ds_read_b128 at
//     consecutive 16-byte slots, conflict-free; a workgroup then walks tiles_per_wg tiles of 64 rows.
// Weight gradient  gw[o, k] = sum_r gy[r, o] x[r, k]: the contraction runs down the rows, both operands staged row-major and read with
// the transposing LDS load (ds_read_b64_tr_b16) as in k_grad_filter_mfma_f16 (ln_conv_f16.hip); the bias gradient is one more matrix
// instruction against a fragment of ones in the tiles that start at column 0.  Per-chunk fp32 slabs, summed in slab order
// (ln_reduce_slabs_async): no float atomics, bitwise the same run to run.
#include "ln_common.h"
#include "ln_linear_f16_plan.h"

#include <hip/hip_fp16.h>

static_assert(LN_LIN16_OK == LN_OK && LN_LIN16_ERR_ARG == LN_ERR_ARG && LN_LIN16_ERR_UNSUPPORTED == LN_ERR_UNSUPPORTED &&
                  LN_LIN16_ERR_WORKSPACE == LN_ERR_WORKSPACE,
              "ln_linear_f16_plan.h restates the codes of latticenet_hip.h");

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));

// WT = false: bank[k, c] = w[c * K + k] (w [N_total, K]: the forward);  WT = true: bank[k, c] = w[k * N_total + c] (the input gradient)
template <int NT, bool K32, bool WT>
__global__ void __launch_bounds__(256)
    k_linear_mfma_f16(const _Float16* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                      const _Float16* __restrict__ residual, long long rows, int K, int n_total, int c_off, int tiles_per_wg,
                      _Float16* __restrict__ out) {
    constexpr int KS = K32 ? 8 : 4;        // halfs per lane and step
    constexpr int KSTEP = K32 ? 32 : 16;   // k per matrix instruction
    extern __shared__ __attribute__((aligned(16))) _Float16 s_w[];  // unit ((s * NT + nt) * 64 + lane) of KS halfs
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int i = lane & 15;
    const int q = lane >> 4;
    const int S = K / KSTEP;
    for (int u = tid; u < S * NT * 64; u += 256) {
        const int ul = u & 63, snt = u >> 6;
        const int nt = snt % NT, s = snt / NT;
        const int c = c_off + 16 * nt + (ul & 15);
        const int k0 = s * KSTEP + KS * (ul >> 4);
        float f[KS];
        if constexpr (WT) {
#pragma unroll
            for (int j = 0; j < KS; ++j) f[j] = w[(size_t)(k0 + j) * n_total + c];
        } else {
            const float2* src = reinterpret_cast<const float2*>(w + (size_t)c * K + k0);
#pragma unroll
            for (int j = 0; j < KS / 2; ++j) {
                const float2 v = src[j];
                f[2 * j] = v.x, f[2 * j + 1] = v.y;
            }
        }
        if constexpr (K32)
            *reinterpret_cast<halfx8*>(s_w + (size_t)u * 8) = halfx8{(_Float16)f[0], (_Float16)f[1], (_Float16)f[2], (_Float16)f[3],
                                                                    (_Float16)f[4], (_Float16)f[5], (_Float16)f[6], (_Float16)f[7]};
        else
            *reinterpret_cast<halfx4*>(s_w + (size_t)u * 4) = halfx4{(_Float16)f[0], (_Float16)f[1], (_Float16)f[2], (_Float16)f[3]};
    }
    __syncthreads();
    for (int t = 0; t < tiles_per_wg; ++t) {
        const long long tile0 = ((long long)blockIdx.x * tiles_per_wg + t) * LN_LIN16_TILE;
        if (tile0 >= rows) break;
        const long long row = tile0 + wave * 16 + i;
        const bool live = row < rows;
        const _Float16* src = in + (size_t)(live ? row : rows - 1) * K + KS * q;  // (a partial tile: the last row in its place, zero selected below)
        floatx4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
        halfx4 lo = *reinterpret_cast<const halfx4*>(src), hi = halfx4{0, 0, 0, 0};
        if constexpr (K32) hi = *reinterpret_cast<const halfx4*>(src + 4);
        for (int s = 0; s < S; ++s) {
            halfx4 a_lo = lo, a_hi = hi;
            if (s + 1 < S) {  // the next step's 16 bytes are on their way while this step's matrix instructions run
                lo = *reinterpret_cast<const halfx4*>(src + (s + 1) * KSTEP);
                if constexpr (K32) hi = *reinterpret_cast<const halfx4*>(src + (s + 1) * KSTEP + 4);
            }
            if (!live) a_lo = halfx4{0, 0, 0, 0}, a_hi = halfx4{0, 0, 0, 0};
            if constexpr (K32) {
                const halfx8 a = {a_lo[0], a_lo[1], a_lo[2], a_lo[3], a_hi[0], a_hi[1], a_hi[2], a_hi[3]};
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const halfx8 b = *reinterpret_cast<const halfx8*>(s_w + ((size_t)(s * NT + nt) * 64 + lane) * 8);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, acc[nt], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const halfx4 b = *reinterpret_cast<const halfx4*>(s_w + ((size_t)(s * NT + nt) * 64 + lane) * 4);
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x16f16(b, a_lo, acc[nt], 0, 0, 0);
                }
            }
        }
        // C/D layout: col = lane & 15 = the row of `in`, row = (lane >> 4) * 4 + reg = the output column within the sixteen
        if (live) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int c = c_off + 16 * nt + 4 * q;
                floatx4 v = acc[nt];
                if (bias) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = v[r] + bias[c + r];
                }
                if (residual) {
                    const halfx4 rs = *reinterpret_cast<const halfx4*>(residual + (size_t)row * n_total + c);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = v[r] + (float)rs[r];
                }
                *reinterpret_cast<halfx4*>(out + (size_t)row * n_total + c) = halfx4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            }
        }
    }
}

// any shape or alignment: one thread per output element, fp32 accumulation, the weight rounded to fp16 where it is read
__global__ void __launch_bounds__(256)
    k_linear_generic_f16(const _Float16* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                         const _Float16* __restrict__ residual, long long work, int K, int N, int wt, _Float16* __restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= work) return;
    const long long r = g / N;
    const int c = int(g - r * N);
    const _Float16* src = in + (size_t)r * K;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float wv = wt ? w[(size_t)k * N + c] : w[(size_t)c * K + k];
        acc = fmaf((float)src[k], (float)(_Float16)wv, acc);
    }
    if (bias) acc = acc + bias[c];
    if (residual) acc = acc + (float)residual[g];
    out[g] = (_Float16)acc;
}

// ---- executor of LnLin16Plan: the plan decides form, chunks, grid and block; the switch below only names the instance -----------------
template <bool WT>
static int ln_lin16_run(const char* what, const LnLin16Plan& p, const _Float16* in, const float* w, const float* bias, const _Float16* residual,
                        long long rows, int K, int N, _Float16* out, hipStream_t st) {
    if (p.form == LN_LIN16_GENERIC) {
        LN_REQUIRE(p.grid > 0, LN_ERR_UNSUPPORTED, "%s: %lld rows x %d columns are more than one launch reaches", what, rows, N);
        LN_LAUNCH("k_linear_generic_f16", k_linear_generic_f16, dim3(p.grid), dim3(p.block), 0, st, in, w, bias, residual, p.work, K, N, WT ? 1 : 0, out);
        return ln_check_launch(what);
    }
    for (int k = 0; k < p.n; ++k) {
        const LnF16Seg c = ln_lin16_chunk(p, k);
        const size_t lds = ln_lin16_bank_bytes(K, c.nt);
#define LN_LIN16_CASE(NN)                                                                                                            \
    if (c.nt == NN) {                                                                                                                \
        if (p.kstep == 32)                                                                                                           \
            LN_LAUNCH("k_linear_mfma_f16", (k_linear_mfma_f16<NN, true, WT>), dim3(p.grid), dim3(p.block), lds, st, in, w, bias, residual, rows, K, \
                      N, c.off, p.tiles_per_wg, out);                                                                                \
        else                                                                                                                         \
            LN_LAUNCH("k_linear_mfma_f16", (k_linear_mfma_f16<NN, false, WT>), dim3(p.grid), dim3(p.block), lds, st, in, w, bias, residual, rows, K, \
                      N, c.off, p.tiles_per_wg, out);                                                                                \
    }
        LN_LIN16_CASE(16) LN_LIN16_CASE(8) LN_LIN16_CASE(4) LN_LIN16_CASE(2) LN_LIN16_CASE(1)
#undef LN_LIN16_CASE
    }
    return ln_check_launch(what);
}
static_assert(ln_lin16_bank_bytes(LN_LIN16_MAX_C, ln_lin16_nt_max(LN_LIN16_MAX_C)) <= LN_LIN16_BANK_MAX &&
                  ln_lin16_bank_bytes(128, ln_lin16_nt_max(128)) <= LN_LIN16_BANK_MAX && LN_LIN16_BANK_MAX <= 64 * 1024,
              "the dynamic LDS of k_linear_mfma_f16 stays within what a launch gets without an attribute");

static unsigned ln_low4(const void* p) { return unsigned(reinterpret_cast<uintptr_t>(p) & 15); }

extern "C" int ln_linear_forward_f16(const void* x_f16, const float* w, const float* bias, const void* residual_f16, int rows, int cin, int cout,
                                     void* y_f16, void* stream) {
    const int refusal = ln_lin16_forward_refusal(LnLin16FwdArgs{x_f16 != nullptr, w != nullptr, y_f16 != nullptr, rows, cin, cout});
    LN_REQUIRE(refusal == LN_OK, refusal, "ln_linear_forward_f16: bad sizes (rows %d, cin %d, cout %d) or null buffer", rows, cin, cout);
    if (rows == 0) return LN_OK;
    // (the bias is read four bytes at a time: it has no say in the form)
    const LnLin16Plan p = ln_lin16_plan(LnLin16In{rows, cin, cout, ln_low4(x_f16) | ln_low4(w) | ln_low4(residual_f16) | ln_low4(y_f16)});
    return ln_lin16_run<false>("ln_linear_forward_f16", p, static_cast<const _Float16*>(x_f16), w, bias, static_cast<const _Float16*>(residual_f16), rows,
                               cin, cout, static_cast<_Float16*>(y_f16), (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// weight gradient gw[o, k] = sum_r gy[r, o] x[r, k] (and gb[o] = sum_r gy[r, o]) on the matrix cores: grid = row chunks, one launch per
// (VT, FT) tile of cout x cin.  A sub-tile of 64 rows of both operands is staged ROW-major (8-byte LDS stores, rows padded by 16 halfs:
// a stride of an odd multiple of 8 dwords, so the 8 rows a 32-lane group of a transposing read touches fall on disjoint banks) and read
// "down the rows" with ds_read_b64_tr_b16: lane i of a 16-lane group passes the address of row i >> 2, columns 4 (i & 3).. of a 4 x 16
// block and receives rows 0..3 of column i - the operand of a contraction over rows.  Rows from `rows` on are never read: zero is
// selected in their place.
// ------------------------------------------------------------------------------------------
template <int VT, int FT>
__global__ void __launch_bounds__(256)
    k_linear_grad_w_mfma_f16(const _Float16* __restrict__ x, const _Float16* __restrict__ gy, long long rows, int cin, int cout, int v_off, int f_off,
                             float* __restrict__ partial_w, float* __restrict__ partial_b) {
    constexpr int V = VT * 16, F = FT * 16;
    constexpr int TILES = VT * FT;
    constexpr int TPW = (TILES + 3) / 4;
    constexpr int SA = V + 16, SG = F + 16;
    __shared__ __attribute__((aligned(16))) _Float16 s_a[LN_LIN16_SUB * SA];  // gy[sub-tile rows, v_off .. v_off + V)
    __shared__ __attribute__((aligned(16))) _Float16 s_g[LN_LIN16_SUB * SG];  // x[sub-tile rows, f_off .. f_off + F)
    typedef short shortx4 __attribute__((ext_vector_type(4)));
    typedef short shortx8 __attribute__((ext_vector_type(8)));
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int i = lane & 15;
    const int q = lane >> 4;
    const long long chunk_begin = (long long)blockIdx.x * LN_LIN16_ROWS;
    const long long chunk_end = chunk_begin + LN_LIN16_ROWS < rows ? chunk_begin + LN_LIN16_ROWS : rows;
    const bool with_bias = partial_b != nullptr;  // (the launches at f_off == 0 of a call that wants grad_b)
    floatx4 acc[TPW], accb[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = accb[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    const halfx8 ones = {1, 1, 1, 1, 1, 1, 1, 1};
    // the rows of the NEXT sub-tile are fetched into registers while the matrix instructions of the current one run
    halfx4 ra[VT], rg[FT];
    auto fetch = [&](long long sub) {
#pragma unroll
        for (int k = 0; k < VT; ++k) {
            const int e = tid + 256 * k;
            const int r = e / (V / 4), c4 = e - r * (V / 4);
            ra[k] = halfx4{0, 0, 0, 0};
            if (sub + r < chunk_end) ra[k] = *reinterpret_cast<const halfx4*>(gy + (size_t)(sub + r) * cout + v_off + c4 * 4);
        }
#pragma unroll
        for (int k = 0; k < FT; ++k) {
            const int e = tid + 256 * k;
            const int r = e / (F / 4), c4 = e - r * (F / 4);
            rg[k] = halfx4{0, 0, 0, 0};
            if (sub + r < chunk_end) rg[k] = *reinterpret_cast<const halfx4*>(x + (size_t)(sub + r) * cin + f_off + c4 * 4);
        }
    };
    if (chunk_begin < chunk_end) fetch(chunk_begin);
    for (long long sub = chunk_begin; sub < chunk_end; sub += LN_LIN16_SUB) {
        __syncthreads();  // the previous sub-tile's reads are done
#pragma unroll
        for (int k = 0; k < VT; ++k) {
            const int e = tid + 256 * k;
            const int r = e / (V / 4), c4 = e - r * (V / 4);
            *reinterpret_cast<halfx4*>(s_a + r * SA + c4 * 4) = ra[k];
        }
#pragma unroll
        for (int k = 0; k < FT; ++k) {
            const int e = tid + 256 * k;
            const int r = e / (F / 4), c4 = e - r * (F / 4);
            *reinterpret_cast<halfx4*>(s_g + r * SG + c4 * 4) = rg[k];
        }
        __syncthreads();
        if (sub + LN_LIN16_SUB < chunk_end) fetch(sub + LN_LIN16_SUB);
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int tile = wave + 4 * t;
            if (tile < TILES) {
                const int vt = tile / FT, ft = tile - vt * FT;
                // rows 4q..4q+3 and 16+4q..16+4q+3 of the 32-row step (any order of the contraction that both operands share)
                const _Float16* pa = s_a + (4 * q + (i >> 2)) * SA + vt * 16 + 4 * (i & 3);
                const _Float16* pg = s_g + (4 * q + (i >> 2)) * SG + ft * 16 + 4 * (i & 3);
#pragma unroll
                for (int s = 0; s < LN_LIN16_SUB / 32; ++s) {
                    const shortx4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(pa + 32 * s * SA));
                    const shortx4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(pa + (32 * s + 16) * SA));
                    const shortx4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(pg + 32 * s * SG));
                    const shortx4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((shortx4 __attribute__((address_space(3)))*)(pg + (32 * s + 16) * SG));
                    const shortx8 a = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                    const shortx8 b = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(halfx8, a), __builtin_bit_cast(halfx8, b), acc[t], 0, 0, 0);
                    if (with_bias && ft == 0) accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(halfx8, a), ones, accb[t], 0, 0, 0);
                }
            }
        }
    }
    float* dst = partial_w + (size_t)blockIdx.x * ((size_t)cout * cin) + (size_t)v_off * cin + f_off;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tile = wave + 4 * t;
        if (tile < TILES) {
            const int vt = tile / FT, ft = tile - vt * FT;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(size_t)(vt * 16 + q * 4 + r) * cin + ft * 16 + i] = acc[t][r];
            if (with_bias && ft == 0 && i == 0) {  // every column of the product with ones is the row sum: column 0 writes it
#pragma unroll
                for (int r = 0; r < 4; ++r) partial_b[(size_t)blockIdx.x * cout + v_off + vt * 16 + q * 4 + r] = accb[t][r];
            }
        }
    }
}

// any shape or alignment (fallback): one thread per (o, k) pair, and per bias element behind the pairs, of one chunk of rows
__global__ void __launch_bounds__(256)
    k_linear_grad_w_f16(const _Float16* __restrict__ x, const _Float16* __restrict__ gy, long long rows, int cin, int cout,
                        float* __restrict__ partial_w, float* __restrict__ partial_b) {
    const long long pairs = (long long)cout * cin;
    const long long j = (long long)blockIdx.y * 256 + threadIdx.x;
    if (j >= pairs + (partial_b ? cout : 0)) return;
    const long long r0 = (long long)blockIdx.x * LN_LIN16_ROWS;
    const long long r1 = r0 + LN_LIN16_ROWS < rows ? r0 + LN_LIN16_ROWS : rows;
    float acc = 0.0f;
    if (j < pairs) {
        const int o = int(j / cin), k = int(j - (long long)o * cin);
        for (long long r = r0; r < r1; ++r) acc = fmaf((float)gy[(size_t)r * cout + o], (float)x[(size_t)r * cin + k], acc);
        partial_w[(size_t)blockIdx.x * pairs + j] = acc;
    } else {
        const int o = int(j - pairs);
        for (long long r = r0; r < r1; ++r) acc = acc + (float)gy[(size_t)r * cout + o];
        partial_b[(size_t)blockIdx.x * cout + o] = acc;
    }
}

extern "C" size_t ln_linear_backward_f16_workspace_bytes(int rows, int cin, int cout) { return ln_lin16_workspace_bytes(rows, cin, cout); }

extern "C" int ln_linear_backward_f16(const void* x_f16, const void* grad_y_f16, const float* w, int rows, int cin, int cout, void* grad_x_f16,
                                      float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes, void* stream) {
    const int refusal = ln_lin16_backward_refusal(LnLin16BwdArgs{x_f16 != nullptr, grad_y_f16 != nullptr, w != nullptr, grad_x_f16 != nullptr,
                                                                 grad_w != nullptr, workspace != nullptr, rows, cin, cout, workspace_bytes});
    LN_REQUIRE(refusal != LN_ERR_WORKSPACE, LN_ERR_WORKSPACE, "ln_linear_backward_f16: workspace of %zu bytes, %zu needed", workspace_bytes,
               ln_lin16_workspace_bytes(rows, cin, cout));
    LN_REQUIRE(refusal == LN_OK, refusal, "ln_linear_backward_f16: bad sizes (rows %d, cin %d, cout %d) or null buffer", rows, cin, cout);
    hipStream_t st = (hipStream_t)stream;
    const size_t pairs = (size_t)cout * cin;
    if (rows == 0) {
        (void)ln_zero_async(grad_w, pairs * sizeof(float), st);
        if (grad_b) (void)ln_zero_async(grad_b, (size_t)cout * sizeof(float), st);
        return ln_check_launch("ln_linear_backward_f16");
    }
    const _Float16* x = static_cast<const _Float16*>(x_f16);
    const _Float16* gy = static_cast<const _Float16*>(grad_y_f16);
    const LnLin16GwPlan g = ln_lin16_gw_plan(LnLin16GwIn{rows, cin, cout, grad_b != nullptr, ln_low4(x) | ln_low4(gy)});
    LN_REQUIRE(g.form != LN_LIN16_GW_UNSUPPORTED, LN_ERR_UNSUPPORTED, "ln_linear_backward_f16: cin %d x cout %d is more than the fallback's grid reaches", cin, cout);
    LnLin16Plan px = {};
    if (grad_x_f16) {
        px = ln_lin16_plan(LnLin16In{rows, cout, cin, ln_low4(gy) | ln_low4(w) | ln_low4(grad_x_f16)});
        LN_REQUIRE(px.form != LN_LIN16_GENERIC || px.grid > 0, LN_ERR_UNSUPPORTED, "ln_linear_backward_f16: %d rows x %d columns are more than one launch reaches", rows, cin);
    }
    float* partial_w = static_cast<float*>(workspace);
    float* partial_b = partial_w + ln_lin16_bias_slab_offset(rows, cin, cout);
    const dim3 grid(g.grid[0], g.grid[1], g.grid[2]), block(g.block);
    if (g.form == LN_LIN16_GW_MFMA) {
        for (int k = 0; k < g.n; ++k) {
            const LnLin16GwTile t = ln_lin16_gw_tile(g, cin, cout, k);
            float* pb = (grad_b && t.f_off == 0) ? partial_b : nullptr;
#define LN_LIN16_GW_CASE(A, B)                                                                                                       \
    if (t.vt == A && t.ft == B)                                                                                                      \
        LN_LAUNCH("k_linear_grad_w_mfma_f16", (k_linear_grad_w_mfma_f16<A, B>), grid, block, 0, st, x, gy, (long long)rows, cin, cout, t.v_off, t.f_off, \
                  partial_w, pb);
            LN_LIN16_GW_CASE(1, 1) LN_LIN16_GW_CASE(1, 2) LN_LIN16_GW_CASE(1, 4) LN_LIN16_GW_CASE(2, 1) LN_LIN16_GW_CASE(2, 2) LN_LIN16_GW_CASE(2, 4)
            LN_LIN16_GW_CASE(4, 1) LN_LIN16_GW_CASE(4, 2) LN_LIN16_GW_CASE(4, 4)
#undef LN_LIN16_GW_CASE
        }
    } else {
        LN_LAUNCH("k_linear_grad_w_f16", k_linear_grad_w_f16, grid, block, 0, st, x, gy, (long long)rows, cin, cout, partial_w, grad_b ? partial_b : nullptr);
    }
    (void)ln_reduce_slabs_async(partial_w, g.chunks, int(pairs), grad_w, st);
    if (grad_b) (void)ln_reduce_slabs_async(partial_b, g.chunks, cout, grad_b, st);
    if (grad_x_f16)
        return ln_lin16_run<true>("ln_linear_backward_f16", px, gy, w, nullptr, nullptr, rows, cout, cin, static_cast<_Float16*>(grad_x_f16), st);
    return ln_check_launch("ln_linear_backward_f16");
}
