// What a per-vertex linear layer on fp16 rows will launch, as plain integer arithmetic: no HIP include, no device code, so a host compiler
// builds this header alone (tests/cabi/linear_f16_plan_check.cpp does).  ln_linear_f16.hip holds the kernels and executors that walk a
// plan; ln_linear_backward_f16_workspace_bytes reads the same functions.  Every dispatch rule of the fp16 linear layer lives here, once:
//   * ln_lin16_plan: the form of one product out[rows, n] = in[rows, k] . bank (matrix-core kernel in column chunks / one thread per
//     output element).  ln_linear_forward_f16 is the product k = cin, n = cout; the input gradient of ln_linear_backward_f16 is the
//     product k = cout, n = cin over the same weights read as their transpose;
//   * ln_lin16_gw_plan: the form of the weight (and bias) gradient (matrix-core tiles over cout x cin / fallback);
//   * ln_lin16_workspace_bytes: the slabs both weight-gradient forms write;
//   * ln_lin16_forward_refusal / ln_lin16_backward_refusal: which calls are refused, and with which code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ln_conv_f16_plan.h"  // ln_f16_cdiv, LnF16Seg, ln_f16_seg, ln_f16_seg_count: how a dimension is walked in power-of-two segments

// ---- tuning constants shared by the plan and the kernels ---------------------------------------------------------------------------
#define LN_LIN16_MAX_C 256            // widest side of a matrix-core shape
#define LN_LIN16_TILE 64              // rows of one tile of the product kernel: four waves of 16
#define LN_LIN16_WGS 512              // workgroups of the product kernel at most: two on each of 256 CUs, each stages its bank once
#define LN_LIN16_BANK_MAX (64 * 1024)  // bytes of a staged bank (chunk): two workgroups fit the 160 KB of a CU
#define LN_LIN16_ROWS 512             // rows per workgroup of the weight gradient (one slab each)
#define LN_LIN16_SUB 64               // ... walked in sub-tiles of 64 rows by the matrix-core kernel
#define LN_LIN16_GRID_Y_MAX 65535

// the codes of include/latticenet_hip.h (a host compiler reads this header without it; ln_linear_f16.hip asserts they agree)
#define LN_LIN16_OK 0
#define LN_LIN16_ERR_ARG (-1)
#define LN_LIN16_ERR_UNSUPPORTED (-2)
#define LN_LIN16_ERR_WORKSPACE (-4)

// ---- the product out = in . bank ----------------------------------------------------------------------------------------------------
enum LnLin16Form : uint8_t {
    LN_LIN16_MFMA,     // k_linear_mfma_f16<nt, K32, WT>: one launch per column chunk (ln_lin16_chunk), the chunk's bank staged once per workgroup
    LN_LIN16_GENERIC,  // k_linear_generic_f16: any shape or alignment, one thread per output element
};
struct LnLin16In {
    long long rows;  // >= 1
    int k, n;        // contraction length, output columns
    unsigned low;    // the low four bits of every pointer the call passes, or-ed together
};
struct LnLin16Plan {
    uint8_t form;
    int kstep;         // matrix-core: 32 (v_mfma_f32_16x16x32_f16) or 16 (the 16x16x16 form: k no multiple of 32)
    int nt;            // matrix-core: the widest chunk, in sixteenths
    int cols16;        // matrix-core: n / 16, what ln_lin16_chunk walks
    int n;             // launches
    int grid, block;   // of every launch
    int tiles_per_wg;  // matrix-core: tiles of 64 rows a workgroup walks behind one staging of the bank
    long long work;    // generic: output elements
};
constexpr bool ln_lin16_mfma_shape(int k, int n) { return k % 16 == 0 && n % 16 == 0 && k <= LN_LIN16_MAX_C && n <= LN_LIN16_MAX_C; }
// bytes of LDS of a chunk of nt sixteenths: the bank slice [k, 16 nt] in halfs, in fragment order
constexpr size_t ln_lin16_bank_bytes(int k, int nt) { return (size_t)k * 16 * nt * 2; }
// the widest chunk: the whole of 256 columns where that leaves room for two workgroups per CU (k <= 128), 128 columns beyond
constexpr int ln_lin16_nt_max(int k) { return ln_lin16_bank_bytes(k, 16) <= LN_LIN16_BANK_MAX ? 16 : 8; }
// the k-th launch of a matrix-core plan: output columns [off, off + 16 nt)
constexpr LnF16Seg ln_lin16_chunk(const LnLin16Plan& p, int k) { return ln_f16_seg(p.cols16, p.nt, k); }

inline LnLin16Plan ln_lin16_plan(const LnLin16In& in) {
    LnLin16Plan p = {};
    p.block = 256;
    if (ln_lin16_mfma_shape(in.k, in.n) && (in.low & 7) == 0) {
        p.form = LN_LIN16_MFMA;
        p.kstep = in.k % 32 == 0 ? 32 : 16;
        p.nt = ln_lin16_nt_max(in.k);
        p.cols16 = in.n / 16;
        p.n = ln_f16_seg_count(p.cols16, p.nt);
        const long long tiles = (in.rows + LN_LIN16_TILE - 1) / LN_LIN16_TILE;
        p.tiles_per_wg = int((tiles + LN_LIN16_WGS - 1) / LN_LIN16_WGS);
        p.grid = int((tiles + p.tiles_per_wg - 1) / p.tiles_per_wg);
        return p;
    }
    p.form = LN_LIN16_GENERIC;
    p.work = in.rows * in.n;
    p.n = 1;
    const long long grid = (p.work + 255) / 256;
    p.grid = grid <= 0x7fffffffLL ? int(grid) : 0;  // 0: more elements than a grid of 256-thread workgroups reaches (refused)
    return p;
}

// ---- weight and bias gradient -------------------------------------------------------------------------------------------------------
// one [cout, cin] fp32 slab per chunk of LN_LIN16_ROWS rows, then one [cout] slab per chunk for the bias, whichever form runs
constexpr long long ln_lin16_chunks(long long rows) { return rows <= 0 ? 0 : (rows + LN_LIN16_ROWS - 1) / LN_LIN16_ROWS; }
constexpr size_t ln_lin16_bias_slab_offset(long long rows, int cin, int cout) {  // in floats
    return (size_t)ln_lin16_chunks(rows) * (size_t)cout * (size_t)cin;
}
constexpr size_t ln_lin16_workspace_bytes(long long rows, int cin, int cout) {
    if (rows <= 0 || cin < 1 || cout < 1) return 256;
    return (ln_lin16_bias_slab_offset(rows, cin, cout) + (size_t)ln_lin16_chunks(rows) * (size_t)cout) * sizeof(float) + 256;
}

enum LnLin16GwForm : uint8_t {
    LN_LIN16_GW_MFMA,         // k_linear_grad_w_mfma_f16<vt, ft>: one launch per tile (ln_lin16_gw_tile), then the slab sums
    LN_LIN16_GW_FALLBACK,     // k_linear_grad_w_f16: any shape, one thread per (o, k) pair and per bias element of a chunk; then the slab sums
    LN_LIN16_GW_UNSUPPORTED,  // more pairs than gridDim.y of the fallback reaches, or more slabs than the slab sum takes: refused
};
struct LnLin16GwIn {
    long long rows;  // >= 1
    int cin, cout;
    bool bias;     // grad_b wanted
    unsigned low;  // the low four bits of x and grad_y, or-ed together
};
struct LnLin16GwPlan {
    uint8_t form;
    int chunks;  // slabs written
    int nv, nf;  // matrix-core: tiles along cout and along cin
    int n;       // launches in front of the slab sums
    int grid[3], block;
};
struct LnLin16GwTile {
    int vt, ft, v_off, f_off;  // sixteenths of cout and of cin, offsets in channels; the tiles with f_off == 0 also sum the bias gradient
};
// the k-th launch of a matrix-core plan: cout outer, cin inner
constexpr LnLin16GwTile ln_lin16_gw_tile(const LnLin16GwPlan& p, int cin, int cout, int k) {
    const LnF16Seg v = ln_f16_seg(cout / 16, 4, k / p.nf), f = ln_f16_seg(cin / 16, 4, k % p.nf);
    return LnLin16GwTile{v.nt, f.nt, v.off, f.off};
}

inline LnLin16GwPlan ln_lin16_gw_plan(const LnLin16GwIn& in) {
    LnLin16GwPlan p = {};
    p.block = 256;
    const long long chunks = ln_lin16_chunks(in.rows);
    const long long elems = (long long)in.cout * in.cin + in.cout;
    if (chunks > 0x7fffffffLL / 2 || elems > 0x7fffffffLL / 2) {
        p.form = LN_LIN16_GW_UNSUPPORTED;
        return p;
    }
    p.chunks = int(chunks);
    p.grid[0] = p.chunks, p.grid[1] = 1, p.grid[2] = 1;
    if (ln_lin16_mfma_shape(in.cin, in.cout) && (in.low & 7) == 0) {
        p.form = LN_LIN16_GW_MFMA;
        p.nv = ln_f16_seg_count(in.cout / 16, 4);
        p.nf = ln_f16_seg_count(in.cin / 16, 4);
        p.n = p.nv * p.nf;
        return p;
    }
    const long long gy = (elems + 255) / 256;  // (bias elements behind the pairs, wanted or not: one grid for both calls)
    if (gy > LN_LIN16_GRID_Y_MAX) {
        p.form = LN_LIN16_GW_UNSUPPORTED;
        p.grid[0] = 0;
        return p;
    }
    p.form = LN_LIN16_GW_FALLBACK;
    p.n = 1;
    p.grid[1] = int(gy);
    return p;
}

// ---- refusals: checked in this order, the first that holds decides; a refused call launches nothing ---------------------------------
struct LnLin16FwdArgs {
    bool x, w, y;  // pointer is not null (bias and residual are optional)
    long long rows;
    int cin, cout;
};
inline int ln_lin16_forward_refusal(const LnLin16FwdArgs& a) {
    if (a.rows < 0 || a.cin < 1 || a.cout < 1) return LN_LIN16_ERR_ARG;
    if (a.rows > 0 && !(a.x && a.w && a.y)) return LN_LIN16_ERR_ARG;
    return LN_LIN16_OK;
}
struct LnLin16BwdArgs {
    bool x, grad_y, w, grad_x, grad_w, workspace;  // pointer is not null (grad_b is optional; w is read for grad_x only)
    long long rows;
    int cin, cout;
    size_t workspace_bytes;
};
inline int ln_lin16_backward_refusal(const LnLin16BwdArgs& a) {
    if (a.rows < 0 || a.cin < 1 || a.cout < 1) return LN_LIN16_ERR_ARG;
    if (!a.grad_w) return LN_LIN16_ERR_ARG;
    if (a.rows == 0) return LN_LIN16_OK;  // nothing is read: grad_w and grad_b are written as zeros, the workspace is not touched
    if (!(a.x && a.grad_y) || (a.grad_x && !a.w)) return LN_LIN16_ERR_ARG;
    if (!a.workspace || a.workspace_bytes < ln_lin16_workspace_bytes(a.rows, a.cin, a.cout)) return LN_LIN16_ERR_WORKSPACE;
    return LN_LIN16_OK;
}
