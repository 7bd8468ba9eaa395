// What a half-precision convolution call will launch, as plain integer arithmetic: no HIP include, no device code, so a host compiler
// builds this header alone (tests/cabi/conv_f16_plan_check.cpp does).  ln_conv_f16.hip holds the kernels and executors that walk a
// plan; ln_conv_grad_filter_f16_workspace_bytes reads the same functions.  Every dispatch rule of the fp16 convolution lives here, once:
//   * ln_f16_forward_plan: the form ln_conv_forward_f16 takes (whole bank in LDS / per-slot matrix-core kernel in column chunks /
//     one thread per output element), its grid, block and LDS;
//   * ln_f16_gf_plan: the form ln_conv_grad_filter_f16 takes (matrix-core tiles over V x F / scalar fallback / refusal);
//   * ln_f16_gf_workspace_bytes: the slabs both filter-gradient forms write.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- tuning constants shared by the plan and the kernels ---------------------------------------------------------------------------
#define LN_GF16_ROWS 512  // lattice vertices per workgroup of the filter gradient (one slab each)
#define LN_GF16_SUB 64    // ... walked in sub-tiles of 64 rows by the matrix-core kernel
#define LN_GF16_GSUB 32   // ... and of 32 rows by the fallback
#define LN_GF16_PAIRS 4096  // (v, f) pairs per workgroup of the fallback: 16 per thread; gridDim.z walks V * F
#define LN_GF16_MAX_LDS (64 * 1024)
// k_conv_f16_tiled: at most 1024 threads = 16 waves = 256 rows per workgroup; at 64 gathered channels every wave has a private region
// through which it re-shapes its 16 gathered rows of 128 bytes, and the workgroup stages the ids of its rows (static_asserts beside the
// kernel tie these to its arrays)
#define LN_F16_TILED_MAX_WAVES 16
#define LN_F16_TILED_REGION_BYTES 2048
#define LN_F16_TILED_MAX_ROWS 256
#define LN_F16_SLOT_LDS_MAX (32 * 1024)  // the per-slot kernel's filter slice of one slot

constexpr int ln_f16_cdiv(long long a, long long b) { return int((a + b - 1) / b); }

// A dimension of n sixteenths (V / 16 or F / 16) is walked in segments of `widest` sixteenths while that many are left, then in at most
// one segment of each narrower power of two: the column chunks of the per-slot forward (widest = 8 or 4) and the tiles of the filter
// gradient (widest = 4, both dimensions).
struct LnF16Seg {
    int nt, off;  // width in sixteenths, offset in channels
};
constexpr int ln_f16_seg_count(int n, int widest) {
    int cnt = n / widest;
    for (int nt = widest >> 1, rest = n % widest; nt >= 1; nt >>= 1)
        if (rest >= nt) ++cnt, rest -= nt;
    return cnt;
}
constexpr LnF16Seg ln_f16_seg(int n, int widest, int k) {
    if (k < n / widest) return LnF16Seg{widest, k * widest * 16};
    k -= n / widest;
    int off = n / widest * widest;
    for (int nt = widest >> 1; nt >= 1; nt >>= 1)
        if (n - off >= nt) {
            if (k == 0) return LnF16Seg{nt, off * 16};
            off += nt, --k;
        }
    return LnF16Seg{0, n * 16};
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// gathered channel counts the per-slot kernel k_conv_mfma_f16 is instantiated for
constexpr bool ln_f16_per_slot_v(int V) { return V == 16 || V == 32 || V == 64 || V == 96 || V == 128 || V == 256; }
// widest column chunk (in sixteenths) of the per-slot kernel: the LDS of one slot's filter slice, V x 16 NT halfs, stays within 32 KB
constexpr size_t ln_f16_per_slot_lds(int V, int NT) { return (size_t)V * 16 * NT * 2; }
constexpr int ln_f16_nt_max(int V) { return ln_f16_per_slot_lds(V, 8) <= LN_F16_SLOT_LDS_MAX ? 8 : 4; }
// whole bank in LDS (k_conv_f16_tiled): E = 9, V and F in {32, 64}
constexpr bool ln_f16_tiled_shape(int E, int V, int F) { return E == 9 && (V == 32 || V == 64) && (F == 32 || F == 64); }
// line-shaped gathers (128-byte rows, re-shaped through LDS) at V = 64, fragment-shaped loads at V = 32
constexpr bool ln_f16_tiled_line(int V) { return V == 64; }
// bytes of LDS of a tiled workgroup that the choice of the sub-tile count goes by: the bank, and at 64 channels the re-shaping regions
// of up to 16 waves and the ids (see the kernel)
constexpr size_t ln_f16_tiled_lds(int V, int F) {
    return (size_t)9 * V * F * 2 + (ln_f16_tiled_line(V) ? LN_F16_TILED_MAX_WAVES * LN_F16_TILED_REGION_BYTES + LN_F16_TILED_MAX_ROWS * 9 * sizeof(int) : 0);
}

// sub-tiles per workgroup of k_conv_f16_tiled: the launch runs in rounds of 256 CUs x (workgroups that fit a CU's LDS); the T with the
// cheapest rounds(T) * T wins, larger T (fewer bank stagings) on ties.
inline int ln_f16_subtiles(int m, size_t lds_bytes) {
    const int per_cu = lds_bytes * 2 <= 150 * 1024 ? 2 : 1;
    const int tiles = (m + 63) / 64;
    int best = 1, best_cost = 1 << 30;
    for (int t = 1; t <= 4; ++t) {
        if (per_cu * t * 4 > 32) break;  // wave slots of a CU
        // (one workgroup per CU: a single sub-tile would leave the CU with four waves — 39 us instead of 21 at C5 — unless the lattice
        // is too small to give every CU more)
        if (per_cu == 1 && t < 3 && tiles >= 3 * 256) continue;
        const int wgs = (tiles + t - 1) / t;
        const int cost = ((wgs + 256 * per_cu - 1) / (256 * per_cu)) * t;
        if (cost <= best_cost) {
            best = t;
            best_cost = cost;
        }
    }
    return best;
}

enum LnF16FwdForm : uint8_t {
    LN_F16_FWD_TILED,    // k_conv_f16_tiled<V, nt, FLIP, WT>: one launch, t sub-tiles of 64 rows per workgroup
    LN_F16_FWD_SLOTS,    // k_conv_mfma_f16<V, nt, FLIP, WT>: one launch per column chunk (ln_f16_chunk), 64 rows per workgroup
    LN_F16_FWD_GENERIC,  // k_conv_generic_f16: any shape, one thread per output element
};
struct LnF16FwdIn {
    int m, E, V, F;                   // rows (>= 1), filter extent, gathered channels, output columns
    int flags;                        // LN_CONV_FLIP_NEIGHBOURS | LN_CONV_TRANSPOSED_FILTER: choose the template instance, no form
    unsigned values_low, filter_low;  // the low four bits of the two pointers
};
struct LnF16FwdPlan {
    uint8_t form;
    bool flip, wt;     // template arguments of every launch (the executor picks the instance by them)
    int V;             // tiled, per-slot: template argument
    int nt;            // tiled: F / 16; per-slot: the widest chunk
    int t;             // tiled: sub-tiles per workgroup
    bool line;         // tiled: line-shaped gather (V = 64) or fragment-shaped (V = 32)
    int kstep;         // per-slot: 32 (v_mfma_f32_16x16x32_f16) or 16 (V = 16: the 16x16x16 form)
    int cols16;        // per-slot: F / 16, what ln_f16_chunk walks
    int n;             // launches
    int grid, block;   // of every launch
    size_t lds;        // tiled: the static LDS of a workgroup that chose t
    long long work;    // generic: output elements
};
// the k-th launch of a per-slot plan: output columns [off, off + 16 nt)
constexpr LnF16Seg ln_f16_chunk(const LnF16FwdPlan& p, int k) { return ln_f16_seg(p.cols16, p.nt, k); }

inline LnF16FwdPlan ln_f16_forward_plan(const LnF16FwdIn& in) {
    LnF16FwdPlan p = {};
    p.flip = (in.flags & 1) != 0;
    p.wt = (in.flags & 2) != 0;
    p.V = in.V;
    p.block = 256;
    if (ln_f16_tiled_shape(in.E, in.V, in.F) && ((in.values_low | in.filter_low) & 15) == 0) {
        p.form = LN_F16_FWD_TILED;
        p.nt = in.F / 16;
        p.line = ln_f16_tiled_line(in.V);
        p.lds = ln_f16_tiled_lds(in.V, in.F);
        p.t = ln_f16_subtiles(in.m, p.lds);
        p.n = 1;
        p.grid = ln_f16_cdiv(in.m, 64 * p.t);
        p.block = 256 * p.t;
        return p;
    }
    if (in.F % 16 == 0 && (in.values_low & 7) == 0 && ln_f16_per_slot_v(in.V)) {
        p.form = LN_F16_FWD_SLOTS;
        p.nt = ln_f16_nt_max(in.V);
        p.kstep = in.V % 32 == 0 ? 32 : 16;
        p.cols16 = in.F / 16;
        p.n = ln_f16_seg_count(p.cols16, p.nt);
        p.grid = ln_f16_cdiv(in.m, 64);
        return p;
    }
    p.form = LN_F16_FWD_GENERIC;
    p.work = (long long)in.m * in.F;
    p.n = 1;
    p.grid = ln_f16_cdiv(p.work, 256);
    return p;
}

// ---- filter gradient ----------------------------------------------------------------------------------------------------------------
// one [E, V, F] fp32 slab per chunk of LN_GF16_ROWS rows, whichever form runs
constexpr size_t ln_f16_gf_workspace_bytes(int m, int E, int V, int F) {
    if (m <= 0) return 256;
    return (size_t)ln_f16_cdiv(m, LN_GF16_ROWS) * E * V * F * sizeof(float) + 256;
}

enum LnF16GfForm : uint8_t {
    LN_F16_GF_MFMA,         // k_grad_filter_mfma_f16<vt, ft>: one launch per tile (ln_f16_gf_tile), then the slab sum
    LN_F16_GF_FALLBACK,     // k_grad_filter_f16: any shape, gridDim.z walks V * F, rows staged as floats in dynamic LDS; then the slab sum
    LN_F16_GF_UNSUPPORTED,  // the fallback's rows do not fit LDS: the call is refused, nothing is launched
};
struct LnF16GfIn {
    int m, E, V, F;                     // rows (>= 1)
    unsigned values_low, grad_out_low;  // the low four bits of the two pointers
};
struct LnF16GfPlan {
    uint8_t form;
    int chunks;        // slabs written
    int nv, nf;        // matrix-core: tiles along V and along F
    int n;             // launches in front of the slab sum
    int grid[3], block;
    size_t lds;        // fallback: dynamic LDS bytes
};
struct LnF16GfTile {
    int vt, ft, v_off, f_off;
};
// the k-th launch of a matrix-core plan: v outer, f inner
constexpr LnF16GfTile ln_f16_gf_tile(const LnF16GfPlan& p, int V, int F, int k) {
    const LnF16Seg v = ln_f16_seg(V / 16, 4, k / p.nf), f = ln_f16_seg(F / 16, 4, k % p.nf);
    return LnF16GfTile{v.nt, f.nt, v.off, f.off};
}

inline LnF16GfPlan ln_f16_gf_plan(const LnF16GfIn& in) {
    LnF16GfPlan p = {};
    p.chunks = ln_f16_cdiv(in.m, LN_GF16_ROWS);
    p.block = 256;
    p.grid[0] = p.chunks, p.grid[1] = in.E, p.grid[2] = 1;
    if (in.V % 16 == 0 && in.F % 16 == 0 && ((in.values_low | in.grad_out_low) & 7) == 0) {
        p.form = LN_F16_GF_MFMA;
        p.nv = ln_f16_seg_count(in.V / 16, 4);
        p.nf = ln_f16_seg_count(in.F / 16, 4);
        p.n = p.nv * p.nf;
        return p;
    }
    p.lds = sizeof(float) * LN_GF16_GSUB * ((size_t)in.V + in.F);
    if (p.lds > LN_GF16_MAX_LDS) {
        p.form = LN_F16_GF_UNSUPPORTED;
        p.grid[0] = p.grid[1] = 0;
        return p;
    }
    p.form = LN_F16_GF_FALLBACK;
    p.n = 1;
    p.grid[2] = ln_f16_cdiv((long long)in.V * in.F, LN_GF16_PAIRS);
    return p;
}
