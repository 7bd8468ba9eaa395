// What a convolution call will launch, as plain integer arithmetic: no HIP include, no device code, so a host compiler builds
// this header alone (tests/cabi/conv_plan_check.cpp does).  ln_conv.hip holds the kernels and an executor that walks a plan; the
// *_workspace_bytes queries read the same functions.  Every dispatch rule of the lattice convolution lives here, once:
//   * the shape predicates (constexpr): used by the plan at run time and by the executor inside `if constexpr`, so the set of
//     instantiated kernels and the set of plannable launches cannot drift apart;
//   * ln_conv_layout: bank bytes and slot split of the per-slot form for a shape (what the size queries report);
//   * ln_conv_plan: the ordered launches of ln_conv_forward_ws for one call, clipped to the workspace on offer;
//   * ln_gf_plan / ln_conv_backward_plan: the filter gradient's launch and the form ln_conv_backward takes.
#pragma once
#include <stddef.h>
#include <stdint.h>

// ---- tuning constants shared by the plan and the kernels (measured notes kept with them) ----------------------------------------
// fused backward of a same-lattice small-filter convolution (k_conv_backward_fused): vertices per workgroup, shapes it covers
#define LN_BWD_MAX_SUBTILES 4
#define LN_BWD_CUS 256
#ifndef LN_BWD_B3_MAX_T
#define LN_BWD_B3_MAX_T 3  // sub-tiles of the bf16x3 form: four fit the LDS since round 6 (unpadded staging) but need 148 registers of the 128 a
                           // 1024-thread workgroup may have (20 spilled); the fp32 form at T = 4 was the slowest choice at 129 k vertices (65 us
                           // against 55 for the bf16x3 form at T = 3: profiles/r6_kernel_stats_C4_one_in_flight.csv)
#endif
#ifndef LN_CONV_LDS_E
#define LN_CONV_LDS_E 16  // filter extents up to 2 (d + 1) + 1 with d <= 6 keep their neighbour ids in LDS
#endif
// Waves per SIMD of the bf16x3 per-slot kernel by gathered width (registers: 2 x V/4 row quarters + the staged bank slice + 4 NT
// accumulators; LDS: 36-48 KB bank slice + 4 KB ids per workgroup): 3 up to 128 channels (<= 168 registers, 3 x 52 KB of LDS), 2 above
// (192 / 256 channels need 174 / 220 registers: at 3 they spill, 1.77 ms instead of 0.63 at 256 x 256).  Measured at 46 k rows, 2 -> 3
// waves: 64 x 64 37.7 -> 32.1 us, 96 x 96 2 x 48.4 -> 2 x 40.8, 128 x 128 129 -> 122, 32 -> 64 20.7 -> 16.1.
#define LN_CONV_B3_WAVES(V) ((V) <= 128 ? 3 : 2)
// Split of the per-slot convolution over the filter slots: 1 (no split) while the vertex tiles alone fill the chip.
#ifndef LN_CONV_SPLIT_TILES
#define LN_CONV_SPLIT_TILES 512  // workgroups aimed at (two per CU)
#endif
#ifndef LN_CONV_WIDE_SPLIT_MIN_V
#define LN_CONV_WIDE_SPLIT_MIN_V 128
#endif
#ifndef LN_CONV_B3_MIN_ROWS
#define LN_CONV_B3_MIN_ROWS 4096
#endif
#ifndef LN_GF_ROWS
#define LN_GF_ROWS 320   // lattice vertices per workgroup (one slab each)
#endif
#ifndef LN_GFB_SUB
#define LN_GFB_SUB 64
#endif
#ifndef LN_GFB_EG
#define LN_GFB_EG 3   // slots per workgroup: E = 9 as three groups (gridDim.y); the gradient rows are split three times instead of nine
#endif
#ifndef LN_GFB_W128F
#define LN_GFB_W128F 2  // waves across the filters of a 128 x 128 block: 4 x 2 waves (512 threads, 248 registers; measured 101 us at 46 k rows
                        // against 118 for 4 x 4 waves, whose 128-register budget spills 13 dwords, and 132 for 64 x 64 sub-blocks)
#endif
// rows per workgroup of the bf16x3 filter gradient: as few as fill the chip (>= 512 workgroups over chunks x slot groups x sub-blocks) while the
// slabs the chunks write (and k_reduce_slabs4 reads back) stay under LN_GFB_SLAB_BYTES; a multiple of the 64-row sub-tile
#define LN_GFB_SLAB_BYTES (24ll << 20)

constexpr int ln_cdiv(long long a, long long b) { return int((a + b - 1) / b); }

// ---- shape predicates ------------------------------------------------------------------------------------------------------------
// gathered channel counts the per-slot kernels are instantiated for
constexpr bool ln_conv_per_slot_v(int V) {
    return V == 8 || V == 16 || V == 32 || V == 48 || V == 64 || V == 96 || V == 128 || V == 192 || V == 256;
}
// 16-row per-slot kernels: output columns go out in chunks of 16 * NT, NT in {8, 4, 2, 1}; the per-slot filter slice V x 16 NT must
// fit LDS, so any nr_filters that is a multiple of 16 runs on the matrix cores
constexpr int ln_conv_nt_max(int V) { return (V * 16 * 8 * 4 <= 32 * 1024) ? 8 : ((V * 16 * 4 * 4 <= 48 * 1024) ? 4 : 2); }
constexpr bool ln_conv_chunk_fits(int V, int NT) { return (NT == 8 || NT == 4 || NT == 2 || NT == 1) && NT <= ln_conv_nt_max(V); }
// 256 gathered channels x 32 columns spills in the bf16x3 form: those lattices take 16 columns per workgroup
constexpr bool ln_conv_chunk_b3_spills(int V, int NT) { return V >= 256 && NT > 1; }
// the chunk has a bf16x3 kernel (three bf16 planes of the slice in LDS); without one, a chunk takes the fp32 kernel even on a
// bf16x3 lattice (192 channels x 64 columns)
constexpr bool ln_conv_chunk_b3(int V, int NT) { return V % 32 == 0 && V * 16 * NT * 6 <= 64 * 1024 && !ln_conv_chunk_b3_spills(V, NT); }
// Sub-tiles per workgroup of the bf16x3 per-slot kernel: 3 (one 768-thread workgroup per CU) where the kernel runs at three waves per
// SIMD and there are at least as many such workgroups as CUs.
constexpr bool ln_conv_b3_three_subtiles(int V) { return LN_CONV_B3_WAVES(V) == 3; }
constexpr int ln_conv_b3_subtiles(int V, int m, int chunks) {
    return ln_conv_b3_three_subtiles(V) && (long long)ln_cdiv(m, 192) * chunks >= LN_BWD_CUS * 3 / 4 ? 3 : 1;
}
// wide form (both operands by LDS-DMA, 32-row MFMA tiles, every output column in one pass over the gathered rows): built for every
// multiple of 32 channels, taken from 96 gathered channels on (below, the 16-row kernels' gathers are as fast: 64 x 64 27 vs 29 us at
// 46 k rows).  Column chunks of 32 * NT, NT in {4, 3, 2, 1}; the kernel's shape follows from NT:
//   NT 4 -> 2 tiles per wave, column-split pairs, 6 row tiles;  3 -> 3 tiles, 4 row tiles;  2 -> 1 tile, pairs, 6;  1 -> 1 tile, 4.
constexpr bool ln_conv_wide_built(int V, int NT) { return V % 32 == 0 && NT >= 1 && NT <= 4; }
constexpr bool ln_conv_wide_shape(int V, int F) { return V % 32 == 0 && V >= 96 && F % 32 == 0; }
constexpr int ln_conv_r32_ntw(int NT) { return NT == 4 ? 2 : (NT == 3 ? 3 : 1); }
constexpr int ln_conv_r32_ch(int NT) { return NT % 2 == 0 ? 2 : 1; }
constexpr int ln_conv_r32_rt(int NT) { return NT % 2 == 0 ? 6 : 4; }
constexpr int LN_CONV_R32SK_RT = 6;  // row tiles of the split-K pairs (96-column chunks)
// small-filter fast path (whole bank in LDS, k_conv_mfma_full<V, F / 16, 9>): V x F up to 1024 over V in {8, 16, 32}, F / 16 a power of two
constexpr bool ln_conv_full_shape(int V, int F) {
    return (V == 8 || V == 16 || V == 32) && (F == 16 || F == 32 || F == 64 || F == 128) && V * F <= 1024;
}
// what the size queries take for the small-filter path when they leave the bank out.  (Wider than ln_conv_full_shape by one shape,
// 32 -> 48 at E = 9: its query reports no bank although the per-slot form runs; kept, the queries' results are part of the ABI.)
constexpr bool ln_conv_small_filter(int E, int V, int F) { return E == 9 && (size_t)E * V * F * 4 <= 64 * 1024 && V <= 32; }
constexpr bool ln_bwd_fused_shape(int E, int V, int F) { return E == 9 && V == 32 && F == 32; }

// 64-vertex sub-tiles per workgroup (1..4) of the fused backward and of k_conv_forward_b3.  The cost model is that of a chip the
// launch has to itself: there a workgroup takes a whole CU (the T = 3 fused backward holds 3 waves per SIMD of 152 registers and
// 126 KB of LDS), so the launch runs in rounds of 256 workgroups and a round costs about T + 1: the T with the cheapest
// rounds(T) * (T + 1) wins, larger T on ties (fewer slabs) — one round at C3 (T = 3; a 257th workgroup would run after all the
// others: twice the time), 3 rounds of T = 3 at 129 k vertices.  It does NOT hold while the caller keeps several scans in flight
// (`overlapped`, LN_CONV_OVERLAPPED): then the issue slots a whole-CU workgroup leaves idle are what the other scans' kernels are
// short of, and the bf16x3 forms take the narrow row-looping shape below instead.
// Shape measured at C3, four scans in flight: (T, C) = (2, 2) +1.7 %, (1, 3) -4.2 % against the whole-CU T = 3.
constexpr int LN_CONV_OVL_T = 2;  // narrow form under LN_CONV_OVERLAPPED: 256 * T threads ...
constexpr int LN_CONV_OVL_C = 2;  // ... that walk C consecutive chunks of 64 * T rows behind ONE bank staging, and write ONE slab
// the narrow form applies: bf16x3 kernels only, from the row count the bf16x3 forward is taken at up to TWO rounds of whole-CU
// workgroups (2 x 256 x 192 rows).  Measured with four scans in flight: +1.6 % at 46.5 k rows (C3), +4.2 % at ~90 k
// (C2, 16 clouds per step), -1.1 % at 129 k (C4: three rounds, between which the other scans get their turn anyway).
constexpr int LN_CONV_OVL_MAX_ROWS = 2 * 64 * LN_BWD_B3_MAX_T * LN_BWD_CUS;
constexpr bool ln_bwd_narrow(int m, bool b3_enabled, bool overlapped) {
    return overlapped && b3_enabled && m >= LN_CONV_B3_MIN_ROWS && m <= LN_CONV_OVL_MAX_ROWS;
}
constexpr int ln_bwd_subtiles(int m, bool b3_enabled, bool overlapped = false) {
    if (ln_bwd_narrow(m, b3_enabled, overlapped)) return LN_CONV_OVL_T;
    const int max_t = b3_enabled ? LN_BWD_B3_MAX_T : LN_BWD_MAX_SUBTILES;
    const int s = (m + 63) / 64;
    int best = 1, best_cost = 1 << 30;
    for (int t = 1; t <= max_t; ++t) {
        const int wgs = (s + t - 1) / t;
        const int cost = ((wgs + LN_BWD_CUS - 1) / LN_BWD_CUS) * (t + 1);  // (+ 1: the bank staging and the slab epilogue of a workgroup — at 129 k
                                                                           // vertices T = 2 / 3 run 4 / 3 rounds and measure 884 / 940 Mpoints/s)
        if (cost <= best_cost) {
            best = t;
            best_cost = cost;
        }
    }
    return best;
}
// chunks of 64 * T rows a workgroup walks (1: every form but the narrow one)
constexpr int ln_bwd_chunks(int m, bool b3_enabled, bool overlapped = false) { return ln_bwd_narrow(m, b3_enabled, overlapped) ? LN_CONV_OVL_C : 1; }
// workgroups = slabs of the fused backward.  64 * T * C >= 192 >= 64 * (the T of the whole-CU model), so the narrow form never
// writes more slabs than the form it replaces and the workspace queries (ln_gf_query) cover both.
static_assert(LN_CONV_OVL_T * LN_CONV_OVL_C >= LN_BWD_B3_MAX_T, "the narrow form would write more slabs than the workspace queries report");
constexpr int ln_bwd_workgroups(int m, bool b3_enabled, bool overlapped = false) {
    return ln_cdiv(m, 64 * ln_bwd_subtiles(m, b3_enabled, overlapped) * ln_bwd_chunks(m, b3_enabled, overlapped));
}

// ---- layout of the per-slot form: what the size queries report ------------------------------------------------------------------
// bf16x3 path: channel counts that are multiples of 32, lattices large enough to be matrix-bound; bytes of the filter bank split
// into three bf16 parts (0: fp32 path)
constexpr size_t ln_conv_bank_bytes(int m, int E, int V, int F, bool b3_enabled) {
    if (V % 32 != 0 || F % 16 != 0 || m < LN_CONV_B3_MIN_ROWS || E > LN_CONV_LDS_E || !b3_enabled) return 0;
    return (((size_t)E * V * F * 3 * sizeof(unsigned short)) + 255) & ~size_t(255);
}
constexpr int ln_conv_slots_per_split(int V, int m, int E, int F) {
    if (!ln_conv_per_slot_v(V)) return E;
    const long long tiles = (long long)ln_cdiv(m, 64) * ln_cdiv(F, 16 * ln_conv_nt_max(V));
    if (tiles * 2 > LN_CONV_SPLIT_TILES || E < 2) return E;
    int nsplit = int((LN_CONV_SPLIT_TILES + tiles - 1) / tiles);
    if (nsplit > E) nsplit = E;
    return (E + nsplit - 1) / nsplit;  // slots per workgroup
}
// Slot split of the WIDE form on mid-size lattices (0 / 1: not taken), from 128 gathered channels on where the 192-row workgroups of
// the unsplit wide form would fill less than half the chip.
// Measured at 11.4 k rows (level 2 of the SemanticKITTI network; tools/conv_time.py --coarse 1, us per call incl. bank split and
// partial sum): 128 -> 128 46.9 -> 35.7, 256 -> 256 296 -> 109, 192 -> 192 191 -> 76, 256 -> 128 157 -> 55, 128 -> 64 32.2 -> 26.3.
constexpr bool ln_conv_wide_fills_chip(int m, int F) { return (long long)ln_cdiv(m, 192) * ln_cdiv(F, 128) >= LN_BWD_CUS / 2; }
constexpr int ln_conv_wide_split(int V, int m, int E, int F, bool have_bank) {
    if (!have_bank || !ln_conv_per_slot_v(V) || V % 32 != 0 || V < LN_CONV_WIDE_SPLIT_MIN_V || F % 32 != 0 || E < 3 || m < LN_CONV_B3_MIN_ROWS)
        return 0;
    if (ln_conv_wide_fills_chip(m, F)) return 0;  // the unsplit wide form already runs
    // workgroups of the widest launch: the 128-column chunks go out together, a narrower rest as a launch of its own
    const long long wgs = (long long)ln_cdiv(m, 192) * (F >= 128 ? F / 128 : 1);
    // rounds of one workgroup per CU x slots walked per workgroup; the smallest split among the cheapest (fewer partial slabs)
    int best = 1;
    long long best_cost = 1ll << 60;
    for (int n = 2; n <= E; ++n) {
        const long long cost = ((wgs * n + LN_BWD_CUS - 1) / LN_BWD_CUS) * ((E + n - 1) / n);
        if (cost < best_cost) {
            best = n;
            best_cost = cost;
        }
    }
    return best;
}
struct LnConvLayout {
    size_t bank_bytes;  // split filter bank at the front of the workspace (0: fp32 path)
    int wide_split;     // > 1: the wide form with its slots split
    int nsplit, e_per;  // partial slabs [nsplit][m][F] behind the bank, slots per split
};
// `have_bank`: the bank has room in the workspace on offer (the size queries: always)
constexpr LnConvLayout ln_conv_layout(int m, int E, int V, int F, bool b3_enabled, bool have_bank) {
    LnConvLayout l = {ln_conv_bank_bytes(m, E, V, F, b3_enabled), 0, 1, ln_conv_slots_per_split(V, m, E, F)};
    l.wide_split = ln_conv_wide_split(V, m, E, F, l.bank_bytes > 0 && have_bank);
    if (l.wide_split > 1) l.e_per = (E + l.wide_split - 1) / l.wide_split;
    l.nsplit = (E + l.e_per - 1) / l.e_per;
    return l;
}
constexpr size_t ln_conv_slab_bytes(int nsplit, int m, int F) { return nsplit > 1 ? (size_t)nsplit * m * F * sizeof(float) : 0; }
// ln_conv_bank_workspace_bytes / ln_conv_forward_workspace_bytes
constexpr size_t ln_conv_bank_query(int m, int E, int V, int F, bool b3_enabled) {
    if (m <= 0 || F % 16 != 0 || ln_conv_small_filter(E, V, F)) return 0;
    return ln_conv_bank_bytes(m, E, V, F, b3_enabled);
}
constexpr size_t ln_conv_forward_query(int m, int E, int V, int F, bool b3_enabled) {
    if (m <= 0 || F % 16 != 0) return 256;
    return ln_conv_bank_query(m, E, V, F, b3_enabled) + ln_conv_slab_bytes(ln_conv_layout(m, E, V, F, b3_enabled, true).nsplit, m, F) + 256;
}

// ---- the forward plan --------------------------------------------------------------------------------------------------------------
enum LnConvKernel : uint8_t {
    LN_K_FORWARD_B3,    // k_conv_forward_b3<t>: the V = F = 32, E = 9 forward on the bf16 matrix cores
    LN_K_FULL,          // k_conv_mfma_full<V, nt, 9, FLIP, WT>: small filter, whole bank in LDS
    LN_K_SPLIT_BANK32,  // k_conv_split_bank32<V, nt, WT>: bank of `cnt` wide chunks of 32 nt columns
    LN_K_ROWS32,        // k_conv_rows32_b3<V, r32_ntw(nt), r32_ch(nt), r32_rt(nt), FLIP>
    LN_K_ROWS32SK,      // k_conv_rows32sk_b3<V, nt, LN_CONV_R32SK_RT, FLIP>
    LN_K_SPLIT_BANK,    // k_conv_split_bank<V, nt, WT>: bank of `cnt` chunks of 16 nt columns
    LN_K_MFMA_B3,       // k_conv_mfma_b3<V, nt, FLIP, t>
    LN_K_MFMA,          // k_conv_mfma<V, nt, FLIP, WT>
    LN_K_SUM_PARTIALS,  // ln_k_sum_partials: out = sum of the nsplit slabs
    LN_K_GENERIC,       // k_conv_generic: any shape, one thread per output element
};
struct LnConvLaunch {
    uint8_t kernel;     // LnConvKernel
    uint8_t nt, t;      // template arguments (see LnConvKernel)
    uint8_t c;          // LN_K_FORWARD_B3: chunks of 64 t rows per workgroup (1 elsewhere)
    bool carries_sum;   // a bank split whose extra workgroups [split_x, grid[0]) add the caller's pending slabs
    int grid[3], block;
    int f_off, cols;    // output columns [f_off, f_off + cols) (conv and bank-split launches)
    int split_x;        // bank split: workgroups of a plane that split
    size_t bank_off;    // bf16 elements from the start of the bank
    size_t bank_elems;  // ... and how many this launch writes or reads
};
#define LN_CONV_MAX_LAUNCHES 10  // 16-row form: 4 chunk sizes x (split + conv) + the sum; wide form: 2 x 2 + 1
struct LnConvPlanIn {
    int m, E, V, F;                                    // rows, filter extent, gathered channels, output columns
    bool flip, wt;                                     // LN_CONV_FLIP_NEIGHBOURS, LN_CONV_TRANSPOSED_FILTER
    bool b3_enabled;                                   // bf16x3 path on (LN_CONV_EXACT_F32 unset)
    bool values_aligned, filter_aligned;               // 16 bytes
    bool ws_aligned;                                   // workspace present and 256-byte aligned
    size_t ws_bytes;
    bool bank_ready;                                   // LN_CONV_BANK_READY: no bank-split launches
    int riding_total;                                  // elements of a slab sum waiting for a bank split to ride in (0: none)
    bool overlapped = false;                           // LN_CONV_OVERLAPPED: the caller keeps several scans in flight (speed hint)
};
struct LnConvPlan {
    size_t bank_bytes, slab_bytes;  // workspace layout in use: [bank][nsplit slabs]; their sum never exceeds the workspace offered
    int nsplit, e_per;
    bool sum_left;                  // a slab sum was waiting and no launch carries it: the caller launches it
    int n;
    LnConvLaunch launch[LN_CONV_MAX_LAUNCHES];
};

inline LnConvLaunch* ln_plan_add(LnConvPlan& p, LnConvKernel k, int nt, int t, int gx, int gy, int gz, int block, int f_off, int cols) {
    LnConvLaunch& l = p.launch[p.n++];
    l = LnConvLaunch{uint8_t(k), uint8_t(nt), uint8_t(t), 1, false, {gx, gy, gz}, block, f_off, cols, 0, 0, 0};
    return &l;
}

inline LnConvPlan ln_conv_plan(const LnConvPlanIn& in) {
    const int m = in.m, E = in.E, V = in.V, F = in.F;
    LnConvPlan p = {};
    p.nsplit = 1;
    p.e_per = E;
    p.sum_left = in.riding_total > 0;
    if (E == 9 && in.filter_aligned) {  // d = 3 small-filter fast path
        if (!in.flip && !in.wt && V == 32 && F == 32 && m >= LN_CONV_B3_MIN_ROWS && in.b3_enabled && in.values_aligned) {
            const int bt = ln_bwd_subtiles(m, true, in.overlapped), t = bt < 3 ? bt : 3, c = ln_bwd_chunks(m, true, in.overlapped);
            ln_plan_add(p, LN_K_FORWARD_B3, 2, t, ln_cdiv(m, 64 * t * c), 1, 1, 256 * t, 0, F)->c = uint8_t(c);
            return p;
        }
        if (ln_conv_full_shape(V, F)) {
            ln_plan_add(p, LN_K_FULL, F / 16, 1, ln_cdiv(m, 64), 1, 1, 256, 0, F);
            return p;
        }
    }
    if (!(F % 16 == 0 && in.values_aligned && in.filter_aligned && ln_conv_per_slot_v(V))) {
        ln_plan_add(p, LN_K_GENERIC, 0, 0, ln_cdiv((long long)m * F, 256), 1, 1, 256, 0, F);
        return p;
    }
    // workspace: [filter bank split into three bf16 parts (bf16x3 path)] [partial slabs of the slot split]
    const size_t bank_bytes = ln_conv_bank_bytes(m, E, V, F, in.b3_enabled);
    const bool b3 = bank_bytes > 0 && in.ws_aligned && in.ws_bytes >= bank_bytes;
    // Mid-size lattices with wide rows (coarse levels of a U-net: 5-30 k rows x 128+ channels): too few 192-row workgroups for the wide
    // form, and the 16-row kernels re-gather every row once per column chunk.  There the wide form runs with the slots split over
    // gridDim.z (its workgroups then fill the chip) and the partial sums are added by the launch behind it.
    const LnConvLayout lay = ln_conv_layout(m, E, V, F, in.b3_enabled, b3);
    p.bank_bytes = b3 ? bank_bytes : 0;
    p.nsplit = lay.nsplit;
    p.e_per = lay.e_per;
    if (p.nsplit > 1 && (!in.ws_aligned || in.ws_bytes - p.bank_bytes < ln_conv_slab_bytes(p.nsplit, m, F))) {
        p.e_per = E;  // no room for the partial slabs: one workgroup walks all slots
        p.nsplit = 1;
    }
    p.slab_bytes = ln_conv_slab_bytes(p.nsplit, m, F);
    const int nsplit = p.nsplit;
    int f_off = 0;
    size_t bank_off = 0;
    // every bank split but the first of a call: the pending slab sum rides in the first
    auto split = [&](LnConvKernel k, int nt, int cnt, int cols_per_chunk) {
        if (in.bank_ready) return;
        const int sx = ln_cdiv(V * cols_per_chunk, 256);
        LnConvLaunch* l = ln_plan_add(p, k, nt, 1, sx, E, cnt, 256, f_off, cnt * cols_per_chunk);
        l->split_x = sx;
        l->bank_off = bank_off;
        l->bank_elems = (size_t)E * cnt * V * cols_per_chunk * 3;
        if (p.sum_left) {
            l->carries_sum = true;
            l->grid[0] += ln_cdiv(in.riding_total / 64, E * cnt);
            p.sum_left = false;
        }
    };
    auto conv = [&](LnConvKernel k, int nt, int t, int rows, int block, int cnt, int cols_per_chunk, bool banked) {
        LnConvLaunch* l = ln_plan_add(p, k, nt, t, ln_cdiv(m, rows), cnt, nsplit, block, f_off, cnt * cols_per_chunk);
        if (banked) {
            l->bank_off = bank_off;
            l->bank_elems = (size_t)E * cnt * V * cols_per_chunk * 3;
            bank_off += l->bank_elems;
        }
        f_off += cnt * cols_per_chunk;
    };
    // wide form: while the 192-row workgroups alone fill half the chip, or with the slots split.  Column chunks of 128, then one
    // narrower chunk
    if (b3 && ln_conv_wide_shape(V, F) && ((lay.wide_split > 1 && nsplit > 1) || (nsplit == 1 && ln_conv_wide_fills_chip(m, F)))) {
        // 96 columns (three tiles: no even split of the columns over a pair of waves) take the split-K pairs: 96 -> 96 62.5 -> 54.1 us,
        // 128 -> 96 80.7 -> 69.1 us at 46.5 k rows; at 128 / 64 columns the column-split pairs are faster (80 vs 85, 50.6 vs 52 us:
        // the pair's partial sums cost a pass through LDS at the end)
        const bool rest_sk = F % 128 == 96;
        for (int nt = 4; nt >= 1; --nt) {
            const int cnt = (F - f_off) / (32 * nt);
            if (cnt == 0) continue;
            const bool sk = rest_sk && nt == 3;
            const int rt = sk ? LN_CONV_R32SK_RT : ln_conv_r32_rt(nt);
            split(LN_K_SPLIT_BANK32, nt, cnt, 32 * nt);
            conv(sk ? LN_K_ROWS32SK : LN_K_ROWS32, nt, 1, 32 * rt, sk ? 128 * rt : 64 * rt * ln_conv_r32_ch(nt), cnt, 32 * nt, true);
        }
    }
    // 16-row form: all chunks of the widest size go out as ONE launch (gridDim.y = their count), then at most one launch per narrower size
    for (int nt = 8; nt >= 1; nt >>= 1) {
        if (!ln_conv_chunk_fits(V, nt) || (b3 && ln_conv_chunk_b3_spills(V, nt))) continue;
        const int cnt = (F - f_off) / (16 * nt);
        if (cnt == 0) continue;
        if (b3 && ln_conv_chunk_b3(V, nt)) {
            split(LN_K_SPLIT_BANK, nt, cnt, 16 * nt);
            const int t = ln_conv_b3_subtiles(V, m, cnt * nsplit);
            conv(LN_K_MFMA_B3, nt, t, 64 * t, 256 * t, cnt, 16 * nt, true);
        } else {
            conv(LN_K_MFMA, nt, 1, 64, 256, cnt, 16 * nt, false);
        }
    }
    if (nsplit > 1) ln_plan_add(p, LN_K_SUM_PARTIALS, 0, 0, ln_cdiv((long long)m * F / 4, 256), 1, 1, 256, 0, F);
    return p;
}

// ---- filter gradient and ln_conv_backward -------------------------------------------------------------------------------------------
// Any multiple of 16 in both dimensions: the [V, F] block of a slot is covered by sub-blocks of {64, 32, 16} x {64, 32, 16}.
constexpr bool ln_gf_mfma_supported(int V, int F) { return V % 16 == 0 && F % 16 == 0; }
// block of the bf16x3 form, in channels x filters (0: none divides the shape)
struct LnGfBlock {
    int vs, fs;
};
constexpr LnGfBlock ln_gfb_block(int V, int F) {
    // (whole faces of 128 x 64, 64 x 128 and 96 x 96 on 4 x 2 / 2 x 4 / 3 x 2 waves measured the same as their 64 x 64 / 32 x 96
    // sub-blocks — 65 vs 66 us, 71 vs 71 us at 46 k rows —, and 96 x 96 on 2 x 2 waves spills: only 128 x 128 takes the whole face)
    constexpr int cand[7][2] = {{128, 128}, {64, 64}, {32, 96}, {96, 32}, {64, 32}, {32, 64}, {32, 32}};
    for (int k = 0; k < 7; ++k)
        if (V % cand[k][0] == 0 && F % cand[k][1] == 0) return LnGfBlock{cand[k][0], cand[k][1]};
    return LnGfBlock{0, 0};
}
// waves over the channels / the filters of a block (k_grad_filter_b3<vs / 16, fs / 16, 9, WV, WF>)
constexpr int ln_gfb_wv(int vs, int fs) { return vs == 128 && fs == 128 ? 4 : 2; }
constexpr int ln_gfb_wf(int vs, int fs) { return vs == 128 && fs == 128 ? LN_GFB_W128F : 2; }
constexpr int ln_gfb_rows(int m, int E, int V, int F) {
    const LnGfBlock b = ln_gfb_block(V, F);
    if (E != 9 || b.vs == 0) return 0;  // (the kernel is instantiated for E = 9: d = 3)
    const long long z = (long long)(V / b.vs) * (F / b.fs) * (E / LN_GFB_EG);  // workgroups per row chunk
    const long long slab = (long long)E * V * F * 4;
    const bool one_per_cu = b.vs * b.fs > 64 * 96;                          // blocks on more than eight waves take a whole CU
    long long chunks = ((one_per_cu ? 256 : 512) + z - 1) / z;              // (else two workgroups per CU) ...
    const long long budget = one_per_cu ? 2 * LN_GFB_SLAB_BYTES : LN_GFB_SLAB_BYTES;
    const long long cap = budget / slab > 0 ? budget / slab : 1;
    if (chunks > cap) chunks = cap;                                         // ... unless the slabs would cost more than the products
    long long rows = ((m + chunks - 1) / chunks + LN_GFB_SUB - 1) / LN_GFB_SUB * LN_GFB_SUB;
    if (rows < LN_GFB_SUB) rows = LN_GFB_SUB;
    return int(rows);
}
// ln_conv_grad_filter_workspace_bytes: one [E, V, F] slab per row chunk, whichever form runs; the fused backward of a same-lattice
// convolution (ln_conv_backward) has its own chunking
constexpr size_t ln_gf_query(int m, int E, int V, int F, bool b3_enabled) {
    if (!ln_gf_mfma_supported(V, F) || m <= 0) return 256;
    int chunks = ln_cdiv(m, LN_GF_ROWS);
    if (ln_bwd_fused_shape(E, V, F)) {  // with and without LN_CONV_OVERLAPPED: one workspace size serves both
        if (ln_bwd_workgroups(m, b3_enabled, false) > chunks) chunks = ln_bwd_workgroups(m, b3_enabled, false);
        if (ln_bwd_workgroups(m, b3_enabled, true) > chunks) chunks = ln_bwd_workgroups(m, b3_enabled, true);
    }
    const int rows_b3 = ln_gfb_rows(m, E, V, F);
    if (rows_b3 > 0 && ln_cdiv(m, rows_b3) > chunks) chunks = ln_cdiv(m, rows_b3);
    return (size_t)chunks * E * V * F * sizeof(float) + 256;
}
constexpr size_t ln_round256(size_t b) { return (b + 255) & ~size_t(255); }
// Both backward calls lay their workspace out as [filter gradient's slabs, rounded to 256][workspace of the value-gradient
// convolution]: the split point, read by the queries below and by the calls themselves
constexpr size_t ln_bwd_gf_bytes(int m, int E, int V, int F, bool b3_enabled) { return ln_round256(ln_gf_query(m, E, V, F, b3_enabled)); }
// ln_linear_backward_workspace_bytes: [filter gradient's slabs][workspace of the grad_x convolution]
constexpr size_t ln_linear_backward_query(int rows, int cin, int cout, bool b3_enabled) {
    return ln_bwd_gf_bytes(rows, 1, cout, cin, b3_enabled) + ln_conv_forward_query(rows, 1, cout, cin, b3_enabled) + 256;
}
// ln_conv_backward_workspace_bytes: [filter gradient's slabs][workspace of the value-gradient convolution over (mn, E, F -> V)]; the
// second part (and the rounding in front of it) only where that convolution takes a bank or splits its slots.  (The byte counts are
// part of the ABI: what hosts allocated before this query existed.)
constexpr size_t ln_conv_backward_query(int mq, int mn, int E, int V, int F, bool b3_enabled) {
    const size_t conv = ln_conv_forward_query(mn, E, F, V, b3_enabled);
    return conv > 256 ? ln_bwd_gf_bytes(mq, E, V, F, b3_enabled) + conv : ln_gf_query(mq, E, V, F, b3_enabled);
}

enum LnGfForm : uint8_t {
    LN_GF_GENERIC,  // k_grad_filter_generic straight into grad_filter: no slabs, no sum
    LN_GF_B3,       // k_grad_filter_b3<vs / 16, fs / 16, 9, wv, wf>: bf16 matrix cores, gradient rows split once for all nine slots
    LN_GF_F32,      // k_grad_filter_mfma<tile, tile>: uniform tiling (both dimensions multiples of the widest tile that divides
                    // them), ONE launch, gridDim.z = sub-blocks
};
struct LnGfPlan {
    uint8_t form;
    int vs, fs, wv, wf;   // LN_GF_B3: block and its waves
    int tile;             // LN_GF_F32: 4, 2 or 1
    int rows, chunks;     // rows per workgroup, slabs written
    int grid[3], block;
    size_t lds;           // dynamic LDS bytes
};
constexpr LnGfPlan ln_gf_plan(int m, int E, int V, int F, bool b3_enabled) {
    LnGfPlan p = {};
    p.block = 256;
    if (!ln_gf_mfma_supported(V, F)) {
        p.form = LN_GF_GENERIC;
        p.grid[0] = ln_cdiv((long long)E * V * F, 256);
        p.grid[1] = p.grid[2] = 1;
        return p;
    }
    const LnGfBlock b = ln_gfb_block(V, F);
    if (E == 9 && m >= LN_CONV_B3_MIN_ROWS && b3_enabled && b.vs > 0) {
        p.form = LN_GF_B3;
        p.vs = b.vs, p.fs = b.fs, p.wv = ln_gfb_wv(b.vs, b.fs), p.wf = ln_gfb_wf(b.vs, b.fs);
        p.rows = ln_gfb_rows(m, E, V, F);
        p.chunks = ln_cdiv(m, p.rows);
        p.grid[0] = p.chunks, p.grid[1] = E / LN_GFB_EG, p.grid[2] = (V / b.vs) * (F / b.fs);
        p.block = 64 * p.wv * p.wf;
        p.lds = (size_t)3 * LN_GFB_SUB * ((b.vs + 16) + (b.fs + 16)) * sizeof(unsigned short);
        return p;
    }
    p.form = LN_GF_F32;
    p.tile = (V % 64 == 0 && F % 64 == 0) ? 4 : ((V % 32 == 0 && F % 32 == 0) ? 2 : 1);
    p.rows = LN_GF_ROWS;
    p.chunks = ln_cdiv(m, LN_GF_ROWS);
    p.grid[0] = p.chunks, p.grid[1] = E, p.grid[2] = (V / (16 * p.tile)) * (F / (16 * p.tile));
    return p;
}

enum LnBwdForm : uint8_t {
    LN_BWD_FUSED_B3,   // k_conv_backward_fused_b3<t>: same lattice on both sides, one gather per (vertex, slot) serves both gradients
    LN_BWD_FUSED_F32,  // k_conv_backward_fused<32, 32, 9, t>
    LN_BWD_FULL_SUM,   // filter-gradient partials, then k_conv_mfma_full<.., true, true> whose extra workgroups sum the slabs
    LN_BWD_TWO_CALLS,  // ln_conv_grad_filter, then ln_conv_forward_ws (a bank split of the latter may carry the slab sum)
};
struct LnBwdPlanIn {
    int mq, mn, E, val_dim, nr_filters;
    bool same_list;    // nbr_q == nbr_n
    bool buffers;      // every pointer of the call is non-null
    size_t ws_bytes;   // (0 without a workspace)
    bool aligned;      // values, grad_out and filter: 16 bytes
    bool b3_enabled;
    bool overlapped = false;  // LN_CONV_OVERLAPPED
};
struct LnBwdPlan {
    uint8_t form;
    int t;               // fused forms: sub-tiles
    int c;               // LN_BWD_FUSED_B3: chunks of 64 t rows per workgroup (1 elsewhere)
    int grid, block;
    int conv_blocks;     // LN_BWD_FULL_SUM: workgroups of the convolution in front of the summing ones
};
constexpr LnBwdPlan ln_conv_backward_plan(const LnBwdPlanIn& in) {
    LnBwdPlan p = {LN_BWD_TWO_CALLS, 0, 1, 0, 256, 0};
    if (!(in.E == 9 && in.mq > 0 && in.mn > 0 && ln_gf_mfma_supported(in.val_dim, in.nr_filters) && in.buffers && in.ws_bytes > 0 &&
          in.ws_bytes >= ln_gf_query(in.mq, in.E, in.val_dim, in.nr_filters, in.b3_enabled) && in.aligned))
        return p;
    if (in.same_list && in.mq == in.mn && ln_bwd_fused_shape(in.E, in.val_dim, in.nr_filters)) {
        p.t = ln_bwd_subtiles(in.mn, in.b3_enabled, in.overlapped);
        p.c = ln_bwd_chunks(in.mn, in.b3_enabled, in.overlapped);
        p.form = in.b3_enabled && p.t <= LN_BWD_B3_MAX_T ? LN_BWD_FUSED_B3 : LN_BWD_FUSED_F32;
        p.grid = ln_bwd_workgroups(in.mn, in.b3_enabled, in.overlapped);
        p.block = 256 * p.t;
    } else if (ln_conv_full_shape(in.nr_filters, in.val_dim)) {  // roles in the value-gradient convolution: nr_filters channels in
        p.form = LN_BWD_FULL_SUM;
        p.conv_blocks = ln_cdiv(in.mn, 64);
        p.grid = p.conv_blocks + ln_cdiv((long long)in.E * in.val_dim * in.nr_filters, 16);
    }
    return p;
}
