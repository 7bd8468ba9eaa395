// Host-only check of the convolution launch plans (lattice_net_amd/csrc/ln_conv_plan.h, the only project header included): built
// with the host compiler under -fsanitize=address,undefined by tests/test_conv_plan.py.  Walks a grid of shapes around every
// boundary of the dispatch and checks each plan's invariants; prints the size queries (`Q ...` lines) for the test to compare with
// the library's C ABI (the last three: ln_conv_backward's at mn = m, m / 2 + 1, 2 m).  argv[1]: 1 = bf16x3 path enabled (the library's default), 0 = LN_CONV_EXACT_F32=1.
// `conv_plan_check plan <b3> mq mn E V F [mq mn E V F ...]`: no grid walk; per shape, what ln_conv_forward_ws (mq rows, V -> F) and
// ln_conv_backward (two lists) launch with the queried workspace, aligned buffers and no bank left by an earlier call:
//   PLAN mq mn E V F / FWD <kernel> nt t nsplit cols e_per (one line per launch) / GF <form> vs fs tile / BWD <form> /
//   VG <kernel> nt t nsplit cols e_per (LN_BWD_TWO_CALLS: the value-gradient convolution over mn rows, F -> V, flipped, transposed bank)
#include "ln_conv_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long g_checked = 0;
static LnConvPlanIn g_in;
#define CHECK(cond)                                                                                                                  \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            printf("FAILED %s (line %d): m %d E %d V %d F %d flip %d wt %d b3 %d aligned %d %d ws %d %zu ready %d riding %d\n", #cond, __LINE__, \
                   g_in.m, g_in.E, g_in.V, g_in.F, g_in.flip, g_in.wt, g_in.b3_enabled, g_in.values_aligned, g_in.filter_aligned,    \
                   g_in.ws_aligned, g_in.ws_bytes, g_in.bank_ready, g_in.riding_total);                                              \
            exit(1);                                                                                                                 \
        }                                                                                                                            \
    } while (0)

static bool is_split(const LnConvLaunch& l) { return l.kernel == LN_K_SPLIT_BANK || l.kernel == LN_K_SPLIT_BANK32; }
static bool is_banked(const LnConvLaunch& l) { return l.kernel == LN_K_ROWS32 || l.kernel == LN_K_ROWS32SK || l.kernel == LN_K_MFMA_B3; }

static LnConvPlan check_plan(const LnConvPlanIn& in) {
    g_in = in;
    ++g_checked;
    const LnConvPlan p = ln_conv_plan(in);
    CHECK(p.n >= 1 && p.n <= LN_CONV_MAX_LAUNCHES);
    // layout: inside the workspace on offer; nothing at all without a usable one
    if (!in.ws_aligned) CHECK(p.bank_bytes == 0 && p.slab_bytes == 0 && p.nsplit == 1);
    else CHECK(p.bank_bytes + p.slab_bytes <= in.ws_bytes);
    CHECK(p.nsplit >= 1 && p.nsplit <= in.E && p.e_per >= 1 && (long long)p.nsplit * p.e_per >= in.E && (p.nsplit - 1) * p.e_per < in.E);
    CHECK(p.slab_bytes == (p.nsplit > 1 ? (size_t)p.nsplit * in.m * in.F * 4 : 0));
    int col = 0, carriers = 0, sums = 0;
    size_t bank_end = 0;
    const LnConvLaunch* pending_split = nullptr;
    for (int k = 0; k < p.n; ++k) {
        const LnConvLaunch& l = p.launch[k];
        for (int d = 0; d < 3; ++d) CHECK(l.grid[d] >= 1 && (d == 0 || l.grid[d] <= 65535));
        CHECK(l.block >= 64 && l.block <= 1024 && l.block % 64 == 0);
        if (l.kernel == LN_K_SUM_PARTIALS) {
            CHECK(k == p.n - 1 && p.nsplit > 1 && (long long)l.grid[0] * 256 * 4 >= (long long)in.m * in.F);
            ++sums;
            continue;
        }
        if (is_split(l)) {  // writes exactly the bank region the next launch reads, for the same columns
            CHECK(!in.bank_ready && !pending_split && k + 1 < p.n && l.grid[1] == in.E);
            CHECK(l.split_x >= 1 && (long long)l.split_x * 256 >= (long long)in.V * l.cols / l.grid[2]);
            if (l.carries_sum) {
                ++carriers;
                CHECK(in.riding_total > 0 && (long long)(l.grid[0] - l.split_x) * l.grid[1] * l.grid[2] >= in.riding_total / 64);
            } else {
                CHECK(l.grid[0] == l.split_x);
            }
            pending_split = &l;
            continue;
        }
        CHECK(!l.carries_sum);
        CHECK(l.f_off == col && l.cols >= 1);  // the columns, in order, once
        col += l.cols;
        if (is_banked(l)) {
            CHECK(p.bank_bytes > 0 && l.bank_off == bank_end && l.bank_elems == (size_t)in.E * in.V * l.cols * 3);
            bank_end = l.bank_off + l.bank_elems;
            CHECK(bank_end * 2 <= p.bank_bytes);
            CHECK(in.bank_ready || (pending_split && pending_split->bank_off == l.bank_off && pending_split->bank_elems == l.bank_elems &&
                                    pending_split->f_off == l.f_off && pending_split->cols == l.cols));
        } else {
            CHECK(!pending_split && l.bank_elems == 0);
        }
        pending_split = nullptr;
        if (l.kernel == LN_K_FORWARD_B3 || l.kernel == LN_K_FULL || l.kernel == LN_K_GENERIC) CHECK(p.n == 1 && p.nsplit == 1 && p.bank_bytes == 0);
        else CHECK(l.grid[2] == p.nsplit && l.grid[1] * (l.cols / l.grid[1]) == l.cols);
        if (l.kernel == LN_K_FORWARD_B3) CHECK(l.t >= 1 && l.t <= 3 && l.block == 256 * l.t && (long long)l.grid[0] * 64 * l.t >= in.m);
        if (l.kernel == LN_K_FULL) CHECK(ln_conv_full_shape(in.V, in.F) && l.nt * 16 == in.F);
        if (l.kernel == LN_K_MFMA_B3) CHECK(ln_conv_chunk_fits(in.V, l.nt) && ln_conv_chunk_b3(in.V, l.nt) && (l.t == 1 || (l.t == 3 && ln_conv_b3_three_subtiles(in.V))));
        if (l.kernel == LN_K_MFMA) CHECK(ln_conv_chunk_fits(in.V, l.nt));
        if (l.kernel == LN_K_ROWS32 || l.kernel == LN_K_ROWS32SK) CHECK(ln_conv_wide_built(in.V, l.nt) && (l.kernel == LN_K_ROWS32 || l.nt == 3));
    }
    CHECK(col == in.F && !pending_split);
    CHECK(sums == (p.nsplit > 1 ? 1 : 0));
    CHECK(carriers <= 1 && p.sum_left == (in.riding_total > 0 && carriers == 0));
    return p;
}

static void print_launches(const char* tag, const LnConvPlan& p) {
    static const char* const names[] = {"LN_K_FORWARD_B3", "LN_K_FULL", "LN_K_SPLIT_BANK32", "LN_K_ROWS32", "LN_K_ROWS32SK", "LN_K_SPLIT_BANK",
                                        "LN_K_MFMA_B3", "LN_K_MFMA", "LN_K_SUM_PARTIALS", "LN_K_GENERIC"};
    for (int k = 0; k < p.n; ++k)
        printf("%s %s %d %d %d %d %d\n", tag, names[p.launch[k].kernel], p.launch[k].nt, p.launch[k].t, p.nsplit, p.launch[k].cols, p.e_per);
}

static int print_plans(int argc, char** argv) {
    if (argc < 8 || (argc - 3) % 5 != 0) {
        printf("usage: conv_plan_check plan <b3> mq mn E V F [mq mn E V F ...]\n");
        return 2;
    }
    const bool b3 = argv[2][0] == '1';
    static const char* const gf_names[] = {"LN_GF_GENERIC", "LN_GF_B3", "LN_GF_F32"};
    static const char* const bwd_names[] = {"LN_BWD_FUSED_B3", "LN_BWD_FUSED_F32", "LN_BWD_FULL_SUM", "LN_BWD_TWO_CALLS"};
    for (int a = 3; a < argc; a += 5) {
        const int mq = atoi(argv[a]), mn = atoi(argv[a + 1]), E = atoi(argv[a + 2]), V = atoi(argv[a + 3]), F = atoi(argv[a + 4]);
        if (mq < 1 || mn < 1 || E < 1 || V < 1 || F < 1) return 2;
        printf("PLAN %d %d %d %d %d\n", mq, mn, E, V, F);
        print_launches("FWD", check_plan(LnConvPlanIn{mq, E, V, F, false, false, b3, true, true, true, ln_conv_forward_query(mq, E, V, F, b3), false, 0}));
        const LnGfPlan g = ln_gf_plan(mq, E, V, F, b3);
        printf("GF %s %d %d %d\n", gf_names[g.form], g.vs, g.fs, g.tile);
        // ln_conv_backward inside exactly its own query: the filter gradient's slabs in front, the value-gradient convolution's workspace behind
        const size_t bq = ln_conv_backward_query(mq, mn, E, V, F, b3), gfb = ln_bwd_gf_bytes(mq, E, V, F, b3);
        const LnBwdPlan bp = ln_conv_backward_plan(LnBwdPlanIn{mq, mn, E, V, F, false, true, bq, true, b3});
        printf("BWD %s\n", bwd_names[bp.form]);
        if (bp.form != LN_BWD_TWO_CALLS) continue;
        const int total = E * V * F;  // the filter gradient's slab sum waits for a bank split to ride in (ln_conv_grad_filter_impl)
        print_launches("VG", check_plan(LnConvPlanIn{mn, E, F, V, true, true, b3, true, true, bq > gfb, bq > gfb ? bq - gfb : 0, false,
                                                     g.form != LN_GF_GENERIC && total % 64 == 0 ? total : 0}));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "plan") == 0) return print_plans(argc, argv);
    const bool b3 = argc < 2 || argv[1][0] == '1';
    const int ms[] = {1, 64, 65, 4095, 4096, 4500, 11400, 16384, 16385, 32768, 32769, 46500, 128000, 400000};
    const int es[] = {1, 7, 9, 11, 16, 17, 27};
    const int cs[] = {1, 5, 8, 16, 32, 48, 64, 80, 96, 128, 160, 192, 224, 256, 320};
    for (int m : ms)
        for (int E : es)
            for (int V : cs)
                for (int F : cs) {
                    const size_t q = ln_conv_forward_query(m, E, V, F, b3);
                    const int mns[3] = {m, m / 2 + 1, 2 * m};  // rows of the neighbour side of a backward whose query side has m
                    printf("Q %d %d %d %d %zu %zu %zu %zu %zu %zu %zu\n", m, E, V, F, q, ln_conv_bank_query(m, E, V, F, b3), ln_gf_query(m, E, V, F, b3),
                           E == 1 ? ln_linear_backward_query(m, F, V, b3) : (size_t)0, ln_conv_backward_query(m, mns[0], E, V, F, b3),
                           ln_conv_backward_query(m, mns[1], E, V, F, b3), ln_conv_backward_query(m, mns[2], E, V, F, b3));
                    for (int flags = 0; flags < 8; ++flags)
                        for (int riding = 0; riding <= 1; ++riding) {
                            LnConvPlanIn in = {m, E, V, F, (flags & 1) != 0, (flags & 2) != 0, b3, true, true, true, ~size_t(0) >> 1, (flags & 4) != 0,
                                               riding ? E * V * F / 64 * 64 : 0};
                            const LnConvPlan full = check_plan(in);  // unlimited workspace: the layout the size query reports
                            const size_t need = full.bank_bytes + full.slab_bytes;
                            CHECK(need + 256 <= q || (ln_conv_small_filter(E, V, F) && need - full.bank_bytes + 256 <= q));
                            if (full.launch[0].kernel != LN_K_FORWARD_B3 && full.launch[0].kernel != LN_K_FULL && full.launch[0].kernel != LN_K_GENERIC &&
                                !ln_conv_small_filter(E, V, F))
                                CHECK(need + 256 == q);
                            in.ws_bytes = q;  // what the query says is enough for the same plan
                            if (!ln_conv_small_filter(E, V, F)) CHECK(check_plan(in).nsplit == full.nsplit && check_plan(in).bank_bytes == full.bank_bytes);
                            else check_plan(in);
                            if (need > 0) {  // one byte short of the layout: the slot split goes, every column is still covered
                                in.ws_bytes = need - 1;
                                const LnConvPlan p1 = check_plan(in);
                                CHECK(p1.nsplit == 1 || full.nsplit == 1);
                            }
                            if (full.bank_bytes > 0) {  // one byte short of the bank: fp32 path
                                in.ws_bytes = full.bank_bytes - 1;
                                CHECK(check_plan(in).bank_bytes == 0);
                            }
                            in.ws_bytes = q;
                            in.ws_aligned = false;  // absent or misaligned workspace
                            check_plan(in);
                            in.ws_aligned = true;
                            in.values_aligned = false;
                            check_plan(in);
                            in.values_aligned = true;
                            in.filter_aligned = false;
                            check_plan(in);
                        }
                    // filter gradient and the backward's form
                    g_in = LnConvPlanIn{m, E, V, F, false, false, b3, true, true, true, 0, false, 0};
                    const LnGfPlan g = ln_gf_plan(m, E, V, F, b3);
                    for (int d = 0; d < 3; ++d) CHECK(g.grid[d] >= 1 && (d == 0 || g.grid[d] <= 65535));
                    CHECK(g.block >= 64 && g.block <= 1024 && g.lds <= 160 * 1024);
                    if (g.form != LN_GF_GENERIC) {
                        CHECK(g.rows >= 1 && (long long)g.chunks * g.rows >= m && (size_t)g.chunks * E * V * F * 4 + 256 <= ln_gf_query(m, E, V, F, b3));
                        CHECK(g.form == LN_GF_B3 ? (V % g.vs == 0 && F % g.fs == 0 && g.block == 64 * g.wv * g.wf) : (V % (16 * g.tile) == 0 && F % (16 * g.tile) == 0));
                    }
                    for (int same = 0; same <= 1; ++same)
                        for (int ok = 0; ok <= 1; ++ok) {
                            const size_t gq = ln_gf_query(m, E, V, F, b3);
                            const LnBwdPlan bp = ln_conv_backward_plan(LnBwdPlanIn{m, m, E, V, F, same != 0, true, ok ? gq : gq - 1, true, b3});
                            CHECK(ok || bp.form == LN_BWD_TWO_CALLS);
                            if (bp.form == LN_BWD_FUSED_B3 || bp.form == LN_BWD_FUSED_F32) {
                                CHECK(same && bp.t >= 1 && bp.t <= (bp.form == LN_BWD_FUSED_B3 ? LN_BWD_B3_MAX_T : LN_BWD_MAX_SUBTILES) &&
                                      (long long)bp.grid * 64 * bp.t >= m && (size_t)bp.grid * E * V * F * 4 + 256 <= gq);
                            } else if (bp.form == LN_BWD_FULL_SUM) {
                                CHECK(ln_conv_full_shape(F, V) && bp.grid > bp.conv_blocks && (long long)bp.conv_blocks * 64 >= m);
                            }
                        }
                    // ln_conv_backward's own query: room for the filter gradient, the form of a generous workspace, and for the value-gradient
                    // convolution (mn rows, F channels in, V out, flipped, transposed bank) the layout its own query gives it
                    for (int mn : mns)
                        for (int same = 0; same <= 1; ++same) {
                            const size_t bq = ln_conv_backward_query(m, mn, E, V, F, b3), gfb = ln_bwd_gf_bytes(m, E, V, F, b3);
                            CHECK(bq >= ln_gf_query(m, E, V, F, b3));
                            const LnBwdPlan bp = ln_conv_backward_plan(LnBwdPlanIn{m, mn, E, V, F, same != 0, true, bq, true, b3});
                            CHECK(bp.form == ln_conv_backward_plan(LnBwdPlanIn{m, mn, E, V, F, same != 0, true, 16 * bq, true, b3}).form);
                            if (bp.form != LN_BWD_TWO_CALLS) continue;
                            LnConvPlanIn vin = {mn, E, F, V, true, true, b3, true, true, bq > gfb, bq > gfb ? bq - gfb : 0, false, E * V * F / 64 * 64};
                            const LnConvPlan behind = check_plan(vin);
                            vin.ws_aligned = true;
                            vin.ws_bytes = ln_conv_forward_query(mn, E, F, V, b3);
                            const LnConvPlan queried = check_plan(vin);
                            CHECK(behind.nsplit == queried.nsplit && behind.bank_bytes == queried.bank_bytes);
                        }
                }
    printf("PLANS OK %ld\n", g_checked);
    return 0;
}
