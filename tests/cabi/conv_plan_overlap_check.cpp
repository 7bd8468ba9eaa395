// Host-only check of the LN_CONV_OVERLAPPED side of the convolution plans (lattice_net_amd/csrc/ln_conv_plan.h, the only project
// header included); built and run by tests/test_conv_plan_overlapped.py.  For every row count on the command line, at V = F = 32, E = 9
// with the bf16x3 path on:
//   `U m ...`  the plan WITHOUT the flag, field by field (forward launch, backward plan, the three size queries): the test compares these
//              lines with tests/golden/conv_plan_unflagged.txt, recorded before the flag existed;
//   `SHAPE T C min_rows max_rows`  the narrow instance and the row counts it is taken at;
//   and, checked here, WITH the flag: the workgroups cover the rows, the slabs are no more than without the flag, the workspace
//   query covers them, and the forward and the backward agree on the shape.
// Compiled with -DLN_PLAN_HAS_NO_FLAG it prints the U lines alone from a header that has no flag (how the golden file was made).
#include "ln_conv_plan.h"

#include <stdio.h>
#include <stdlib.h>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s (line %d): m %d\n", #cond, __LINE__, g_m);     \
            exit(1);                                                         \
        }                                                                    \
    } while (0)
static int g_m = 0;

int main(int argc, char** argv) {
    const int E = 9, V = 32, F = 32;
    for (int a = 1; a < argc; ++a) {
        const int m = g_m = atoi(argv[a]);
        LnConvPlanIn in = {};
        in.m = m, in.E = E, in.V = V, in.F = F;
        in.b3_enabled = in.values_aligned = in.filter_aligned = in.ws_aligned = true;
        in.ws_bytes = ln_conv_forward_query(m, E, V, F, true);
        const LnConvPlan p = ln_conv_plan(in);
        LnBwdPlanIn bin = {};
        bin.mq = bin.mn = m, bin.E = E, bin.val_dim = V, bin.nr_filters = F;
        bin.same_list = bin.buffers = bin.aligned = bin.b3_enabled = true;
        bin.ws_bytes = ln_conv_backward_query(m, m, E, V, F, true);
        const LnBwdPlan b = ln_conv_backward_plan(bin);
        printf("U %d n %d bank %zu slab %zu nsplit %d e_per %d |", m, p.n, p.bank_bytes, p.slab_bytes, p.nsplit, p.e_per);
        for (int k = 0; k < p.n; ++k) {
            const LnConvLaunch& l = p.launch[k];
            printf(" k %d nt %d t %d grid %d %d %d block %d f_off %d cols %d", l.kernel, l.nt, l.t, l.grid[0], l.grid[1], l.grid[2], l.block, l.f_off,
                   l.cols);
        }
        printf(" | bwd %d t %d grid %d block %d conv_blocks %d | q %zu %zu %zu\n", b.form, b.t, b.grid, b.block, b.conv_blocks,
               ln_conv_forward_query(m, E, V, F, true), ln_gf_query(m, E, V, F, true), ln_conv_backward_query(m, m, E, V, F, true));
#ifndef LN_PLAN_HAS_NO_FLAG
        for (int k = 0; k < p.n; ++k) CHECK(p.launch[k].c == 1);
        CHECK(b.c == 1);
        in.overlapped = bin.overlapped = true;
        const LnConvPlan po = ln_conv_plan(in);
        const LnBwdPlan bo = ln_conv_backward_plan(bin);
        CHECK(po.n == p.n && po.launch[0].kernel == p.launch[0].kernel && bo.form == b.form);
        if (po.launch[0].kernel == LN_K_FORWARD_B3) {
            const LnConvLaunch& l = po.launch[0];
            CHECK(l.c >= 1 && l.t >= 1 && l.t <= 3 && l.block == 256 * l.t && l.grid[1] == 1 && l.grid[2] == 1);
            CHECK((long long)l.grid[0] * l.c * 64 * l.t >= m && (long long)(l.grid[0] - 1) * l.c * 64 * l.t < m);
            CHECK(l.c == bo.c && l.t == bo.t && l.grid[0] == bo.grid);  // one shape for both directions
            CHECK(l.c > 1 || (l.t == p.launch[0].t && l.grid[0] == p.launch[0].grid[0]));
        }
        if (bo.form == LN_BWD_FUSED_B3) {
            CHECK(bo.c >= 1 && bo.t >= 1 && bo.t <= LN_BWD_B3_MAX_T && bo.block == 256 * bo.t);
            CHECK((long long)bo.grid * bo.c * 64 * bo.t >= m && (long long)(bo.grid - 1) * bo.c * 64 * bo.t < m);
            CHECK(bo.grid <= b.grid);  // slabs: one per workgroup, no more than without the flag
            CHECK(bo.grid == ln_bwd_workgroups(m, true, true) && b.grid == ln_bwd_workgroups(m, true, false));
            CHECK(bo.t == ln_bwd_subtiles(m, true, true) && bo.c == ln_bwd_chunks(m, true, true));
            // the workspace the host allocates (one query for both) holds every slab
            CHECK((size_t)bo.grid * E * V * F * sizeof(float) <= ln_gf_query(m, E, V, F, true));
            CHECK((size_t)bo.grid * E * V * F * sizeof(float) <= ln_conv_backward_query(m, m, E, V, F, true));
            CHECK(bo.c > 1 || (bo.t == b.t && bo.grid == b.grid));
        }
        // the fp32 fused form (LN_CONV_EXACT_F32) has no narrow shape
        CHECK(ln_bwd_chunks(m, false, true) == 1 && ln_bwd_subtiles(m, false, true) == ln_bwd_subtiles(m, false, false));
        printf("O %d t %d c %d grid %d\n", m, bo.t, bo.c, bo.grid);
#endif
    }
#ifndef LN_PLAN_HAS_NO_FLAG
    printf("SHAPE %d %d %d %d\n", LN_CONV_OVL_T, LN_CONV_OVL_C, LN_CONV_B3_MIN_ROWS, LN_CONV_OVL_MAX_ROWS);
#endif
    printf("OVERLAP PLANS OK\n");
    return 0;
}
