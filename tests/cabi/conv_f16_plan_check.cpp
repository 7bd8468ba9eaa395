// Host-only check of the fp16 convolution's launch plans (lattice_net_amd/csrc/ln_conv_f16_plan.h, the only project header included):
// built with the host compiler under -fsanitize=address,undefined by tests/test_conv_f16_plan.py.  Walks a grid of shapes, row counts
// and pointer alignments around every boundary of the dispatch and checks each plan's invariants, among them that the chunk and tile
// lists are the ones the dispatch loops of ln_conv_f16.hip produced before the plan existed (restated below, on purpose, in their
// original form); prints the workspace query (`Q m E V F bytes`) for the test to compare with the library's C ABI.
// `conv_f16_plan_check plan mq mn E V F values_off grad_out_off [...]`: no grid walk; per case (byte offsets of the `values` and
// `grad_out` arrays from 16-byte alignment; the filter is aligned), what the three products of tests/test_gpu_conv_f16_forms.py launch:
//   PLAN mq mn E V F values_off grad_out_off
//   FWD <form> V nt t line kstep launches [nt:f_off ...]    ln_conv_forward_f16 over mq rows, V -> F, flags 0
//   VG  <form> V nt t line kstep launches [nt:f_off ...]    ... over mn rows, F -> V, flags 3, `grad_out` in the place of `values`
//   GF  <form> launches gridz lds [vt:ft:v_off:f_off ...]   ln_conv_grad_filter_f16 over mq rows (launches: without the slab sum)
#include "ln_conv_f16_plan.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long g_checked = 0;
static int g_m, g_E, g_V, g_F, g_flags;
static unsigned g_a, g_b;
#define CHECK(cond)                                                                                                                 \
    do {                                                                                                                            \
        if (!(cond)) {                                                                                                              \
            printf("FAILED %s (line %d): m %d E %d V %d F %d flags %d low bits %u %u\n", #cond, __LINE__, g_m, g_E, g_V, g_F, g_flags, g_a, g_b); \
            exit(1);                                                                                                                \
        }                                                                                                                           \
    } while (0)

static void note(int m, int E, int V, int F, int flags, unsigned a, unsigned b) {
    g_m = m, g_E = E, g_V = V, g_F = F, g_flags = flags, g_a = a, g_b = b;
    ++g_checked;
}

static bool in_32_64(int c) { return c == 32 || c == 64; }
static bool slot_v(int V) { return V == 16 || V == 32 || V == 64 || V == 96 || V == 128 || V == 256; }

// the column chunks of the per-slot forward as the dispatch loop of ln_conv_f16.hip walked them
static int old_chunks(int V, int F, int (*out)[2]) {
    const int nt_max = (V * 128 * 2 <= 32 * 1024) ? 8 : 4;
    int n = 0, f_off = 0;
    while (f_off < F) {
        const int left = (F - f_off) / 16;
        const int nt = (nt_max >= 8 && left >= 8) ? 8 : (left >= 4 ? 4 : (left >= 2 ? 2 : 1));
        out[n][0] = nt, out[n][1] = f_off;
        ++n;
        f_off += 16 * nt;
    }
    return n;
}

static LnF16FwdPlan check_forward(int m, int E, int V, int F, int flags, unsigned vlow, unsigned flow) {
    note(m, E, V, F, flags, vlow, flow);
    const LnF16FwdPlan p = ln_f16_forward_plan(LnF16FwdIn{m, E, V, F, flags, vlow, flow});
    const bool tiled = E == 9 && in_32_64(V) && in_32_64(F) && vlow % 16 == 0 && flow % 16 == 0;
    const bool slots = !tiled && F % 16 == 0 && vlow % 8 == 0 && slot_v(V);
    CHECK(p.flip == ((flags & 1) != 0) && p.wt == ((flags & 2) != 0));
    CHECK(p.n >= 1 && p.grid >= 1 && p.block >= 256 && p.block <= 1024);
    if (p.form == LN_F16_FWD_TILED) {
        CHECK(tiled && E == 9 && in_32_64(V) && in_32_64(F) && ((vlow | flow) & 15) == 0);
        CHECK(p.V == V && p.nt * 16 == F && p.n == 1 && p.line == (V == 64));
        CHECK(p.t >= 1 && p.t <= 4 && p.block == 256 * p.t);
        CHECK((long long)p.grid * 64 * p.t >= m && (long long)(p.grid - 1) * 64 * p.t < m);
        CHECK(p.lds == (size_t)9 * V * F * 2 + (V == 64 ? 16 * 2048 + 256 * 9 * 4 : 0) && p.lds <= 160 * 1024);
        CHECK(p.t == ln_f16_subtiles(m, p.lds));
    } else if (p.form == LN_F16_FWD_SLOTS) {
        CHECK(slots && p.V == V && p.block == 256 && (long long)p.grid * 64 >= m && (long long)(p.grid - 1) * 64 < m);
        CHECK(p.kstep == (V % 32 == 0 ? 32 : 16));
        int old[64][2];
        CHECK(F / 16 + 1 <= 64);
        const int n_old = old_chunks(V, F, old);
        CHECK(p.n == n_old);
        int col = 0;
        for (int k = 0; k < p.n; ++k) {
            const LnF16Seg c = ln_f16_chunk(p, k);
            CHECK(c.nt == old[k][0] && c.off == old[k][1]);
            CHECK(c.off == col && (c.nt == 8 || c.nt == 4 || c.nt == 2 || c.nt == 1));  // columns [0, F) once, in order
            CHECK(V != 256 || c.nt != 8);
            const size_t lds = (size_t)V * 16 * c.nt * 2;  // s_b of k_conv_mfma_f16<V, NT>
            CHECK(lds <= 32 * 1024 && ln_f16_per_slot_lds(V, c.nt) == lds);
            col += 16 * c.nt;
        }
        CHECK(col == F);
        CHECK(ln_f16_chunk(p, p.n).nt == 0);  // nothing behind the last chunk
    } else {
        CHECK(p.form == LN_F16_FWD_GENERIC && !tiled && !slots);
        CHECK(p.n == 1 && p.block == 256 && p.work == (long long)m * F && (long long)p.grid * 256 >= p.work && (long long)(p.grid - 1) * 256 < p.work);
    }
    return p;
}

static LnF16GfPlan check_gf(int m, int E, int V, int F, unsigned vlow, unsigned glow) {
    note(m, E, V, F, -1, vlow, glow);
    const LnF16GfPlan p = ln_f16_gf_plan(LnF16GfIn{m, E, V, F, vlow, glow});
    const bool mfma = V % 16 == 0 && F % 16 == 0 && vlow % 8 == 0 && glow % 8 == 0;
    const size_t lds = (size_t)32 * 4 * ((size_t)V + F);
    CHECK(p.chunks == (m + 511) / 512 && p.block == 256);
    CHECK(ln_f16_gf_workspace_bytes(m, E, V, F) == (size_t)p.chunks * E * V * F * 4 + 256);
    if (p.form == LN_F16_GF_MFMA) {
        CHECK(mfma && p.grid[0] == p.chunks && p.grid[1] == E && p.grid[2] == 1 && p.lds == 0 && p.n == p.nv * p.nf);
        // the tiles as the two nested loops of ln_conv_f16.hip walked them, and every 16 x 16 cell of V x F covered once
        static unsigned char cell[64][64];
        memset(cell, 0, sizeof(cell));
        CHECK(V / 16 <= 64 && F / 16 <= 64);
        int k = 0;
        for (int v_off = 0; v_off < V;) {
            const int vleft = (V - v_off) / 16;
            const int vt = vleft >= 4 ? 4 : (vleft >= 2 ? 2 : 1);
            for (int f_off = 0; f_off < F;) {
                const int fleft = (F - f_off) / 16;
                const int ft = fleft >= 4 ? 4 : (fleft >= 2 ? 2 : 1);
                CHECK(k < p.n);
                const LnF16GfTile t = ln_f16_gf_tile(p, V, F, k++);
                CHECK(t.vt == vt && t.ft == ft && t.v_off == v_off && t.f_off == f_off);
                CHECK(t.v_off + 16 * t.vt <= V && t.f_off + 16 * t.ft <= F);
                for (int a = 0; a < t.vt; ++a)
                    for (int b = 0; b < t.ft; ++b) ++cell[t.v_off / 16 + a][t.f_off / 16 + b];
                f_off += ft * 16;
            }
            v_off += vt * 16;
        }
        CHECK(k == p.n);
        for (int a = 0; a < V / 16; ++a)
            for (int b = 0; b < F / 16; ++b) CHECK(cell[a][b] == 1);
    } else if (p.form == LN_F16_GF_FALLBACK) {
        CHECK(!mfma && lds <= 64 * 1024 && p.lds == lds && p.n == 1);
        CHECK(p.grid[0] == p.chunks && p.grid[1] == E && p.grid[2] == int(((long long)V * F + 4095) / 4096) && p.grid[2] <= 65535);
    } else {
        CHECK(p.form == LN_F16_GF_UNSUPPORTED && !mfma && lds > 64 * 1024 && p.n == 0);
    }
    return p;
}

static int print_plans(int argc, char** argv) {
    if (argc < 9 || (argc - 2) % 7 != 0) {
        printf("usage: conv_f16_plan_check plan mq mn E V F values_off grad_out_off [...]\n");
        return 2;
    }
    static const char* const fwd_names[] = {"TILED", "SLOTS", "GENERIC"};
    static const char* const gf_names[] = {"MFMA", "FALLBACK", "UNSUPPORTED"};
    for (int a = 2; a < argc; a += 7) {
        const int mq = atoi(argv[a]), mn = atoi(argv[a + 1]), E = atoi(argv[a + 2]), V = atoi(argv[a + 3]), F = atoi(argv[a + 4]);
        const int voff = atoi(argv[a + 5]), goff = atoi(argv[a + 6]);
        if (mq < 1 || mn < 1 || E < 1 || V < 1 || F < 1 || voff < 0 || voff > 15 || goff < 0 || goff > 15) return 2;
        printf("PLAN %d %d %d %d %d %d %d\n", mq, mn, E, V, F, voff, goff);
        for (int vg = 0; vg <= 1; ++vg) {
            const LnF16FwdPlan p = vg ? check_forward(mn, E, F, V, 3, unsigned(goff), 0) : check_forward(mq, E, V, F, 0, unsigned(voff), 0);
            printf("%s %s %d %d %d %d %d %d", vg ? "VG" : "FWD", fwd_names[p.form], p.V, p.nt, p.t, int(p.line), p.kstep, p.n);
            if (p.form == LN_F16_FWD_SLOTS)
                for (int k = 0; k < p.n; ++k) printf(" %d:%d", ln_f16_chunk(p, k).nt, ln_f16_chunk(p, k).off);
            printf("\n");
        }
        const LnF16GfPlan g = check_gf(mq, E, V, F, unsigned(voff), unsigned(goff));
        printf("GF %s %d %d %zu", gf_names[g.form], g.n, g.grid[2], g.lds);
        if (g.form == LN_F16_GF_MFMA)
            for (int k = 0; k < g.n; ++k) {
                const LnF16GfTile t = ln_f16_gf_tile(g, V, F, k);
                printf(" %d:%d:%d:%d", t.vt, t.ft, t.v_off, t.f_off);
            }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "plan") == 0) return print_plans(argc, argv);
    // rows: the kernels' own tiles (64-row tiles, 512-row chunks of 64- and 32-row sub-tiles) and the rounds of 256 and 512 workgroups of
    // 64 T rows that choose the sub-tile count
    int ms[64], nm = 0;
    for (int m : {1, 31, 32, 33, 63, 64, 65, 511, 512, 513, 577, 4500}) ms[nm++] = m;
    for (int k = 1; k <= 4; ++k)
        for (int base : {64 * 256, 64 * 512})
            for (int d = -1; d <= 1; ++d) ms[nm++] = base * k + d;
    int cs[32], nc = 0;
    for (int c = 16; c <= 272; c += 16) cs[nc++] = c;
    for (int c : {1, 5, 24, 40, 60, 72, 100, 220, 300}) cs[nc++] = c;
    const int es[] = {1, 3, 5, 9, 15, 17};
    const unsigned lows[] = {0, 2, 4, 8};
    for (int mi = 0; mi < nm; ++mi)
        for (int E : es)
            for (int vi = 0; vi < nc; ++vi)
                for (int fi = 0; fi < nc; ++fi) {
                    const int m = ms[mi], V = cs[vi], F = cs[fi];
                    printf("Q %d %d %d %d %zu\n", m, E, V, F, ln_f16_gf_workspace_bytes(m, E, V, F));
                    int forms = 0;
                    for (unsigned vlow : lows)
                        for (unsigned flow : lows) {
                            const LnF16FwdPlan p0 = check_forward(m, E, V, F, 0, vlow, flow);
                            forms |= 1 << p0.form;
                            for (int flags = 1; flags < 4; ++flags) {  // the flags choose the template instance and nothing else
                                const LnF16FwdPlan p = check_forward(m, E, V, F, flags, vlow, flow);
                                CHECK(p.form == p0.form && p.n == p0.n && p.grid == p0.grid && p.block == p0.block && p.t == p0.t && p.nt == p0.nt);
                            }
                            check_gf(m, E, V, F, vlow, flow);  // (second pointer: grad_out)
                        }
                    // a shape with a matrix-core form leaves it for the generic one only through a pointer
                    if (F % 16 == 0 && slot_v(V)) CHECK(forms & ((1 << LN_F16_FWD_TILED) | (1 << LN_F16_FWD_SLOTS)));
                }
    // the sub-tile count, from the cost model read by hand: one workgroup per CU at 64 gathered channels (T = 1 up to 256 tiles, then 2,
    // 3 from 513 tiles, 4 from 769), two per CU at 32 (T = 2 / 3 / 4 from 513 / 1025 / 1537 tiles)
    note(0, 9, 0, 0, 0, 0, 0);
    for (int F : {32, 64}) {
        const size_t l64 = ln_f16_tiled_lds(64, F), l32 = ln_f16_tiled_lds(32, F);
        const int b64[4] = {1, 16385, 32769, 49153}, b32[4] = {1, 32769, 65537, 98305};
        for (int t = 1; t <= 4; ++t) {
            CHECK(ln_f16_subtiles(b64[t - 1], l64) == t && ln_f16_subtiles(b32[t - 1], l32) == t);
            if (t > 1) CHECK(ln_f16_subtiles(b64[t - 1] - 1, l64) == t - 1 && ln_f16_subtiles(b32[t - 1] - 1, l32) == t - 1);
        }
    }
    CHECK(ln_f16_gf_workspace_bytes(0, 9, 64, 64) == 256 && ln_f16_gf_workspace_bytes(-3, 9, 64, 64) == 256);
    printf("PLANS OK %ld\n", g_checked);
    return 0;
}
