// Host-only check of the fp16 linear layer's launch plans (lattice_net_amd/csrc/ln_linear_f16_plan.h and, through it, the segment walk of
// ln_conv_f16_plan.h: the only project headers included): built with the host compiler under -fsanitize=address,undefined by
// tests/test_linear_f16_plan.py.  Walks a grid of shapes, row counts and pointer alignments around every boundary of the dispatch and
// checks each plan's invariants (restated below from the rules of the issue, not from the header), the slabs the workspace query
// counts, and the refusal rules; prints the workspace query (`Q rows cin cout bytes`) for the test to compare with the C ABI.
// `linear_f16_plan_check plan rows cin cout x_off [...]`: no grid walk; per case (byte offset of `x` from 16-byte alignment; every other
// array is aligned), what the two calls of tests/test_gpu_linear_f16.py launch:
//   PLAN rows cin cout x_off
//   FWD <form> kstep nt tiles_per_wg launches grid [nt:off ...]   ln_linear_forward_f16
//   GX  <form> kstep nt tiles_per_wg launches grid [nt:off ...]   the input gradient of ln_linear_backward_f16 (k = cout, n = cin)
//   GW  <form> launches chunks gridy [vt:ft:v_off:f_off ...]      its weight gradient (launches: without the slab sums)
#include "ln_linear_f16_plan.h"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static long g_checked = 0;
static long long g_rows;
static int g_k, g_n;
static unsigned g_low;
#define CHECK(cond)                                                                                                      \
    do {                                                                                                                 \
        if (!(cond)) {                                                                                                   \
            printf("FAILED %s (line %d): rows %lld k/cin %d n/cout %d low bits %u\n", #cond, __LINE__, g_rows, g_k, g_n, g_low); \
            exit(1);                                                                                                     \
        }                                                                                                                \
    } while (0)

static void note(long long rows, int k, int n, unsigned low) {
    g_rows = rows, g_k = k, g_n = n, g_low = low;
    ++g_checked;
}

static LnLin16Plan check_product(long long rows, int k, int n, unsigned low) {
    note(rows, k, n, low);
    const LnLin16Plan p = ln_lin16_plan(LnLin16In{rows, k, n, low});
    const bool mfma = k % 16 == 0 && n % 16 == 0 && k <= 256 && n <= 256 && low % 8 == 0;
    CHECK(p.block == 256 && p.n >= 1);
    if (p.form == LN_LIN16_MFMA) {
        CHECK(mfma);
        CHECK(p.kstep == (k % 32 == 0 ? 32 : 16) && k % p.kstep == 0);
        CHECK(p.cols16 * 16 == n);
        // rows: every tile of 64 belongs to one workgroup, no workgroup is empty, at most 512 workgroups
        const long long tiles = (rows + 63) / 64;
        CHECK(p.tiles_per_wg >= 1 && p.grid >= 1 && p.grid <= 512);
        CHECK((long long)p.grid * p.tiles_per_wg >= tiles && (long long)(p.grid - 1) * p.tiles_per_wg < tiles);
        CHECK(tiles > 512 || p.tiles_per_wg == 1);
        // columns [0, n) once, in order; every chunk's bank within 64 KB (two workgroups per CU), and ONE chunk wherever the whole bank is
        int col = 0;
        for (int c = 0; c < p.n; ++c) {
            const LnF16Seg s = ln_lin16_chunk(p, c);
            CHECK(s.off == col && (s.nt == 16 || s.nt == 8 || s.nt == 4 || s.nt == 2 || s.nt == 1));
            CHECK((size_t)k * 16 * s.nt * 2 <= 64 * 1024 && ln_lin16_bank_bytes(k, s.nt) == (size_t)k * 16 * s.nt * 2);
            col += 16 * s.nt;
        }
        CHECK(col == n && ln_lin16_chunk(p, p.n).nt == 0);
        if ((size_t)k * n * 2 <= 64 * 1024 && (n & (n - 1)) == 0) CHECK(p.n == 1);
        if ((size_t)k * n * 2 > 64 * 1024) CHECK(p.n >= 2);
    } else {
        CHECK(p.form == LN_LIN16_GENERIC && !mfma && p.n == 1 && p.work == rows * n);
        if (p.grid > 0) CHECK((long long)p.grid * 256 >= p.work && (long long)(p.grid - 1) * 256 < p.work);
        else CHECK((p.work + 255) / 256 > 0x7fffffffLL);
    }
    return p;
}

static LnLin16GwPlan check_gw(long long rows, int cin, int cout, bool bias, unsigned low) {
    note(rows, cin, cout, low);
    const LnLin16GwPlan p = ln_lin16_gw_plan(LnLin16GwIn{rows, cin, cout, bias, low});
    const bool mfma = cin % 16 == 0 && cout % 16 == 0 && cin <= 256 && cout <= 256 && low % 8 == 0;
    const long long chunks = (rows + 511) / 512;
    // the workspace is what the slabs need: one [cout, cin] and one [cout] fp32 slab per chunk, the bias slabs behind the weight slabs
    CHECK(ln_lin16_workspace_bytes(rows, cin, cout) == ((size_t)chunks * cout * cin + (size_t)chunks * cout) * 4 + 256);
    CHECK(ln_lin16_bias_slab_offset(rows, cin, cout) == (size_t)chunks * cout * cin);
    if (p.form == LN_LIN16_GW_UNSUPPORTED) {
        CHECK(!mfma && p.n == 0);
        return p;
    }
    CHECK(p.chunks == chunks && p.block == 256 && p.grid[0] == p.chunks && p.grid[2] == 1);
    if (p.form == LN_LIN16_GW_MFMA) {
        CHECK(mfma && p.grid[1] == 1 && p.n == p.nv * p.nf);
        static unsigned char cell[16][16];
        memset(cell, 0, sizeof(cell));
        int bias_tiles = 0;
        for (int k = 0; k < p.n; ++k) {
            const LnLin16GwTile t = ln_lin16_gw_tile(p, cin, cout, k);
            CHECK((t.vt == 4 || t.vt == 2 || t.vt == 1) && (t.ft == 4 || t.ft == 2 || t.ft == 1));
            CHECK(t.v_off % 16 == 0 && t.f_off % 16 == 0 && t.v_off + 16 * t.vt <= cout && t.f_off + 16 * t.ft <= cin);
            for (int a = 0; a < t.vt; ++a)
                for (int b = 0; b < t.ft; ++b) ++cell[t.v_off / 16 + a][t.f_off / 16 + b];
            if (t.f_off == 0) bias_tiles += t.vt;  // the launches that also sum the bias gradient
        }
        for (int a = 0; a < cout / 16; ++a)
            for (int b = 0; b < cin / 16; ++b) CHECK(cell[a][b] == 1);
        CHECK(bias_tiles == cout / 16);  // every output channel's bias gradient once
    } else {
        CHECK(p.form == LN_LIN16_GW_FALLBACK && !mfma && p.n == 1);
        const long long elems = (long long)cout * cin + cout;
        CHECK((long long)p.grid[1] * 256 >= elems && (long long)(p.grid[1] - 1) * 256 < elems && p.grid[1] <= 65535);
    }
    return p;
}

static void check_refusals() {
    note(0, 0, 0, 0);
    const int OK = 0, ARG = -1, WS = -4;
    // forward: sizes first, then the three required buffers at rows > 0
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{true, true, true, 5, 16, 16}) == OK);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{false, false, false, 0, 16, 16}) == OK);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{true, true, true, -1, 16, 16}) == ARG);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{true, true, true, 5, 0, 16}) == ARG);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{true, true, true, 5, 16, 0}) == ARG);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{true, true, true, 0, 16, -2}) == ARG);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{false, true, true, 5, 16, 16}) == ARG);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{true, false, true, 5, 16, 16}) == ARG);
    CHECK(ln_lin16_forward_refusal(LnLin16FwdArgs{true, true, false, 5, 16, 16}) == ARG);
    // backward
    const size_t q = ln_lin16_workspace_bytes(700, 24, 20);
    CHECK(q == ((size_t)2 * 24 * 20 + 2 * 20) * 4 + 256);
    auto bwd = [&](bool x, bool gy, bool w, bool gx, bool gw, bool ws, long long rows, int cin, int cout, size_t bytes) {
        return ln_lin16_backward_refusal(LnLin16BwdArgs{x, gy, w, gx, gw, ws, rows, cin, cout, bytes});
    };
    CHECK(bwd(true, true, true, true, true, true, 700, 24, 20, q) == OK);
    CHECK(bwd(true, true, false, false, true, true, 700, 24, 20, q) == OK);       // no grad_x: w is not read
    CHECK(bwd(true, true, true, true, true, true, 700, 24, 20, q - 1) == WS);
    CHECK(bwd(true, true, true, true, true, false, 700, 24, 20, q) == WS);
    CHECK(bwd(true, true, true, true, true, true, -1, 24, 20, q) == ARG);
    CHECK(bwd(true, true, true, true, true, true, 700, 0, 20, q) == ARG);
    CHECK(bwd(true, true, true, true, true, true, 700, 24, 0, q) == ARG);
    CHECK(bwd(true, true, true, true, false, true, 700, 24, 20, q) == ARG);
    CHECK(bwd(false, true, true, true, true, true, 700, 24, 20, q) == ARG);
    CHECK(bwd(true, false, true, true, true, true, 700, 24, 20, q) == ARG);
    CHECK(bwd(true, true, false, true, true, true, 700, 24, 20, q) == ARG);       // grad_x wanted, no w
    CHECK(bwd(false, false, false, false, false, true, 700, 24, 20, 0) == ARG);   // an argument error comes before the workspace
    CHECK(bwd(false, false, false, false, true, false, 0, 24, 20, 0) == OK);      // rows == 0: only grad_w is needed
    CHECK(bwd(false, false, false, false, false, false, 0, 24, 20, 0) == ARG);
    CHECK(ln_lin16_workspace_bytes(0, 64, 64) == 256 && ln_lin16_workspace_bytes(-3, 64, 64) == 256 && ln_lin16_workspace_bytes(5, 0, 64) == 256);
}

static int print_plans(int argc, char** argv) {
    if (argc < 6 || (argc - 2) % 4 != 0) {
        printf("usage: linear_f16_plan_check plan rows cin cout x_off [...]\n");
        return 2;
    }
    static const char* const names[] = {"MFMA", "GENERIC"};
    static const char* const gw_names[] = {"MFMA", "FALLBACK", "UNSUPPORTED"};
    for (int a = 2; a < argc; a += 4) {
        const int rows = atoi(argv[a]), cin = atoi(argv[a + 1]), cout = atoi(argv[a + 2]), xoff = atoi(argv[a + 3]);
        if (rows < 1 || cin < 1 || cout < 1 || xoff < 0 || xoff > 15) return 2;
        printf("PLAN %d %d %d %d\n", rows, cin, cout, xoff);
        for (int gx = 0; gx <= 1; ++gx) {
            const LnLin16Plan p = gx ? check_product(rows, cout, cin, 0) : check_product(rows, cin, cout, unsigned(xoff));
            printf("%s %s %d %d %d %d %d", gx ? "GX" : "FWD", names[p.form], p.kstep, p.nt, p.tiles_per_wg, p.n, p.grid);
            if (p.form == LN_LIN16_MFMA)
                for (int k = 0; k < p.n; ++k) printf(" %d:%d", ln_lin16_chunk(p, k).nt, ln_lin16_chunk(p, k).off);
            printf("\n");
        }
        const LnLin16GwPlan g = check_gw(rows, cin, cout, true, unsigned(xoff));
        printf("GW %s %d %d %d", gw_names[g.form], g.n, g.chunks, g.grid[1]);
        if (g.form == LN_LIN16_GW_MFMA)
            for (int k = 0; k < g.n; ++k) {
                const LnLin16GwTile t = ln_lin16_gw_tile(g, cin, cout, k);
                printf(" %d:%d:%d:%d", t.vt, t.ft, t.v_off, t.f_off);
            }
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "plan") == 0) return print_plans(argc, argv);
    // rows: the kernels' own tiles (16-row waves, 64-row tiles, 512-row slab chunks) and the 512 workgroups of 64 rows behind which a
    // workgroup walks a second and a third tile
    long long ms[48];
    int nm = 0;
    for (long long m : {1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1024, 1025, 1300, 46538}) ms[nm++] = m;
    for (int k = 1; k <= 3; ++k)
        for (int d = -1; d <= 1; ++d) ms[nm++] = 64LL * 512 * k + d;
    ms[nm++] = 2147483647LL;
    int cs[40], nc = 0;
    for (int c = 16; c <= 288; c += 16) cs[nc++] = c;
    for (int c : {1, 3, 4, 7, 20, 24, 130, 300, 5000}) cs[nc++] = c;
    const unsigned lows[] = {0, 2, 4, 8};
    for (int mi = 0; mi < nm; ++mi)
        for (int ki = 0; ki < nc; ++ki)
            for (int ni = 0; ni < nc; ++ni) {
                const long long m = ms[mi];
                const int cin = cs[ki], cout = cs[ni];
                if (m <= 0x7fffffff) printf("Q %lld %d %d %zu\n", m, cin, cout, ln_lin16_workspace_bytes(m, cin, cout));
                for (unsigned low : lows) {
                    const LnLin16Plan p = check_product(m, cin, cout, low);
                    // a matrix-core shape leaves the matrix cores only through a pointer
                    if (cin % 16 == 0 && cout % 16 == 0 && cin <= 256 && cout <= 256) CHECK((p.form == LN_LIN16_MFMA) == (low % 8 == 0));
                    for (int bias = 0; bias <= 1; ++bias) check_gw(m, cin, cout, bias != 0, low);
                }
            }
    // the widest chunk, read by hand: the whole of 256 columns up to a contraction length of 128, 128 columns beyond
    note(0, 0, 0, 0);
    CHECK(ln_lin16_nt_max(16) == 16 && ln_lin16_nt_max(128) == 16 && ln_lin16_nt_max(144) == 8 && ln_lin16_nt_max(256) == 8);
    check_refusals();
    printf("PLANS OK %ld\n", g_checked);
    return 0;
}
