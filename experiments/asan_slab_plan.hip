// asan_slab_plan.hip — the HOST side of dcll_conv_lif_backward_slab and dcll_conv_lif_sequence_slabs under AddressSanitizer, on the
// CPU: a stand-alone program that walks the geometries of tests/bwd_slab_cases.py and tests/seq_slab_cases.py (and the bounds around
// them) through ws_make_plan — the slab rule, the column split, the small-batch lowering with the slab count, the layout the
// launcher checks before a launch — through ss_count / ss_rule / ss_layout — the tile rule with slabs, every tile's layout against
// the exported LDS formula — and through the exported predicates, and checks the invariants the kernels' indexing relies on.
// Nothing is launched and no GPU is needed.
//
//   cd snn_modulation_classification_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -o /tmp/asan_slab_plan ../../experiments/asan_slab_plan.hip dcll_bwd_wide.hip \
//         dcll_bwd_any.hip && ASAN_OPTIONS=detect_leaks=0 /tmp/asan_slab_plan
//
// (detect_leaks=0: the HIP runtime's start-up allocations are not this program's.)  Exit status 0 and "asan_slab_plan ok" = clean.
#include "../snn_modulation_classification_amd/csrc/dcll_bwd_slab.hip"
#include "../snn_modulation_classification_amd/csrc/dcll_seq_slab.hip"

#include <vector>

// what dcll_hip.hip provides to the library's translation units
static thread_local char err_buf[DCLL_ERR_LEN];
char *dcll_err_buf(void) { return err_buf; }
void dcll_trace_note(const char *) {}
// what dcll_seq_slab.hip hands layers of at most 64 channels to, and its weight permutation: never reached here (c_out > 64 only,
// nothing launched)
extern "C" int32_t dcll_conv_lif_sequence_tiles_plan(const dcll_conv_desc *, int32_t, int32_t, int32_t, int32_t *, int32_t *, int32_t *) { abort(); }
extern "C" int64_t dcll_conv_lif_sequence_tiles_lds(const dcll_conv_desc *, int32_t, int32_t) { abort(); }
extern "C" int64_t dcll_conv_lif_sequence_tiles_scratch(const dcll_conv_desc *, int32_t) { abort(); }
extern "C" int dcll_conv_lif_sequence_tiles(const dcll_conv_desc *, const uint32_t *, const float *, const float *, const float *, float *,
                                            float *, float *, uint32_t *, float *, float *, float *, int32_t, int32_t, int32_t, int32_t, void *) { abort(); }
int dcll_launch_seq_wprep(const dcll_conv_desc *, const float *, float *, int, hipStream_t, bool, const char *) { abort(); }

#define REQUIRE(cond)                                                                                        \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            fprintf(stderr, "asan_slab_plan: %s fails at line %d (c_in %d c_out %d k %dx%d plane %dx%d pad %d,%d nchunk %d)\n", #cond, \
                    __LINE__, d.c_in, d.c_out, d.kh, d.kw, d.h, d.w, d.pad_h, d.pad_w, nchunk);              \
            return 1;                                                                                        \
        }                                                                                                    \
    } while (0)

// one (descriptor, ty, tx) through the sequence plan: the plan's bounds partition the pooled plane, every tile's layout is the
// exported formula and inside the LDS, the weight room is inside the launch's LDS
static long seq_checked = 0, seq_served = 0;
static int walk_seq(dcll_conv_desc d, int ty, int tx)
{
    int nchunk = ty * 100 + tx;     // (for REQUIRE's message)
    int rc, NY = 0, NX = 0;
    ++seq_checked;
    const int n = ss_count(&d, ty, tx, "asan_slab_plan", &rc, &NY, &NX);
    if (!n) {
        REQUIRE(rc == DCLL_ERR_UNSUPPORTED || rc == DCLL_ERR_INVALID);
        REQUIRE(dcll_conv_lif_sequence_slabs_lds(&d, ty, tx) == 0);
        return 0;
    }
    ++seq_served;
    int ch, cw, ph, pw;
    conv_shape(&d, &ch, &cw, &ph, &pw);
    REQUIRE(n == NY * NX && NY >= 1 && NX >= 1 && NY <= ph && NX <= pw);
    std::vector<int32_t> by(NY + 1), bx(NX + 1);
    int32_t nn[2];
    REQUIRE(dcll_conv_lif_sequence_slabs_plan(&d, 3, ty, tx, nn, by.data(), bx.data()) == n && nn[0] == NY && nn[1] == NX);
    REQUIRE(by[0] == 0 && by[NY] == ph && bx[0] == 0 && bx[NX] == pw);
    long base = 0;
    int c_prev = 0;
    for (int ka = 0; ka < NY; ++ka) {
        const band_rows ry = band_plan(ka, NY, d.h, d.kh, d.pad_h, d.pool_h, ch, ph);
        REQUIRE(ry.P0 == by[ka] && ry.P1 == by[ka + 1] && ry.P1 > ry.P0 && ry.C0 == c_prev && ry.C1 >= ry.C0 && ry.I0 <= ry.I1 && ry.I1 <= d.h);
        c_prev = ry.C1;
        for (int kb = 0; kb < NX; ++kb) {
            const band_rows rx = band_plan(kb, NX, d.w, d.kw, d.pad_w, d.pool_w, cw, pw);
            const ss_lay L = ss_layout(ry, rx, d.c_in, d.kh, d.kw, d.refractory != 0);
            REQUIRE(L.end == ss_floats(&d, L.CR, L.CC, L.HR, L.HC) && L.o_e0 <= L.o_v && L.o_v <= L.o_arp && L.o_arp <= L.o_tau);
            // the first held input pixel and the last one lie inside a channel of img
            const int q0 = (ry.I0 + d.pad_h - ry.C0) * L.CB + rx.I0 + d.pad_w - rx.C0;
            REQUIRE(L.HR == 0 || L.HC == 0 || (q0 >= 0 && q0 + (L.HR - 1) * L.CB + L.HC - 1 < L.CHS));
            if (L.end > base) base = L.end;
        }
    }
    REQUIRE(c_prev == ch && base * 4 <= ANY_LDS_MAX && base * 4 == dcll_conv_lif_sequence_slabs_lds(&d, NY, NX));
    const int nsteps = (int)any_chain_steps(&d);
    for (long wg : {1L, 256L, 257L, 100000L}) {
        const int nwl = seq_weight_room(base, nsteps, SS_MT, wg);
        REQUIRE(nwl >= 0 && nwl <= nsteps && (base + (long)nwl * 64 * SS_MT) * 4 <= ANY_LDS_MAX);
    }
    REQUIRE(dcll_conv_lif_sequence_slabs_scratch(&d, 3) == (long)nsteps * 64 * ss_gmt(&d) + 2L * 3 * d.c_in * d.h * d.w);
    return 0;
}

static long checked = 0, served = 0;


static int walk(dcll_conv_desc d, int nchunk, long full_ldsf)
{
    ws_plan p;
    ++checked;
    const int rc = ws_make_plan(&d, nchunk, &p, "asan_slab_plan");
    if (rc != DCLL_OK) {
        REQUIRE(rc == DCLL_ERR_UNSUPPORTED || rc == DCLL_ERR_INVALID);
        REQUIRE(strlen(err_buf) > 0 && strlen(err_buf) < DCLL_ERR_LEN);
        REQUIRE(nchunk == 0);                       // (a served layer is served at every chunk count)
        return 0;
    }
    ++served;
    const ws_geom &g = p.g;
    const int rows = d.c_out < SLAB_ROWS ? d.c_out : SLAB_ROWS;
    REQUIRE(p.NS == slab_count(d.c_out) && p.NS >= 1 && p.NS <= SLAB_MAX);
    REQUIRE(g.TPW >= 1 && g.TPW <= WS_MAX_TPW && g.TPW <= g.NT && p.nsplit == (g.NT + g.TPW - 1) / g.TPW && p.nsplit <= 65535);
    REQUIRE(g.ldsf >= WS_RED_FLOATS && g.ldsf <= WS_LDS_MAX_FLOATS && (full_ldsf == 0 || g.ldsf <= full_ldsf));
    REQUIRE(g.o_g + (long)rows * g.GLD <= g.ldsf);
    REQUIRE(g.TPW <= 8 * p.NQ && (g.PS == 1 || (p.NQ == 1 && g.TPW * g.PS <= 8)));
    REQUIRE((p.NQ == 1 || p.NQ == 2 || p.NQ == 4) && (g.PS == 1 || g.PS == 2 || g.PS == 4 || g.PS == 8));
    // the kernel's reads: the last B operand of the last column tile's last tap at the last pixel pair, the last g float
    const int ch = g.CP / g.cw;
    for (int t0 = 0; t0 < g.NT; t0 += g.TPW) {
        const int t1 = t0 + g.TPW < g.NT ? t0 + g.TPW : g.NT;
        const int c0 = (t0 * 32) / g.KK, c1 = ((t1 * 32 < g.N ? t1 * 32 : g.N) - 1) / g.KK;
        const long img_last = (long)(c1 - c0) * g.CF + (long)(g.KK - 1) / g.kw * g.RF + (g.kw - 1) + 1 + (long)(ch - 1) * g.RF + (g.cwp - 2);
        REQUIRE(c1 >= c0 && c1 < d.c_in && img_last < g.o_g);
    }
    REQUIRE((long)(rows - 1) * g.GLD + 1 + 2L * (g.PP - 1) < (long)rows * g.GLD && 2L * g.PP <= g.GLD);
    return 0;
}

int main()
{
    // the slab rule: a partition of [0, c_out)
    for (int c_out = 1; c_out <= 300; ++c_out) {
        std::vector<int> owner(c_out, 0);
        for (int s = 0; s < slab_count(c_out); ++s) {
            if (slab_rows(s, c_out) < 1 || slab_rows(s, c_out) > SLAB_ROWS) return 2;
            for (int r = 0; r < slab_rows(s, c_out); ++r) ++owner.at(slab_first(s) + r);
        }
        for (int v : owner)
            if (v != 1) return 2;
    }
    const int couts[] = {1, 32, 33, 64, 65, 96, 97, 128, 129, 130, 200, 4096, 64 * 65535, 64 * 65535 + 1};
    const int cins[] = {1, 2, 3, 5, 7, 16, 24, 33, 64, 70};
    const int kernels[][2] = {{1, 1}, {2, 5}, {3, 3}, {4, 8}, {7, 7}, {9, 9}, {16, 16}, {8, 16}, {17, 3}};
    const int planes[][2] = {{1, 1}, {3, 3}, {4, 4}, {4, 8}, {3, 11}, {5, 7}, {3, 5}, {9, 8}, {16, 16}, {20, 20}, {157, 4}, {158, 4}};
    const int chunks[] = {1, 2, 3, 4, 5, 33, 63, 64, 85, 86, 127, 128, 255, 256};
    for (int c_out : couts)
        for (int c_in : cins)
            for (const auto &k : kernels)
                for (const auto &hw : planes)
                    for (int pad = 0; pad < 2; ++pad) {
                        dcll_conv_desc d;
                        memset(&d, 0, sizeof d);
                        d.c_in = c_in, d.c_out = c_out, d.h = hw[0], d.w = hw[1], d.kh = k[0], d.kw = k[1];
                        d.pad_h = pad ? k[0] / 2 : 0, d.pad_w = pad ? k[1] / 2 : 0;
                        d.pool_h = d.pool_w = 1, d.stride = d.dilation = d.groups = 1, d.target = 10;
                        if (walk(d, 0, 0)) return 1;
                        ws_plan full;
                        const bool ok = ws_make_plan(&d, 0, &full, "asan_slab_plan") == DCLL_OK;
                        const int64_t lds = dcll_conv_lif_backward_slab_lds(&d);
                        if (c_out > SLAB_ROWS && lds != (ok ? (int64_t)full.g.ldsf * 4 : 0)) return 3;
                        if (!ok) continue;
                        for (int n : chunks)
                            if (walk(d, n, full.g.ldsf)) return 1;
                    }
    // the sequence plan: the rule and explicit plans, refractory and plain, with pooling
    {
        const int scouts[] = {65, 96, 97, 128, 129, 200, 64 * 65535, 64 * 65535 + 1};
        const int scins[] = {1, 3, 41, 42, 64, 70, 128};
        const int splanes[][2] = {{3, 3}, {4, 4}, {4, 8}, {3, 11}, {6, 6}, {13, 11}, {16, 16}, {4, 40}, {16, 17}};
        const int sk[][2] = {{1, 1}, {2, 5}, {3, 3}, {7, 7}, {9, 9}, {16, 16}, {17, 3}};
        const int stiles[][2] = {{0, 0}, {1, 1}, {3, 1}, {1, 3}, {2, 2}, {4, 4}, {0, 2}, {2, 0}, {-1, 2}, {40, 40}};
        for (int c_out : scouts)
            for (int c_in : scins)
                for (const auto &k : sk)
                    for (const auto &hw : splanes)
                        for (int pool = 1; pool <= 3; ++pool)
                            for (int refr = 0; refr < 2; ++refr) {
                                dcll_conv_desc d;
                                memset(&d, 0, sizeof d);
                                d.c_in = c_in, d.c_out = c_out, d.h = hw[0], d.w = hw[1], d.kh = k[0], d.kw = k[1];
                                d.pad_h = k[0] / 2, d.pad_w = k[1] / 2, d.pool_h = pool, d.pool_w = pool == 3 ? 2 : pool;
                                d.stride = d.dilation = d.groups = 1, d.target = 10, d.refractory = refr;
                                if (check_desc(&d) != DCLL_OK) continue;
                                for (const auto &t : stiles)
                                    if (walk_seq(d, t[0], t[1])) return 5;
                            }
    }
    // refusals: a null descriptor, stride / dilation / groups
    if (dcll_conv_lif_backward_slab_lds(nullptr) != 0) return 4;
    dcll_conv_desc d;
    memset(&d, 0, sizeof d);
    d.c_in = 2, d.c_out = 96, d.h = d.w = 10, d.kh = d.kw = 3, d.pad_h = d.pad_w = 1, d.pool_h = d.pool_w = 1, d.target = 10;
    d.stride = 2, d.dilation = 1, d.groups = 1;
    if (dcll_conv_lif_backward_slab_lds(&d) != 0 || !strstr(err_buf, "plain convolutions only")) return 4;
    d.stride = 1, d.dilation = 2;
    if (dcll_conv_lif_backward_slab_lds(&d) != 0) return 4;
    d.dilation = 1, d.groups = 2;
    if (dcll_conv_lif_backward_slab_lds(&d) != 0) return 4;
    if (dcll_conv_lif_sequence_slabs_lds(nullptr, 0, 0) != 0 || dcll_conv_lif_sequence_slabs_plan(nullptr, 1, 0, 0, nullptr, nullptr, nullptr) != 0) return 4;
    printf("asan_slab_plan ok: %ld weight-gradient plans walked, %ld served; %ld sequence plans walked, %ld served\n", checked, served,
           seq_checked, seq_served);
    return 0;
}
