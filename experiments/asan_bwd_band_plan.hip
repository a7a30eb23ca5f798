// asan_bwd_band_plan.hip — the HOST side of dcll_conv_lif_backward_bands under AddressSanitizer and UBSan, on the CPU: a stand-alone
// program that walks the geometries of tests/bwd_band_cases.py and the bounds around them (one row, column and channel more and
// less) through wb_make_plan — the band rule, every forced band count 0 .. ch + 1, every chunk count 1 .. 256 with its small-batch
// lowering — through the exported predicate and plan query, and through the invariants the launcher re-checks and the kernel's
// indexing relies on.  Nothing is launched and no GPU is needed.
//
//   cd snn_modulation_classification_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -o /tmp/asan_bwd_band_plan ../../experiments/asan_bwd_band_plan.hip dcll_bwd_slab.hip \
//         dcll_bwd_wide.hip dcll_bwd_any.hip && ASAN_OPTIONS=detect_leaks=0 /tmp/asan_bwd_band_plan
//
// (detect_leaks=0: the HIP runtime's start-up allocations are not this program's.)  Exit status 0 and "asan_bwd_band_plan ok" = clean.
#include "../snn_modulation_classification_amd/csrc/dcll_bwd_band.hip"

#include <vector>

// what dcll_hip.hip provides to the library's translation units
static thread_local char err_buf[DCLL_ERR_LEN];
char *dcll_err_buf(void) { return err_buf; }
void dcll_trace_note(const char *) {}

#define REQUIRE(cond)                                                                                                               \
    do {                                                                                                                            \
        if (!(cond)) {                                                                                                              \
            fprintf(stderr, "asan_bwd_band_plan: %s fails at line %d (c_in %d c_out %d k %dx%d plane %dx%d pad %d,%d bands %d nchunk %d)\n", \
                    #cond, __LINE__, d.c_in, d.c_out, d.kh, d.kw, d.h, d.w, d.pad_h, d.pad_w, bands, nchunk);                       \
            return 1;                                                                                                               \
        }                                                                                                                           \
    } while (0)

static long pairs = 0, served = 0, forwarded = 0, refused = 0;

// one (descriptor, bands, nchunk): the plan, the launcher's invariants, the kernel's reads and writes
static int walk(const dcll_conv_desc &d, int bands, int nchunk, const wb_plan *full)
{
    wb_plan p;
    const long B = 3;
    REQUIRE(wb_make_plan(&d, bands, B, nchunk, &p, "asan_bwd_band_plan") == DCLL_OK);       // (a served layer is served at every chunk count)
    const wb_geom &g = p.g;
    REQUIRE(wb_plan_ok(p));
    REQUIRE(g.TPW <= WB_MAX_TPW && g.TPW <= g.NT && p.nsplit == (g.NT + g.TPW - 1) / g.TPW);
    REQUIRE((p.NQ == 1 || p.NQ == 2 || p.NQ == 4) && (g.PS == 1 || g.PS == 2 || g.PS == 4 || g.PS == 8));
    REQUIRE(p.rows == (d.c_out < 32 * p.MT ? d.c_out : 32 * p.MT) && g.IR == g.RB + d.kh - 1 && g.CFB == g.IR * g.RF);
    if (full) {     // the lowering keeps the bands and never needs more LDS than the full launch
        REQUIRE(g.ldsf <= full->g.ldsf && g.RB == full->g.RB && g.NB == full->g.NB && g.TPW <= full->g.TPW);
        REQUIRE((int64_t)g.ldsf * 4 <= dcll_conv_lif_backward_bands_lds(&d, bands));
    }
    REQUIRE(bands == 0 ? (long)(g.NB - 1) * g.RB < g.ch : g.NB == bands);                    // (the rule leaves no empty band)
    // every workgroup's column range: its channels, the staging writes and the B-operand reads of a full band
    for (int t0 = 0; t0 < g.NT; t0 += g.TPW) {
        const int t1 = t0 + g.TPW < g.NT ? t0 + g.TPW : g.NT;
        const int c0 = (t0 * 32) / g.KK, c1 = ((t1 * 32 < g.N ? t1 * 32 : g.N) - 1) / g.KK;
        REQUIRE(c1 >= c0 && c1 < d.c_in);
        const long last_write = (long)(c1 - c0) * g.CFB + (long)(g.IR - 1) * g.RF + (d.w - 1) + d.pad_w;
        const long last_read = (long)(c1 - c0) * g.CFB + (long)(d.kh - 1) * g.RF + (d.kw - 1) + 1 + (long)(g.RB - 1) * g.RF + (g.cwp - 2);
        REQUIRE(last_write < g.o_g && last_read < g.o_g);
    }
    // the g rows: the last float of the last row of a full band, and the bias sum's range
    REQUIRE(g.o_g + (long)(p.rows - 1) * g.GLD + (long)g.RB * g.cwp <= g.ldsf && g.RB * g.cwp <= g.GLD && g.cwp == 2 * g.hp);
    REQUIRE(8L * p.MT * 16 * 64 <= g.ldsf);                                                 // the pixel-split pieces
    return 0;
}

static int walk_desc(dcll_conv_desc d)
{
    int nchunk = 0, bands = 0;
    if (check_desc(&d) != DCLL_OK) return 0;
    int ch, cw, ph, pw;
    conv_shape(&d, &ch, &cw, &ph, &pw);
    for (bands = -1; bands <= ch + 1; ++bands) {
        nchunk = 0;
        int32_t out[8];
        const int64_t lds = dcll_conv_lif_backward_bands_lds(&d, bands);
        const int prc = dcll_conv_lif_backward_bands_plan(&d, 3, bands, out);
        REQUIRE((lds > 0) == (prc == DCLL_OK) && lds <= ANY_LDS_MAX);
        if (dcll_bwd_band_forwards(&d, bands)) {
            ++pairs, ++forwarded;
            REQUIRE(lds == dcll_conv_lif_backward_slab_lds(&d));
            REQUIRE(prc != DCLL_OK || (out[0] == 1 && out[1] == ch && out[2] == 0 && out[7] == 3));
            continue;
        }
        wb_plan full;
        const int rc = wb_make_plan(&d, bands, 3, 0, &full, "asan_bwd_band_plan");
        if (rc != DCLL_OK) {
            ++pairs, ++refused;
            REQUIRE(rc == DCLL_ERR_UNSUPPORTED && lds == 0 && strlen(err_buf) > 0 && strlen(err_buf) < DCLL_ERR_LEN);
            REQUIRE(dcll_bwd_wgrad_band_check(&d, bands, "asan_bwd_band_plan") == rc);
            for (int i = 0; i < 8; ++i) REQUIRE(out[i] == 0);
            continue;
        }
        REQUIRE(bands >= 0 && bands <= ch && lds == (int64_t)full.g.ldsf * 4);
        if (walk(d, bands, 0, nullptr)) return 1;
        ++pairs, ++served;
        // the bands partition [0, ch) exactly once
        std::vector<int> owner(ch, 0);
        for (int k = 0; k < full.g.NB; ++k) {
            const int r0 = k * full.g.RB, rb = full.g.RB < ch - r0 ? full.g.RB : ch - r0;
            for (int r = 0; r < rb; ++r) ++owner.at(r0 + r);
        }
        for (int v : owner) REQUIRE(v == 1);
        // the exported plan: an unlimited scratch gives min(B NB, 256) chunks
        const long nc = 3L * full.g.NB < WB_MAX_CHUNKS ? 3L * full.g.NB : WB_MAX_CHUNKS;
        wb_plan q;
        REQUIRE(wb_make_plan(&d, bands, 3, (int)nc, &q, "asan_bwd_band_plan") == DCLL_OK);
        REQUIRE(out[0] == q.g.NB && out[1] == q.g.RB && out[2] == q.g.TPW && out[3] == q.g.PS && out[4] == q.NQ && out[5] == q.NS &&
                out[6] == q.nsplit && out[7] == nc);
        for (nchunk = 1; nchunk <= WB_MAX_CHUNKS; ++nchunk) {
            ++pairs;
            if (walk(d, bands, nchunk, &full)) return 1;
        }
    }
    return 0;
}

int main()
{
    // the geometries of tests/bwd_band_cases.py: {c_in, c_out, kh, kw, pad_h, pad_w, h, w}
    static const int geoms[][8] = {
        {1, 1, 3, 3, 1, 1, 2, 5},      {3, 32, 3, 3, 1, 1, 3, 6},     {1, 33, 3, 3, 1, 1, 4, 7},    {3, 64, 3, 3, 1, 1, 5, 8},
        {1, 65, 3, 3, 1, 1, 6, 5},     {3, 96, 3, 3, 1, 1, 7, 6},     {1, 129, 3, 3, 1, 1, 8, 7},   {3, 1, 3, 3, 1, 1, 9, 8},
        {3, 33, 5, 3, 2, 1, 6, 7},     {2, 65, 2, 2, 3, 1, 4, 6},     {2, 20, 2, 2, 3, 1, 4, 6},    {3, 64, 3, 3, 0, 0, 8, 7},
        {2, 36, 3, 3, 1, 0, 6, 3},     {7, 96, 1, 1, 0, 0, 6, 7},     {3, 129, 2, 5, 1, 2, 6, 8},   {2, 65, 9, 9, 4, 4, 10, 10},
        {2, 20, 9, 9, 4, 4, 10, 9},    {70, 33, 3, 3, 1, 1, 6, 7},    {3, 65, 3, 3, 1, 1, 7, 6},    {2, 9, 5, 3, 2, 1, 8, 5},
        {2, 33, 3, 3, 1, 1, 4, 4},     {3, 97, 3, 3, 1, 1, 9, 11},    {1, 32, 4, 8, 1, 3, 3, 5},    {5, 32, 4, 8, 1, 3, 3, 5},
        {9, 65, 4, 8, 1, 3, 3, 5},     {17, 32, 4, 8, 1, 3, 3, 5},    {33, 65, 4, 8, 1, 3, 3, 5},   {24, 65, 4, 8, 1, 3, 3, 5},
        {1, 64, 7, 7, 3, 3, 24, 40},   {64, 64, 7, 7, 3, 3, 24, 40},  {32, 32, 7, 7, 3, 3, 48, 48}, {4, 96, 3, 3, 1, 1, 24, 40},
        {1, 65, 1, 1, 0, 0, 157, 4},   {1, 65, 1, 1, 0, 0, 158, 4},   {1, 65, 1, 1, 0, 0, 400, 4},  {1, 65, 1, 1, 0, 0, 2, 700},
        {64, 64, 7, 7, 3, 3, 128, 128}, {32, 32, 7, 7, 3, 3, 100, 100}, {20, 200, 16, 16, 8, 8, 20, 24}, {2, 96, 17, 3, 8, 1, 10, 10}};
    long ngeom = 0;
    for (const auto &q : geoms)
        for (int dv = 0; dv < 7; ++dv) {    // the geometry, and one row / column / input channel / output channel more or less
            dcll_conv_desc d;
            memset(&d, 0, sizeof d);
            d.c_in = q[0] + (dv == 1), d.c_out = q[1] + (dv == 2) - (dv == 3), d.kh = q[2], d.kw = q[3], d.pad_h = q[4], d.pad_w = q[5];
            d.h = q[6] + (dv == 4) - (dv == 5), d.w = q[7] + (dv == 6);
            d.pool_h = d.pool_w = 1, d.stride = d.dilation = d.groups = 1, d.target = 10;
            if (d.c_out < 1 || d.h < 1) continue;
            ++ngeom;
            if (walk_desc(d)) return 1;
        }
    // the grid's bound and the refusals of the entry points
    dcll_conv_desc d;
    memset(&d, 0, sizeof d);
    d.c_in = 1, d.c_out = 64 * 65535, d.h = d.w = 2, d.kh = d.kw = 1, d.pool_h = d.pool_w = 1, d.stride = d.dilation = d.groups = 1, d.target = 4;
    if (dcll_conv_lif_backward_bands_lds(&d, 2) <= 0) return 4;
    d.c_out += 1;
    if (dcll_conv_lif_backward_bands_lds(&d, 2) != 0 || !strstr(err_buf, "more than 65535 slabs")) return 4;
    d.c_out = 96, d.stride = 2;
    if (dcll_conv_lif_backward_bands_lds(&d, 2) != 0 || !strstr(err_buf, "plain convolutions only")) return 4;
    int32_t out[8];
    if (dcll_conv_lif_backward_bands_lds(nullptr, 0) != 0 || dcll_conv_lif_backward_bands_plan(nullptr, 1, 0, out) == DCLL_OK ||
        dcll_conv_lif_backward_bands_plan(&d, 1, 0, nullptr) != DCLL_ERR_INVALID)
        return 4;
    printf("asan_bwd_band_plan ok: %ld geometries, %ld (descriptor, bands, chunks) pairs walked: %ld served layouts, %ld forwarded, "
           "%ld refused\n", ngeom, pairs, served, forwarded, refused);
    return 0;
}
