// asan_step_slab_plan.hip — the HOST side of dcll_conv_lif_step_slab under AddressSanitizer, on the CPU: a stand-alone program that
// walks the geometries of tests/step_slab_cases.py (and the bounds around them) through dcll_step_slab_plan — the layer predicate,
// NB_fit, the small-batch rule, explicit band counts — and through the exported _plan / _lds / _scratch, and checks the invariants
// the kernel's indexing relies on: the bands partition the conv rows and the pooled rows, every pooling window of an owned row lies
// in its band, every band's layout is the exported LDS formula and inside the LDS, the first and the last B-operand offset a lane
// can form lie inside the band's staged rows, the slabs partition [0, c_out).  Nothing is launched and no GPU is needed.
//
//   cd snn_modulation_classification_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -o /tmp/asan_step_slab_plan ../../experiments/asan_step_slab_plan.hip \
//         && ASAN_OPTIONS=detect_leaks=0 /tmp/asan_step_slab_plan
//
// (detect_leaks=0: the HIP runtime's start-up allocations are not this program's.)  Exit status 0 and "asan_step_slab_plan ok" = clean.
#include "../snn_modulation_classification_amd/csrc/dcll_step_slab.hip"

#include <vector>

// what dcll_hip.hip provides to the library's translation units
static thread_local char err_buf[DCLL_ERR_LEN];
char *dcll_err_buf(void) { return err_buf; }
void dcll_trace_note(const char *) {}
// dcll_step_wide.hip's part of the forwarding rule, restated: a plain conv layer of at most 64 output channels with a kernel up to
// 16x16 whose working set (c_out <= 32: k_lif_step_any's, the same image and a c_out-row v plane) fits in the LDS
static bool wide_serves(const dcll_conv_desc *d)
{
    if (check_desc(d) != DCLL_OK || !plain_conv(d) || d->c_out > 64 || d->kh > ANY_MAX_K || d->kw > ANY_MAX_K) return false;
    int ch, cw, ph, pw;
    conv_shape(d, &ch, &cw, &ph, &pw);
    const long img = (long)d->c_in * (d->h + 2 * d->pad_h) * (d->w + 2 * d->pad_w);
    const long vpl = step_slab_pooled(d) ? (long)d->c_out * ch * cw : 0;
    return (img + vpl + (d->c_out <= 32 ? 32 : 64)) * 4 <= ANY_LDS_MAX;
}
int dcll_step_wide_check(const dcll_conv_desc *d, const char *who)
{
    return wide_serves(d) ? DCLL_OK : fail(DCLL_ERR_UNSUPPORTED, "not served by the 64-channel step", who);
}
extern "C" int64_t dcll_conv_lif_step_wide_lds(const dcll_conv_desc *d) { return wide_serves(d) ? 4 : 0; }

#define REQUIRE(cond)                                                                                                        \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "asan_step_slab_plan: %s fails at line %d (c_in %d c_out %d k %dx%d plane %dx%d pad %d,%d pool %d,%d B %d bands %d)\n", \
                    #cond, __LINE__, d.c_in, d.c_out, d.kh, d.kw, d.h, d.w, d.pad_h, d.pad_w, d.pool_h, d.pool_w, B, bands);  \
            return 1;                                                                                                        \
        }                                                                                                                    \
    } while (0)

static long checked = 0, served = 0, forwarded = 0;

static int walk(dcll_conv_desc d, int B, int bands)
{
    ++checked;
    int32_t nb = -7, ns = -7;
    const int rc = dcll_conv_lif_step_slab_plan(&d, B, bands, &nb, &ns);
    const int64_t lds = dcll_conv_lif_step_slab_lds(&d, B, bands);
    if (rc != DCLL_OK) {
        REQUIRE(rc == DCLL_ERR_UNSUPPORTED || rc == DCLL_ERR_INVALID);
        REQUIRE(strlen(err_buf) > 0 && strlen(err_buf) < DCLL_ERR_LEN && lds == 0 && nb == -7 && ns == -7);
        return 0;
    }
    if (nb == 0) {      // dcll_conv_lif_step_wide's call
        ++forwarded;
        REQUIRE(ns == 0 && bands == 0 && d.c_out <= SLAB_ROWS && wide_serves(&d) && lds == 4);
        return 0;
    }
    ++served;
    int ch, cw, ph, pw;
    conv_shape(&d, &ch, &cw, &ph, &pw);
    REQUIRE(ns == slab_count(d.c_out) && ns >= 1 && ns <= SLAB_MAX && nb >= 1 && nb <= ph && (bands == 0 || nb == bands));
    REQUIRE(dcll_conv_lif_step_slab_scratch(&d) == any_chain_steps(&d) * 128 * ns);
    const int WP = d.w + 2 * d.pad_w, KK = d.kh * d.kw, npair = (int)any_chain_pairs(&d), pph = (d.pool_h - 1) / 2;
    long mx = 0;
    int c_prev = 0, p_prev = 0;
    for (int k = 0; k < nb; ++k) {
        const band_rows r = band_plan(k, nb, d.h, d.kh, d.pad_h, d.pool_h, ch, ph);
        REQUIRE(r.C0 == c_prev && r.P0 == p_prev && r.C1 > r.C0 && r.P1 > r.P0 && r.C1 <= ch && r.P1 <= ph);
        c_prev = r.C1;
        p_prev = r.P1;
        for (int py = r.P0; py < r.P1; ++py) {      // the windows of the band's pooled rows, clipped to the plane, lie in its conv rows
            const int y0 = py * d.pool_h - pph < 0 ? 0 : py * d.pool_h - pph;
            const int y1 = (py + 1) * d.pool_h - pph > ch ? ch : (py + 1) * d.pool_h - pph;
            REQUIRE(y0 < y1 && r.C0 <= y0 && y1 <= r.C1);
        }
        const long crows = r.C1 - r.C0, rows = crows + d.kh - 1, CHS = rows * WP, NPb = crows * cw;
        const long fl = step_slab_lds_floats(&d, k, nb);
        REQUIRE(fl == d.c_in * CHS + (step_slab_pooled(&d) ? SLAB_ROWS * NPb : 0) + SLAB_ROWS && fl * 4 <= ANY_LDS_MAX);
        if (fl > mx) mx = fl;
        // the last pixel's last B operand of the channel-pair part (both halves) and of an odd last channel's taps
        const long base_last = (NPb - 1) / cw * WP + (NPb - 1) % cw;
        if (npair) REQUIRE(base_last + CHS + (long)((npair - 1) / KK) * 2 * CHS + (d.kh - 1) * WP + d.kw - 1 < d.c_in * CHS);
        if (d.c_in & 1) REQUIRE((d.c_in - 1) * CHS + base_last + (long)((KK - 1) / d.kw) * WP + (KK - 1) % d.kw < d.c_in * CHS);
        // the staging's divisions: exact while q * divisor < 2^32
        REQUIRE((double)d.c_in * CHS * WP < 4294967296.0 && (double)d.c_in * rows * rows < 4294967296.0);
        REQUIRE(!step_slab_pooled(&d) || (double)SLAB_ROWS * NPb * NPb < 4294967296.0);
    }
    REQUIRE(c_prev == ch && p_prev == ph && mx * 4 == lds);
    if (bands == 0) {   // the rule: no smaller count fits unless the small-batch rule asked for this one
        int fit = 0;
        for (int q = 1; q <= ph && !fit; ++q)
            if (step_slab_lds_max(&d, q) * 4 <= ANY_LDS_MAX) fit = q;
        const long units = 2 * (((long)ch * cw + 31) / 32);
        long ns0 = (units + SS_UNITS - 1) / SS_UNITS;
        if (ns0 > ANY_CUS / ((long)B * ns)) ns0 = ANY_CUS / ((long)B * ns);
        if (ns0 > ph) ns0 = ph;
        REQUIRE(fit >= 1 && nb == (ns0 > fit ? ns0 : fit));
    }
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
    const int couts[] = {1, 32, 33, 40, 64, 65, 96, 97, 128, 129, 200, 64 * 65535, 64 * 65535 + 1};
    const int cins[] = {1, 3, 64, 70, 84, 85, 96, 128};
    const int kernels[][2] = {{1, 1}, {2, 5}, {3, 3}, {7, 7}, {9, 9}, {16, 16}, {17, 3}};
    const int planes[][2] = {{1, 1}, {4, 4}, {5, 7}, {6, 3}, {8, 8}, {6, 11}, {9, 10}, {12, 11}, {16, 16}, {17, 16}, {24, 40}, {128, 128}};
    const int pools[][2] = {{1, 1}, {2, 2}, {3, 3}, {1, 2}, {3, 2}};
    const int batches[] = {1, 17, 18, 43, 64, 65, 300};
    const int bandss[] = {0, 1, 2, 3, 5, 40, -1};
    for (int c_out : couts)
        for (int c_in : cins)
            for (const auto &k : kernels)
                for (const auto &hw : planes)
                    for (const auto &pl : pools)
                        for (int pad = 0; pad < 2; ++pad) {
                            dcll_conv_desc d;
                            memset(&d, 0, sizeof d);
                            d.c_in = c_in, d.c_out = c_out, d.h = hw[0], d.w = hw[1], d.kh = k[0], d.kw = k[1];
                            d.pad_h = pad ? k[0] / 2 : 0, d.pad_w = pad ? k[1] / 2 : 0;
                            d.pool_h = pl[0], d.pool_w = pl[1], d.stride = d.dilation = d.groups = 1, d.target = 10;
                            for (int B : batches)
                                for (int bands : bandss) {
                                    if (hw[0] > 40 && ((B != 1 && B != 64) || bands > 1)) continue;     // (128 rows: the fit loop is long)
                                    if (walk(d, B, bands)) return 1;
                                }
                        }
    // refusals: a null descriptor, null results, stride / dilation / groups, a batch of none
    int32_t nb, ns;
    if (dcll_conv_lif_step_slab_lds(nullptr, 1, 0) != 0 || dcll_conv_lif_step_slab_scratch(nullptr) != 0) return 4;
    if (dcll_conv_lif_step_slab_plan(nullptr, 1, 0, &nb, &ns) == DCLL_OK) return 4;
    dcll_conv_desc d;
    memset(&d, 0, sizeof d);
    d.c_in = 2, d.c_out = 96, d.h = d.w = 10, d.kh = d.kw = 3, d.pad_h = d.pad_w = 1, d.pool_h = d.pool_w = 1, d.target = 10;
    d.stride = d.dilation = d.groups = 1;
    if (dcll_conv_lif_step_slab_plan(&d, 1, 0, nullptr, &ns) != DCLL_ERR_INVALID) return 4;
    if (dcll_conv_lif_step_slab_plan(&d, 0, 0, &nb, &ns) != DCLL_ERR_INVALID || dcll_conv_lif_step_slab_lds(&d, 0, 0) != 0) return 4;
    d.stride = 2;
    if (dcll_conv_lif_step_slab_lds(&d, 1, 0) != 0 || !strstr(err_buf, "plain convolutions only")) return 4;
    d.stride = 1, d.dilation = 2;
    if (dcll_conv_lif_step_slab_lds(&d, 1, 0) != 0) return 4;
    d.dilation = 1, d.groups = 2;
    if (dcll_conv_lif_step_slab_lds(&d, 1, 0) != 0) return 4;
    printf("asan_step_slab_plan ok: %ld plans walked, %ld served by k_lif_step_slab, %ld forwarded\n", checked, served, forwarded);
    return 0;
}
