// test infrastructure: a stand-alone host driver of the product's calibration arithmetic (csrc/calib_math.hpp, and through it the
// vote of csrc/tta_math.hpp and the taps, gathers, softmax and cross entropy of csrc/pixel_math.hpp), the very functions the kernel
// of csrc/calib.hip calls, walked pixel by pixel ("thread by thread") in the launch's order, the workgroup's LDS tables replaced by
// the global ones.
//
//   hostcheck_calib REQUEST RESULT
//
// REQUEST, little-endian: int32 n, c, H, W, k, align_corners, label_dtype, ignore_index, nb, nt, n_edges, n_temps, null_mask
// (bit 0: labels, 1: hist, 2: scores, 3: cm, 4: pred_out, 5: edges, 6: temps are passed as NULL); n_edges float32 edges; n_temps
// float32 temperatures; per view int32 h, w, flip; then per view its (n, c, h, w) float32 logits; the n * H * W labels (uint8 or int64).
// RESULT: int64 hist (c, nb, 3), scores (2 + nt), cm (c, c); 3 int64 counts of pixels at which a bit-for-bit claim does not hold (-1
// where it does not apply): conf vs consistency_pixel_fwd's and nll vs ce_pixel_fwd's (k == 1, T == 1), pred vs tta_vote_pixel /
// tta_single_pixel (T == 1, or k == 1); n * H * W uint8 pred; float32 conf, squared error (n * H * W each) and nll (nt, n * H * W),
// NaN at pixels that are not scored.
// Every tensor lives in an exactly-sized heap block and the outputs are filled with 0xA5 before use, so a sanitizer build sees every
// byte outside them. Exit code 2 for a request the product refuses (the refusal is the product's own calib_check).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cutmix-semisup-seg_amd/csrc/calib_math.hpp"
#include "../hostcheck_common.hpp"

using namespace cms;

static Blocks g_blocks;          // every heap block of the run (hostcheck_common.hpp)

static uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_calib REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[13];
    if (fread(head, sizeof(int32_t), 13, f) != 13) return 1;
    cms_calib_desc d;
    memset(&d, 0, sizeof(d));
    d.n = head[0], d.c = head[1], d.H = head[2], d.W = head[3], d.k = head[4], d.align_corners = head[5];
    d.label_dtype = head[6], d.ignore_index = head[7], d.nb = head[8], d.nt = head[9];
    const int n_edges = head[10], n_temps = head[11], null_mask = head[12];
    if (n_edges < 0 || n_edges > 4096 || n_temps < 0 || n_temps > 4096) return 1;
    float* edges = (float*)read_block(f, (size_t)n_edges * sizeof(float), &g_blocks);
    float* temps = (float*)read_block(f, (size_t)n_temps * sizeof(float), &g_blocks);
    // what the driver itself needs to lay the request out; the product's check decides everything else
    if (d.k < 1 || d.k > CMS_TTA_MAX_VIEWS || d.n < 1 || d.c < 1 || d.c > kTtaMaxClasses || d.H < 1 || d.W < 1 ||
        !tta_count_ok(d.n, d.H, d.W))
        return 2;
    for (int i = 0; i < d.k; ++i) {
        int32_t v[3];
        if (fread(v, sizeof(int32_t), 3, f) != 3) return 1;
        d.h[i] = v[0], d.w[i] = v[1], d.flip[i] = v[2];
        if (v[0] < 1 || v[1] < 1 || !tta_count_ok(d.n, d.c, v[0], v[1])) return 2;
    }
    for (int i = 0; i < d.k; ++i) d.logits[i] = (const float*)read_block(f, (size_t)d.n * d.c * d.h[i] * d.w[i] * sizeof(float), &g_blocks);
    const size_t plane = (size_t)d.H * d.W, pix = (size_t)d.n * plane;
    if (d.label_dtype != CMS_LABEL_U8 && d.label_dtype != CMS_LABEL_I64) return 2;
    void* labels = read_block(f, pix * (d.label_dtype == CMS_LABEL_I64 ? 8 : 1), &g_blocks);
    fclose(f);
    // the tables are sized for what the request CLAIMS only when the claim is inside the limits (else the check refuses first)
    const int nb = d.nb >= 1 && d.nb <= CMS_CALIB_MAX_BINS ? d.nb : 1, nt = d.nt >= 1 && d.nt <= CMS_CALIB_MAX_TEMPS ? d.nt : 1;
    if ((d.nb == nb && n_edges != nb - 1) || (d.nt == nt && n_temps != nt)) return 1;
    const size_t cells = (size_t)d.c * nb;
    int64_t* hist = (int64_t*)g_blocks.keep(calloc(cells * 3, sizeof(int64_t)));
    int64_t* scores = (int64_t*)g_blocks.keep(calloc(2 + nt, sizeof(int64_t)));
    int64_t* cm = (int64_t*)g_blocks.keep(calloc((size_t)d.c * d.c, sizeof(int64_t)));
    uint8_t* pred = (uint8_t*)g_blocks.keep(malloc(pix));
    float* conf = (float*)g_blocks.keep(malloc(pix * sizeof(float)));
    float* brier = (float*)g_blocks.keep(malloc(pix * sizeof(float)));
    float* nll = (float*)g_blocks.keep(malloc(pix * nt * sizeof(float)));
    memset(pred, 0xA5, pix);
    d.labels = (null_mask & 1) ? nullptr : labels;
    d.hist = (null_mask & 2) ? nullptr : hist;
    d.scores = (null_mask & 4) ? nullptr : scores;
    d.cm = (null_mask & 8) ? nullptr : cm;
    d.pred_out = (null_mask & 16) ? nullptr : pred;
    d.edges = (null_mask & 32) ? nullptr : edges;
    d.temps = (null_mask & 64) ? nullptr : temps;
    if (calib_check(&d)) return 2;

    cms_tta_desc td;
    calib_tta_desc(&d, &td);
    TtaViews v;
    tta_make_views(&td, &v);
    CalibParams prm;
    calib_make_params(&d, &prm);
    const bool align = d.align_corners != 0, ident = d.k == 1 && d.h[0] == d.H && d.w[0] == d.W, t_one = d.temps[0] == 1.0f;
    int64_t claims[3] = {d.k == 1 && t_one ? 0 : -1, d.k == 1 && t_one ? 0 : -1, (t_one || d.k == 1) ? 0 : -1};
    float score[kTtaMaxClasses], score2[kTtaMaxClasses];
    const float nan_ = nanf("");
    for (size_t idx = 0; idx < pix; ++idx) {
        const int x = (int)(idx % d.W);
        const size_t t_ = idx / d.W;
        const int y = (int)(t_ % d.H), n = (int)(t_ / d.H);
        const int label = calib_valid_label(tta_label(d.labels, d.label_dtype, idx), d.ignore_index, d.c);
        CalibPixel px;
        float px_nll[CMS_CALIB_MAX_TEMPS];
        int want_pred;
        if (d.k >= 2) {
            calib_vote_pixel(v, d.k, n, d.c, y, x, align, label, prm, [&](int c) -> float& { return score[c]; }, px, px_nll);
            want_pred = tta_vote_pixel(v, d.k, n, d.c, y, x, align, [&](int c) -> float& { return score2[c]; });
        } else if (ident) {
            calib_single_pixel<true>(v, n, d.c, y, x, align, label, prm, px, px_nll);
            want_pred = tta_single_pixel<true>(v, n, d.c, y, x, align);
        } else {
            calib_single_pixel<false>(v, n, d.c, y, x, align, label, prm, px, px_nll);
            want_pred = tta_single_pixel<false>(v, n, d.c, y, x, align);
        }
        if (claims[2] >= 0 && px.pred != want_pred) claims[2] += 1;
        if (d.pred_out) d.pred_out[idx] = (uint8_t)px.pred;
        conf[idx] = brier[idx] = nan_;
        for (int t = 0; t < nt; ++t) nll[(size_t)t * pix + idx] = nan_;
        if (label < 0) continue;
        if (claims[0] >= 0) {
            // the training step's own functions on the same gathered logits
            const int h = v.h[0], w = v.w[0];
            const size_t pl = (size_t)h * w;
            const float* base = v.logits[0] + (size_t)n * d.c * pl;
            const Tap ty = bilin_tap(y, v.sy[0], h, align);
            const Tap tx = tta_tap_x(x, v.sx[0], w, align, v.flip[0] != 0);
            const size_t off = (size_t)y * w + (v.flip[0] ? w - 1 - x : x);
            auto l = [&](int c) { return ident ? base[c * pl + off] : bilin_gather(base + c * pl, w, ty, tx); };
            const PixelFwd fw = consistency_pixel_fwd<0>(l, l, d.c, LOSS_VAR, 1.0f);
            if (bits(fw.conf) != bits(px.conf)) claims[0] += 1;
            if (bits(ce_pixel_fwd<0>(l, d.c, label)) != bits(px_nll[0])) claims[1] += 1;
        }
        const int cell = px.pred * nb + calib_bin(prm, px.conf);
        hist[3 * cell] += 1;
        hist[3 * cell + 1] += px.pred == label;
        hist[3 * cell + 2] += (int64_t)calib_fx(px.conf, kCalibConfScale, 1.0f);
        if (d.cm) d.cm[label * d.c + px.pred] += 1;
        scores[0] += 1;
        scores[1] += (int64_t)calib_fx(px.brier, kCalibBrierScale, 2.0f);
        conf[idx] = px.conf, brier[idx] = px.brier;
        for (int t = 0; t < nt; ++t) {
            scores[2 + t] += (int64_t)calib_fx(px_nll[t], kCalibNllScale, kCalibNllCap);
            nll[(size_t)t * pix + idx] = px_nll[t];
        }
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(hist, sizeof(int64_t), cells * 3, o);
    fwrite(scores, sizeof(int64_t), 2 + nt, o);
    fwrite(cm, sizeof(int64_t), (size_t)d.c * d.c, o);
    fwrite(claims, sizeof(int64_t), 3, o);
    fwrite(pred, 1, pix, o);
    fwrite(conf, sizeof(float), pix, o);
    fwrite(brier, sizeof(float), pix, o);
    fwrite(nll, sizeof(float), pix * nt, o);
    fclose(o);
    return 0;
}
