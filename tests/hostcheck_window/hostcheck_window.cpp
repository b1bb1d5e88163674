// test infrastructure: a stand-alone host driver of the product's sliding-window arithmetic (csrc/window_math.hpp, and through it the
// vote of csrc/tta_math.hpp and the taps, gathers and softmax of csrc/pixel_math.hpp), the very functions the kernels of
// csrc/window.hip call, walked pixel by pixel ("thread by thread") in the launch's order, the workgroup's LDS tables replaced by
// heap blocks.
//
//   hostcheck_window REQUEST RESULT
//
// REQUEST, little-endian int32 words, the first being the operation:
//   op = 0 (vote): n, c, H, W, k, align_corners, label_dtype, ignore_index, wh, ww, null_mask (bit 0: labels, 1: cm, 2: pred_out,
//                  3: logits[0] are passed as NULL); per view 11 x int32 hl, wl, Hv, Wv, gy, gx, eh, ew, sh, sw, flip; per view an
//                  int64 count and that many float32 logits; the n * H * W labels (uint8 or int64).
//                  RESULT: int64 cm (c, c); one int64: the pixels at which win_vote_pixel differs from tta_vote_pixel when no view
//                  has more than one window and k >= 2 (-1 where that does not apply); n * H * W uint8 pred; float32 score
//                  (n, c, H, W): the scores the prediction was taken from (k == 1 with one window: the interpolated logits).
//   op = 1 (crop): n, c, H, W, Hv, Wv, flip, wh, ww, sh, sw, then the (n, c, H, W) float32 source
//                  RESULT: (n * gy * gx, c, eh, ew) float32
// Every tensor lives in an exactly-sized heap block and the outputs are poisoned before use, so a sanitizer build sees every byte
// outside them. Exit code 2 for a request the product refuses (the refusal is the product's own check), 3 for a view table whose
// logits count is not the one the descriptor implies.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cutmix-semisup-seg_amd/csrc/window_math.hpp"
#include "../hostcheck_common.hpp"

using namespace cms;

static Blocks g_blocks;          // every heap block of the run (hostcheck_common.hpp)

static int vote(FILE* f, const char* result) {
    int32_t head[11];
    if (fread(head, sizeof(int32_t), 11, f) != 11) return 1;
    cms_window_desc d;
    memset(&d, 0, sizeof(d));
    d.n = head[0], d.c = head[1], d.H = head[2], d.W = head[3], d.k = head[4], d.align_corners = head[5];
    d.label_dtype = head[6], d.ignore_index = head[7], d.wh = head[8], d.ww = head[9];
    const int null_mask = head[10];
    uint8_t dummy = 0;
    d.pred_out = &dummy;                                   // "something to produce" while the sizes are judged
    if (d.k < 1 || d.k > CMS_TTA_MAX_VIEWS) return win_check_vote(&d) ? 2 : 1;       // no view table to read: the product's verdict
    for (int i = 0; i < d.k; ++i) {
        int32_t v[11];
        if (fread(v, sizeof(int32_t), 11, f) != 11) return 1;
        d.hl[i] = v[0], d.wl[i] = v[1], d.Hv[i] = v[2], d.Wv[i] = v[3], d.gy[i] = v[4], d.gx[i] = v[5], d.eh[i] = v[6], d.ew[i] = v[7];
        d.sh[i] = v[8], d.sw[i] = v[9], d.flip[i] = v[10];
    }
    // the product's verdict on the sizes before anything is read or allocated by them
    float probe = 0.0f;
    for (int i = 0; i < d.k; ++i) d.logits[i] = &probe;
    if (win_check_vote(&d)) return 2;
    for (int i = 0; i < d.k; ++i) {
        int64_t count;
        if (fread(&count, sizeof(int64_t), 1, f) != 1) return 1;
        if (count != (int64_t)d.n * d.gy[i] * d.gx[i] * d.c * d.hl[i] * d.wl[i]) return 3;
        d.logits[i] = (const float*)read_block(f, (size_t)count * sizeof(float), &g_blocks);
    }
    const size_t plane = (size_t)d.H * d.W, pix = (size_t)d.n * plane;
    if (d.label_dtype != CMS_LABEL_U8 && d.label_dtype != CMS_LABEL_I64) return 2;
    void* labels = read_block(f, pix * (d.label_dtype == CMS_LABEL_I64 ? 8 : 1), &g_blocks);
    int64_t* cm = (int64_t*)g_blocks.keep(calloc((size_t)d.c * d.c, sizeof(int64_t)));
    uint8_t* pred = (uint8_t*)g_blocks.keep(malloc(pix));
    float* out = (float*)g_blocks.keep(malloc(pix * d.c * sizeof(float)));
    float* score = (float*)g_blocks.keep(malloc((size_t)d.c * sizeof(float)));
    float* score2 = (float*)g_blocks.keep(malloc((size_t)d.c * sizeof(float)));
    memset(pred, 0xA5, pix);
    d.labels = (null_mask & 1) ? nullptr : labels;
    d.cm = (null_mask & 2) ? nullptr : cm;
    d.pred_out = (null_mask & 4) ? nullptr : pred;
    if (null_mask & 8) d.logits[0] = nullptr;
    if (win_check_vote(&d)) return 2;

    const bool align = d.align_corners != 0, forward = win_all_single(&d);
    WinViews v;
    win_make_views(&d, &v);
    cms_tta_desc td;
    win_tta_desc(&d, &td);
    TtaViews tv;
    tta_make_views(&td, &tv);
    int64_t claim = forward && d.k >= 2 ? 0 : -1;
    for (size_t idx = 0; idx < pix; ++idx) {
        const int x = (int)(idx % d.W);
        const size_t t_ = idx / d.W;
        const int y = (int)(t_ % d.H), n = (int)(t_ / d.H);
        for (int c = 0; c < d.c; ++c) score[c] = score2[c] = NAN;
        int best;
        if (forward && d.k == 1) {
            // cms_tta_vote's single view: the argmax of the logits
            const bool ident = td.h[0] == d.H && td.w[0] == d.W;
            best = ident ? tta_single_pixel<true>(tv, n, d.c, y, x, align) : tta_single_pixel<false>(tv, n, d.c, y, x, align);
            const size_t pl = (size_t)td.h[0] * td.w[0];
            const float* base = tv.logits[0] + (size_t)n * d.c * pl;
            const Tap ty = bilin_tap(y, tv.sy[0], td.h[0], align);
            const Tap tx = tta_tap_x(x, tv.sx[0], td.w[0], align, tv.flip[0] != 0);
            const size_t off = (size_t)y * td.w[0] + (tv.flip[0] ? td.w[0] - 1 - x : x);
            for (int c = 0; c < d.c; ++c) score[c] = ident ? base[c * pl + off] : bilin_gather(base + c * pl, td.w[0], ty, tx);
        } else if (forward) {
            best = tta_vote_pixel(tv, d.k, n, d.c, y, x, align, [&](int c) -> float& { return score[c]; });
            const int other = win_vote_pixel(v, d.k, n, d.c, d.H, d.W, y, x, align, [&](int c) -> float& { return score2[c]; });
            if (other != best || memcmp(score, score2, (size_t)d.c * sizeof(float)) != 0) claim += 1;
        } else {
            best = win_vote_pixel(v, d.k, n, d.c, d.H, d.W, y, x, align, [&](int c) -> float& { return score[c]; });
        }
        if (d.pred_out) d.pred_out[idx] = (uint8_t)best;
        for (int c = 0; c < d.c; ++c) out[((size_t)n * d.c + c) * plane + (idx % plane)] = score[c];
        if (d.labels && d.cm) {
            const int tr = tta_label(d.labels, d.label_dtype, idx);
            if (tr != d.ignore_index && tr >= 0 && tr < d.c) d.cm[tr * d.c + best] += 1;
        }
    }
    FILE* o = fopen(result, "wb");
    if (!o) return 1;
    fwrite(cm, sizeof(int64_t), (size_t)d.c * d.c, o);
    fwrite(&claim, sizeof(int64_t), 1, o);
    fwrite(pred, 1, pix, o);
    fwrite(out, sizeof(float), pix * d.c, o);
    fclose(o);
    return 0;
}

static int crop(FILE* f, const char* result) {
    int32_t h[11];
    if (fread(h, sizeof(int32_t), 11, f) != 11) return 1;
    const int n = h[0], c = h[1], H = h[2], W = h[3], Hv = h[4], Wv = h[5], flip = h[6], wh = h[7], ww = h[8], sh = h[9], sw = h[10];
    float probe = 0.0f;
    if (win_check_crop(&probe, &probe, n, c, H, W, Hv, Wv, wh, ww, sh, sw, CMS_F32)) return 2;
    const int gy = win_count(Hv, wh, sh), gx = win_count(Wv, ww, sw), eh = win_extent(Hv, wh), ew = win_extent(Wv, ww);
    const size_t total = (size_t)n * gy * gx * c * eh * ew;
    const float* src = (const float*)read_block(f, (size_t)n * c * H * W * sizeof(float), &g_blocks);
    float* dst = (float*)g_blocks.keep(malloc(total * sizeof(float)));
    for (size_t i = 0; i < total; ++i) dst[i] = NAN;
    for (size_t idx = 0; idx < total; ++idx) {
        const WinCropAt a = win_crop_at(idx, c, Hv, Wv, gy, gx, eh, ew, sh, sw);
        const float* plane = src + a.plane * ((size_t)H * W);
        dst[idx] = win_crop_pixel([&](size_t i) { return plane[i]; }, H, W, Hv, Wv, flip != 0, a.vy, a.vx);
    }
    FILE* o = fopen(result, "wb");
    if (!o) return 1;
    fwrite(dst, sizeof(float), total, o);
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_window REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t op;
    if (fread(&op, sizeof(int32_t), 1, f) != 1) return 1;
    const int rc = op == 0 ? vote(f, argv[2]) : (op == 1 ? crop(f, argv[2]) : 1);
    fclose(f);
    return rc;
}
