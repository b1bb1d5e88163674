// Calibration and pseudo-label quality (csrc/calib.hip): descriptor validation, the LDS budget and the per-pixel arithmetic -- the
// vote of tta_math.hpp with the confidence kept, the bin of a confidence, and the fixed-point values that are summed. Everything
// here is plain C++ / `__host__ __device__`, so tests/hostcheck_calib drives the very code the kernel is made of on the host; the
// product never runs it there. Taps, gathers, the softmax and the cross entropy are pixel_math.hpp's, the vote and the single-view
// argmax tta_math.hpp's, under the same `fp contract(off)` discipline.
//
// Why fixed point: every value that is summed over pixels is first rounded to an integer (conf * 2^24, the squared error * 2^24,
// nll * 2^20), so the sums are integer sums and do not depend on the order in which the atomics arrive: the same input gives the
// same bits on every call. Ranges: conf <= 1 -> 2^24, the squared error <= 2 -> 2^25, nll is cut at 88 (-logf(FLT_MIN) = 87.34)
// -> 88 * 2^20 < 2^27; over at most 2^31 - 1 pixels of a launch that is below 2^58, and an int64 takes 32 such launches of the
// worst case before it could overflow (an evaluation of 10^5 images of 2 MPixel with nll = 88 everywhere stays below 2^62).
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/cutmixseg.h"
#include "tta_math.hpp"

namespace cms {

constexpr int kCalibBlock = 256;
constexpr size_t kCalibLdsLimit = 160 * 1024;            // gfx950: LDS per CU, all of which one workgroup may take
constexpr float kCalibConfScale = 16777216.0f;           // 2^24
constexpr float kCalibBrierScale = 16777216.0f;          // 2^24
constexpr float kCalibNllScale = 1048576.0f;             // 2^20
constexpr float kCalibNllCap = 88.0f;
constexpr int kCalibScores = 2 + CMS_CALIB_MAX_TEMPS;

// what the kernel reads besides the views: the partition and the temperatures, worked out once on the host
struct CalibParams {
    float edges[CMS_CALIB_MAX_BINS - 1];
    float inv_t[CMS_CALIB_MAX_TEMPS];
    int scaled[CMS_CALIB_MAX_TEMPS];                     // temps[t] != 1: the multiply is made
    int nb, nt;
};

// the vote's part of the descriptor
inline void calib_tta_desc(const cms_calib_desc* d, cms_tta_desc* t) {
    for (int i = 0; i < CMS_TTA_MAX_VIEWS; ++i) t->logits[i] = d->logits[i], t->h[i] = d->h[i], t->w[i] = d->w[i], t->flip[i] = d->flip[i];
    t->n = d->n, t->c = d->c, t->H = d->H, t->W = d->W, t->k = d->k, t->align_corners = d->align_corners;
    t->labels = d->labels, t->label_dtype = d->label_dtype, t->ignore_index = d->ignore_index;
    t->cm = d->cm, t->pred_out = d->pred_out;
}

// bytes of LDS a workgroup takes: the score columns (k >= 2), then 64-bit cells (confidence sums, the score totals), then 32-bit
// cells (pixels and correct pixels per bin, the confusion matrix)
inline size_t calib_lds_bytes(int c, int nb, int k) {
    const size_t cells = (size_t)c * nb;
    return (k >= 2 ? (size_t)c * kCalibBlock * sizeof(float) : 0) + (cells + kCalibScores) * 8 + (2 * cells + (size_t)c * c) * 4;
}

// NULL when cms_calib_accumulate accepts the descriptor, else what is wrong with it
inline const char* calib_check(const cms_calib_desc* d) {
    if (!d) return "NULL descriptor";
    cms_tta_desc t;
    calib_tta_desc(d, &t);
    if (const char* why = tta_check_vote(&t)) return why;
    if (!d->labels) return "labels NULL";
    if (!d->hist) return "hist NULL";
    if (!d->scores) return "scores NULL";
    if (d->nb < 1 || d->nb > CMS_CALIB_MAX_BINS) return "1 <= nb <= 48 bins";
    if (d->nb > 1 && !d->edges) return "edges NULL";
    for (int j = 0; j + 1 < d->nb; ++j) {
        const float e = d->edges[j];
        if (!(e > 0.0f && e < 1.0f)) return "an edge outside (0, 1)";
        if (j > 0 && !(e > d->edges[j - 1])) return "edges not strictly ascending";
    }
    if (d->nt < 1 || d->nt > CMS_CALIB_MAX_TEMPS) return "1 <= nt <= 8 temperatures";
    if (!d->temps) return "temps NULL";
    for (int i = 0; i < d->nt; ++i) {
        const float T = d->temps[i];
        if (!(T > 0.0f) || !(T <= FLT_MAX)) return "a temperature that is not finite and > 0";
    }
    if (calib_lds_bytes(d->c, d->nb, d->k) > kCalibLdsLimit) return "the workgroup's tables do not fit the LDS";
    return nullptr;
}

inline void calib_make_params(const cms_calib_desc* d, CalibParams* p) {
    p->nb = d->nb, p->nt = d->nt;
    for (int j = 0; j < CMS_CALIB_MAX_BINS - 1; ++j) p->edges[j] = j + 1 < d->nb ? d->edges[j] : 2.0f;
    for (int i = 0; i < CMS_CALIB_MAX_TEMPS; ++i) {
        const bool on = i < d->nt;
        p->inv_t[i] = on ? 1.0f / d->temps[i] : 1.0f;            // rounded once, here
        p->scaled[i] = on && d->temps[i] != 1.0f;
    }
}

// a scored label, or -1: cms_tta_vote's rule
CMS_HD int calib_valid_label(int label, int ignore_index, int C) { return (label != ignore_index && label >= 0 && label < C) ? label : -1; }

// logit * (1 / T), a rounded product; the logit itself at T == 1
CMS_HD float calib_scale(float l, float inv_t, bool scaled) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float s = l * inv_t;
    return scaled ? s : l;
}

// one class' term of the squared error: (p - [hit])^2, two roundings
CMS_HD float calib_brier_term(float p, bool hit) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d = p - (hit ? 1.0f : 0.0f);
    const float q = d * d;
    return q;
}

CMS_HD float calib_nll_of_prob(float p) { return -logf(fmaxf(p, FLT_MIN)); }

// bin = #{ j : edge_j <= conf }: a confidence equal to an edge is in the upper bin, the trainers' `conf >= conf_thresh`
CMS_HD int calib_bin(const CalibParams& p, float conf) {
    int b = 0;
    for (int j = 0; j + 1 < p.nb; ++j) b += p.edges[j] <= conf ? 1 : 0;
    return b;
}

// rint(min(v, cap) * scale) as an integer >= 0 (scale a power of two: the product is exact); a NaN counts as the cap
CMS_HD unsigned long long calib_fx(float v, float scale, float cap) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float s = fminf(v, cap) * scale;
    if (!(s > 0.0f)) s = 0.0f;
    return (unsigned long long)rintf(s);
}

// what one scored pixel contributes; its NLL per temperature goes to a plain array of CMS_CALIB_MAX_TEMPS floats beside it (an
// array on its own is what the compiler keeps in registers under a run-time index; inside this struct it went to scratch)
struct CalibPixel {
    int pred;
    float conf, brier;
};

// One output pixel of a single view (k == 1). `label` < 0: the pixel is not scored and only the prediction is worked out.
template <bool IDENT>
CMS_HD void calib_single_pixel(const TtaViews& v, int n, int C, int y, int x, bool align_corners, int label, const CalibParams& p,
                               CalibPixel& out, float* nll) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    out.pred = tta_single_pixel<IDENT>(v, n, C, y, x, align_corners);
    if (label < 0) return;
    const int h = v.h[0], w = v.w[0];
    const size_t plane = (size_t)h * w;
    const float* base = v.logits[0] + (size_t)n * C * plane;
    Tap ty = {0, 0, 0.0f, 0.0f}, tx = {0, 0, 0.0f, 0.0f};
    size_t off = 0;
    if (IDENT) {
        off = (size_t)y * w + (v.flip[0] ? w - 1 - x : x);
    } else {
        ty = bilin_tap(y, v.sy[0], h, align_corners);
        tx = tta_tap_x(x, v.sx[0], w, align_corners, v.flip[0] != 0);
    }
    for (int t = 0; t < p.nt; ++t) {
        const float it = p.inv_t[t];
        const bool sc = p.scaled[t] != 0;
        auto l = [&](int c) {
            return calib_scale(IDENT ? base[c * plane + off] : bilin_gather(base + c * plane, w, ty, tx), it, sc);
        };
        if (t == 0) {
            SoftmaxRegs<0> s;
            softmax_regs<0>(l, C, s);
            out.conf = s.rz;                                           // consistency_pixel_fwd's conf
            float acc = 0.0f;
            for (int c = 0; c < C; ++c) acc += calib_brier_term(softmax_prob<0>(s, l, c), c == label);
            out.brier = acc;
            nll[0] = -((l(label) - s.mx) - logf(s.z));             // ce_pixel_fwd's expression on the statistics at hand
        } else {
            nll[t] = ce_pixel_fwd<0>(l, C, label);
        }
    }
}

// the mean probability of `label` over k >= 2 views at one temperature: tta_vote_pixel's walk for one class, no score table
CMS_HD float calib_label_prob(const TtaViews& v, int k, int n, int C, int y, int x, bool align_corners, int label, float inv_t,
                              bool scaled) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float sum = 0.0f;
    for (int i = 0; i < k; ++i) {
        const int h = v.h[i], w = v.w[i];
        const size_t plane = (size_t)h * w;
        const float* base = v.logits[i] + (size_t)n * C * plane;
        const Tap ty = bilin_tap(y, v.sy[i], h, align_corners);
        const Tap tx = tta_tap_x(x, v.sx[i], w, align_corners, v.flip[i] != 0);
        auto logit = [&](int c) { return calib_scale(bilin_gather(base + (size_t)c * plane, w, ty, tx), inv_t, scaled); };
        SoftmaxRegs<0> s;
        softmax_regs<0>(logit, C, s);
        const float pl = softmax_prob<0>(s, logit, label);
        sum = i == 0 ? pl : sum + pl;
    }
    return sum / (float)k;
}

// One output pixel of the vote over k >= 2 views; `score(c)` as in tta_vote_pixel.
template <class S>
CMS_HD void calib_vote_pixel(const TtaViews& v, int k, int n, int C, int y, int x, bool align_corners, int label, const CalibParams& p,
                             S score, CalibPixel& out, float* nll) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float it = p.inv_t[0];
    const bool sc = p.scaled[0] != 0;
    out.pred = tta_vote_pixel_x(v, k, n, C, y, x, align_corners, score, [&](float l) { return calib_scale(l, it, sc); });
    if (label < 0) return;
    const float kf = (float)k;
    out.conf = fminf(score(out.pred) / kf, 1.0f);
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) acc += calib_brier_term(score(c) / kf, c == label);
    out.brier = acc;
    nll[0] = calib_nll_of_prob(score(label) / kf);
    for (int t = 1; t < p.nt; ++t)
        nll[t] = calib_nll_of_prob(calib_label_prob(v, k, n, C, y, x, align_corners, label, p.inv_t[t], p.scaled[t] != 0));
}

}  // namespace cms
