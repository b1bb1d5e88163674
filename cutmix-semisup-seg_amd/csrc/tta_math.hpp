// Test-time augmentation (csrc/tta.hip): descriptor validation, view geometry and the per-pixel vote. Everything here is plain C++ /
// `__host__ __device__`, so tests/hostcheck_tta drives the very code the kernels are made of on the host; the product never runs it
// there. Taps, gathers and the softmax are pixel_math.hpp's, under the same `fp contract(off)` discipline.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/cutmixseg.h"
#include "pixel_math.hpp"

namespace cms {

constexpr int kTtaMaxClasses = 64;
constexpr long long kTtaMaxElems = 0x7fffffffLL;

// what the kernel reads per view: the descriptor's pointers and sizes plus the two scales, worked out once on the host
struct TtaViews {
    const float* logits[CMS_TTA_MAX_VIEWS];
    int h[CMS_TTA_MAX_VIEWS], w[CMS_TTA_MAX_VIEWS], flip[CMS_TTA_MAX_VIEWS];
    float sy[CMS_TTA_MAX_VIEWS], sx[CMS_TTA_MAX_VIEWS];
};

// a * b * c (all >= 1) <= kTtaMaxElems, without overflow whatever the ints are
inline bool tta_count_ok(int a, int b, int c, int d = 1) {
    unsigned long long p = (unsigned long long)a;
    const int rest[3] = {b, c, d};
    for (int i = 0; i < 3; ++i) {
        p *= (unsigned long long)rest[i];           // < 2^31 * 2^31 = 2^62
        if (p > (unsigned long long)kTtaMaxElems) return false;
    }
    return true;
}

// NULL when cms_tta_vote accepts the descriptor, else what is wrong with it
inline const char* tta_check_vote(const cms_tta_desc* d) {
    if (!d) return "NULL descriptor";
    if (d->k < 1 || d->k > CMS_TTA_MAX_VIEWS) return "1 <= k <= 16 views";
    if (d->c < 1 || d->c > kTtaMaxClasses) return "1 <= num_classes <= 64";
    if (d->n < 1 || d->H < 1 || d->W < 1) return "bad geometry (n, H, W >= 1)";
    for (int i = 0; i < d->k; ++i) {
        if (d->h[i] < 1 || d->w[i] < 1) return "bad geometry (a view below 1 x 1)";
        if (!d->logits[i]) return "logits NULL";
    }
    if (d->cm && !d->labels) return "cm given without labels";
    if (!d->cm && !d->pred_out) return "nothing to produce (cm and pred_out NULL)";
    if (d->labels && d->label_dtype != CMS_LABEL_U8 && d->label_dtype != CMS_LABEL_I64) return "bad label dtype";
    if (!tta_count_ok(d->n, d->H, d->W)) return "more than 2^31 - 1 output pixels";
    return nullptr;
}

inline const char* tta_check_resize(const void* src, const void* dst, int n, int c, int H, int W, int Hs, int Ws, int dtype) {
    if (!src || !dst) return "NULL pointer";
    if (n < 1 || c < 1 || H < 1 || W < 1 || Hs < 1 || Ws < 1) return "bad geometry";
    if (dtype != CMS_F32 && dtype != CMS_BF16) return "bad dtype";
    if (!tta_count_ok(n, c, H, W) || !tta_count_ok(n, c, Hs, Ws)) return "more than 2^31 - 1 elements";
    return nullptr;
}

inline void tta_make_views(const cms_tta_desc* d, TtaViews* v) {
    for (int i = 0; i < CMS_TTA_MAX_VIEWS; ++i) {
        const bool on = i < d->k;
        v->logits[i] = on ? d->logits[i] : nullptr;
        v->h[i] = on ? d->h[i] : 1;
        v->w[i] = on ? d->w[i] : 1;
        v->flip[i] = on ? (d->flip[i] != 0) : 0;
        v->sy[i] = on ? bilin_scale(d->h[i], d->H, d->align_corners != 0) : 0.0f;
        v->sx[i] = on ? bilin_scale(d->w[i], d->W, d->align_corners != 0) : 0.0f;
    }
}

// x taps of a view; a flipped view is un-mirrored: the taps point at the mirrored columns, the weights stay
CMS_HD Tap tta_tap_x(int x, float sx, int w, bool align_corners, bool flip) {
    Tap t = bilin_tap(x, sx, w, align_corners);
    if (flip) {
        t.i0 = w - 1 - t.i0;
        t.i1 = w - 1 - t.i1;
    }
    return t;
}

// the label of pixel `pix` as an int; an int64 label outside [0, 2^31) is -1 (never a class)
CMS_HD int tta_label(const void* labels, int label_dtype, size_t pix) {
    if (label_dtype == CMS_LABEL_U8) return (int)((const uint8_t*)labels)[pix];
    const int64_t v = ((const int64_t*)labels)[pix];
    return (v < 0 || v > 0x7fffffff) ? -1 : (int)v;
}

// torch.argmax's order on two candidates: larger wins, the first index keeps a tie, NaN counts as maximal (csrc/eval.hip)
CMS_HD bool tta_beats(float v, float best) { return v > best || (v != v && best == best); }

// One output pixel of a single view (k == 1): the argmax of its logits, csrc/eval.hip's loop. IDENT: the view has the output's size
// and is read without interpolation.
template <bool IDENT>
CMS_HD int tta_single_pixel(const TtaViews& v, int n, int C, int y, int x, bool align_corners) {
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
    int best = 0;
    float bv = IDENT ? base[off] : bilin_gather(base, w, ty, tx);
    for (int c = 1; c < C; ++c) {
        const float val = IDENT ? base[c * plane + off] : bilin_gather(base + c * plane, w, ty, tx);
        if (tta_beats(val, bv)) {
            bv = val;
            best = c;
        }
    }
    return best;
}

// One output pixel of the vote over k >= 2 views -> its prediction. `score(c)` is a float lvalue per class (a column of LDS in the
// kernel, an array on the host); views outermost, so a view's taps and softmax statistics live in registers and
// score_c = ((p_0c + p_1c) + p_2c) + ... comes out in view order.
// `xf(logit)` is applied to every gathered logit before the softmax: the identity in the vote, the temperature scaling of
// csrc/calib_math.hpp.
template <class S, class X>
CMS_HD int tta_vote_pixel_x(const TtaViews& v, int k, int n, int C, int y, int x, bool align_corners, S score, X xf) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int i = 0; i < k; ++i) {
        const int h = v.h[i], w = v.w[i];
        const size_t plane = (size_t)h * w;
        const float* base = v.logits[i] + (size_t)n * C * plane;
        const Tap ty = bilin_tap(y, v.sy[i], h, align_corners);
        const Tap tx = tta_tap_x(x, v.sx[i], w, align_corners, v.flip[i] != 0);
        auto logit = [&](int c) { return xf(bilin_gather(base + (size_t)c * plane, w, ty, tx)); };
        SoftmaxRegs<0> s;
        softmax_regs<0>(logit, C, s);
        if (i == 0) {
            for (int c = 0; c < C; ++c) score(c) = softmax_prob<0>(s, logit, c);
        } else {
            for (int c = 0; c < C; ++c) {
                const float p = softmax_prob<0>(s, logit, c);
                score(c) = score(c) + p;
            }
        }
    }
    int best = 0;
    float bv = score(0);
    for (int c = 1; c < C; ++c) {
        const float sc = score(c);
        if (tta_beats(sc, bv)) {
            bv = sc;
            best = c;
        }
    }
    return best;
}

template <class S>
CMS_HD int tta_vote_pixel(const TtaViews& v, int k, int n, int C, int y, int x, bool align_corners, S score) {
    return tta_vote_pixel_x(v, k, n, C, y, x, align_corners, score, [](float l) { return l; });
}

// The align_corners=False tap of output index `dst` with its position worked out exactly: src = (dst + 0.5) * in / out - 0.5
// = ((2 dst + 1) in - out) / (2 out) in integers, clamped at 0; only the weight is rounded (three roundings of a number <= 1).
// bilin_tap places the sample in fp32: at a source size of 33 .. 47 that moves it by a few 1e-6 of a pixel -- harmless where the
// same taps are used on both sides of a comparison (the loss and evaluation kernels), but on N(0,1) data it moves the resized
// value by up to 1e-5, more than the resize is held to against its fp64 restatement (tests/test_gpu_tta.py).
CMS_HD Tap tta_tap_exact(int dst, int in_size, int out_size) {
    const long long num = (2LL * dst + 1) * in_size - out_size, den = 2LL * out_size;
    Tap t;
    if (num <= 0) {
        t.i0 = 0;
        t.w1 = 0.0f;
    } else {
        const long long q = num / den;
        t.i0 = q > in_size - 1 ? in_size - 1 : (int)q;
        t.w1 = (float)(num - q * den) / (float)den;
    }
    t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
    t.w0 = 1.0f - t.w1;
    return t;
}

// One output element of cms_tta_resize: `ld(i)` is element i of the source plane as fp32. bilin_gather's expression on a loader.
template <class L>
CMS_HD float tta_resize_pixel(L ld, int H, int W, int Hs, int Ws, int y, int x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const Tap ty = tta_tap_exact(y, H, Hs);
    const Tap tx = tta_tap_exact(x, W, Ws);
    const size_t r0 = (size_t)ty.i0 * W, r1 = (size_t)ty.i1 * W;
    const float a = fmaf(tx.w1, ld(r0 + tx.i1), tx.w0 * ld(r0 + tx.i0));
    const float b = fmaf(tx.w1, ld(r1 + tx.i1), tx.w0 * ld(r1 + tx.i0));
    return fmaf(ty.w1, b, ty.w0 * a);
}

}  // namespace cms
