// Sliding-window evaluation (csrc/window.hip): descriptor validation, the window grid of a view, the windows that cover a pixel in
// closed form, and the per-pixel stitch. Everything here is plain C++ / `__host__ __device__`, so tests/hostcheck_window drives the
// very code the kernels are made of on the host; the product never runs it there. Taps, gathers and the softmax are pixel_math.hpp's,
// the view reads and the argmax rule tta_math.hpp's, under the same `fp contract(off)` discipline. include/cutmixseg.h states the
// definition.
#pragma once
#include "tta_math.hpp"

namespace cms {

// what the kernel reads per view: the descriptor's pointers and sizes plus the two tap scales, worked out once on the host. A view
// of one window (gy * gx == 1) carries the scales of cms_tta_vote (view -> canvas), any other the scales window logits -> window.
struct WinViews {
    const float* logits[CMS_TTA_MAX_VIEWS];
    int hl[CMS_TTA_MAX_VIEWS], wl[CMS_TTA_MAX_VIEWS], Hv[CMS_TTA_MAX_VIEWS], Wv[CMS_TTA_MAX_VIEWS];
    int gy[CMS_TTA_MAX_VIEWS], gx[CMS_TTA_MAX_VIEWS], eh[CMS_TTA_MAX_VIEWS], ew[CMS_TTA_MAX_VIEWS];
    int sh[CMS_TTA_MAX_VIEWS], sw[CMS_TTA_MAX_VIEWS], flip[CMS_TTA_MAX_VIEWS];
    float sy[CMS_TTA_MAX_VIEWS], sx[CMS_TTA_MAX_VIEWS];
};

// ---------------------------------------------------------------------------------------------- the grid of one axis
CMS_HD int win_extent(int view, int window) { return window < view ? window : view; }

// ceil((view - window) / stride) + 1 windows, one when the window holds the view; view, window, stride >= 1
CMS_HD int win_count(int view, int window, int stride) {
    if (view <= window) return 1;
    return (int)(((long long)view - window + stride - 1) / stride) + 1;
}

CMS_HD int win_origin(int j, int stride, int view, int extent) {
    const long long o = (long long)j * stride;
    const int last = view - extent;
    return o < last ? (int)o : last;
}

// the view row (column) of canvas row (column) `y`: the row whose centre band holds the centre of y; y itself when view == canvas
CMS_HD int win_view_coord(int y, int view, int canvas) {
    const long long r = ((2LL * y + 1) * view) / (2LL * canvas);
    return r > view - 1 ? view - 1 : (int)r;
}

// The windows lo..hi (inclusive, never empty) of an axis that hold coordinate r, 0 <= r < view. Windows 0 .. g - 2 start at
// j * stride; the last one starts at view - extent <= (g - 1) * stride and holds r exactly when r >= view - extent. Of the regular
// ones j holds r when j * stride <= r < j * stride + extent. stride <= extent leaves no gap, so the set is one range.
struct WinRange {
    int lo, hi;
};

CMS_HD WinRange win_cover(int r, int view, int extent, int stride, int g) {
    WinRange c;
    c.lo = r >= extent ? (r - extent) / stride + 1 : 0;
    if (r >= view - extent) {
        c.hi = g - 1;
    } else {
        const int q = r / stride;
        c.hi = q < g - 2 ? q : g - 2;
    }
    return c;
}

// ---------------------------------------------------------------------------------------------- descriptor checks
// NULL when (window, stride) is a window this project evaluates with, else what is wrong
inline const char* win_check_axis(int window, int stride) {
    if (window < 1) return "a window below 1";
    if (stride < 1) return "a stride below 1";
    if (stride > window) return "a stride above its window (pixels would be left out)";
    if (stride < (window + 3) / 4) return "a stride below ceil(window / 4)";
    return nullptr;
}

// the logits of one view: n * G * c * hl * wl <= 2^31 - 1
inline bool win_logits_ok(int n, int gy, int gx, int c, int hl, int wl) {
    unsigned long long p = 1;
    const int f[6] = {n, gy, gx, c, hl, wl};
    for (int i = 0; i < 6; ++i) {
        p *= (unsigned long long)f[i];          // < 2^31 * 2^31
        if (p > (unsigned long long)kTtaMaxElems) return false;
    }
    return true;
}

// the cms_tta_desc of the same views read whole: what cms_window_vote forwards when no view has more than one window, and what
// carries cms_tta_vote's own refusals
inline void win_tta_desc(const cms_window_desc* d, cms_tta_desc* t) {
    for (int i = 0; i < CMS_TTA_MAX_VIEWS; ++i) {
        t->logits[i] = d->logits[i];
        t->h[i] = d->hl[i], t->w[i] = d->wl[i], t->flip[i] = d->flip[i];
    }
    t->n = d->n, t->c = d->c, t->H = d->H, t->W = d->W, t->k = d->k, t->align_corners = d->align_corners;
    t->labels = d->labels, t->label_dtype = d->label_dtype, t->ignore_index = d->ignore_index;
    t->cm = d->cm, t->pred_out = d->pred_out;
}

// NULL when cms_window_vote accepts the descriptor, else what is wrong with it
inline const char* win_check_vote(const cms_window_desc* d) {
    if (!d) return "NULL descriptor";
    cms_tta_desc t;
    win_tta_desc(d, &t);
    if (const char* why = tta_check_vote(&t)) return why;
    if (d->wh < 1 || d->ww < 1) return "a window below 1";
    for (int i = 0; i < d->k; ++i) {
        if (d->Hv[i] < 1 || d->Wv[i] < 1) return "bad geometry (a view below 1 x 1)";
        if (const char* why = win_check_axis(d->wh, d->sh[i])) return why;
        if (const char* why = win_check_axis(d->ww, d->sw[i])) return why;
        if (d->eh[i] != win_extent(d->Hv[i], d->wh) || d->ew[i] != win_extent(d->Wv[i], d->ww))
            return "eh / ew is not min(window, view)";
        if (d->gy[i] != win_count(d->Hv[i], d->wh, d->sh[i]) || d->gx[i] != win_count(d->Wv[i], d->ww, d->sw[i]))
            return "gy / gx does not follow from the view, the window and the stride";
        if (d->hl[i] > d->eh[i] || d->wl[i] > d->ew[i]) return "logits larger than their window";
        if (!win_logits_ok(d->n, d->gy[i], d->gx[i], d->c, d->hl[i], d->wl[i])) return "more than 2^31 - 1 logits in a view";
    }
    return nullptr;
}

// does the call forward to cms_tta_vote? (no view has more than one window)
inline bool win_all_single(const cms_window_desc* d) {
    for (int i = 0; i < d->k; ++i)
        if (d->gy[i] != 1 || d->gx[i] != 1) return false;
    return true;
}

// NULL when cms_window_crop accepts its arguments, else what is wrong with them
inline const char* win_check_crop(const void* src, const void* dst, int n, int c, int H, int W, int Hv, int Wv, int wh, int ww, int sh,
                                  int sw, int dtype) {
    if (!src || !dst) return "NULL pointer";
    if (n < 1 || c < 1 || H < 1 || W < 1 || Hv < 1 || Wv < 1) return "bad geometry";
    if (dtype != CMS_F32 && dtype != CMS_BF16) return "bad dtype";
    if (const char* why = win_check_axis(wh, sh)) return why;
    if (const char* why = win_check_axis(ww, sw)) return why;
    if (!tta_count_ok(n, c, H, W)) return "more than 2^31 - 1 elements";
    // n * c * (gy * eh) * (gx * ew): gy * eh < 2^31 * 2^31 before the bound is applied factor by factor
    if (!win_logits_ok(n, win_count(Hv, wh, sh), win_count(Wv, ww, sw), c, win_extent(Hv, wh), win_extent(Wv, ww)))
        return "more than 2^31 - 1 elements";
    return nullptr;
}

inline void win_make_views(const cms_window_desc* d, WinViews* v) {
    const bool align = d->align_corners != 0;
    for (int i = 0; i < CMS_TTA_MAX_VIEWS; ++i) {
        const bool on = i < d->k;
        v->logits[i] = on ? d->logits[i] : nullptr;
        v->hl[i] = on ? d->hl[i] : 1, v->wl[i] = on ? d->wl[i] : 1;
        v->Hv[i] = on ? d->Hv[i] : 1, v->Wv[i] = on ? d->Wv[i] : 1;
        v->gy[i] = on ? d->gy[i] : 1, v->gx[i] = on ? d->gx[i] : 1;
        v->eh[i] = on ? d->eh[i] : 1, v->ew[i] = on ? d->ew[i] : 1;
        v->sh[i] = on ? d->sh[i] : 1, v->sw[i] = on ? d->sw[i] : 1;
        v->flip[i] = on ? (d->flip[i] != 0) : 0;
        const bool single = on && d->gy[i] == 1 && d->gx[i] == 1;
        v->sy[i] = !on ? 0.0f : bilin_scale(d->hl[i], single ? d->H : d->eh[i], align);
        v->sx[i] = !on ? 0.0f : bilin_scale(d->wl[i], single ? d->W : d->ew[i], align);
    }
}

// ---------------------------------------------------------------------------------------------- the stitch
// One canvas pixel -> its prediction. `score(c)` is a float lvalue per class (a column of LDS in the kernel, an array on the host).
// Views outermost and, inside a view, its covering windows in row-major order, so a window's taps and softmax statistics live in
// registers and the score comes out as ((q_0 + q_1) + q_2) + ..., q = p of a whole view or p / cnt of a window.
template <class S>
CMS_HD int win_vote_pixel(const WinViews& v, int k, int n, int C, int H, int W, int y, int x, bool align_corners, S score) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    bool first = true;
    for (int i = 0; i < k; ++i) {
        const int hl = v.hl[i], wl = v.wl[i], gy = v.gy[i], gx = v.gx[i];
        const size_t plane = (size_t)hl * wl;
        if (gy == 1 && gx == 1) {
            // the whole view is one window: tta_vote_pixel's read
            const float* base = v.logits[i] + (size_t)n * C * plane;
            const Tap ty = bilin_tap(y, v.sy[i], hl, align_corners);
            const Tap tx = tta_tap_x(x, v.sx[i], wl, align_corners, v.flip[i] != 0);
            auto logit = [&](int c) { return bilin_gather(base + (size_t)c * plane, wl, ty, tx); };
            SoftmaxRegs<0> s;
            softmax_regs<0>(logit, C, s);
            for (int c = 0; c < C; ++c) {
                const float p = softmax_prob<0>(s, logit, c);
                if (first) score(c) = p;
                else score(c) = score(c) + p;
            }
            first = false;
            continue;
        }
        const int Hv = v.Hv[i], Wv = v.Wv[i], eh = v.eh[i], ew = v.ew[i], sh = v.sh[i], sw = v.sw[i];
        const int ry = win_view_coord(y, Hv, H);
        int rx = win_view_coord(x, Wv, W);
        if (v.flip[i]) rx = Wv - 1 - rx;
        const WinRange cy = win_cover(ry, Hv, eh, sh, gy), cx = win_cover(rx, Wv, ew, sw, gx);
        const float cnt = (float)((cy.hi - cy.lo + 1) * (cx.hi - cx.lo + 1));
        for (int j = cy.lo; j <= cy.hi; ++j) {
            const Tap ty = bilin_tap(ry - win_origin(j, sh, Hv, eh), v.sy[i], hl, align_corners);
            for (int ii = cx.lo; ii <= cx.hi; ++ii) {
                const Tap tx = bilin_tap(rx - win_origin(ii, sw, Wv, ew), v.sx[i], wl, align_corners);
                const size_t item = ((size_t)n * gy + j) * gx + ii;
                const float* base = v.logits[i] + item * C * plane;
                auto logit = [&](int c) { return bilin_gather(base + (size_t)c * plane, wl, ty, tx); };
                SoftmaxRegs<0> s;
                softmax_regs<0>(logit, C, s);
                for (int c = 0; c < C; ++c) {
                    const float q = softmax_prob<0>(s, logit, c) / cnt;
                    if (first) score(c) = q;
                    else score(c) = score(c) + q;
                }
                first = false;
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

// ---------------------------------------------------------------------------------------------- the crop
// Where element `idx` of the window batch (n * gy * gx, c, eh, ew) of a view lies in the view: sample, channel, row and STORED
// column (the column of the mirrored view when it is mirrored).
struct WinCropAt {
    size_t plane;      // n * c + ch: the source plane
    int vy, vx;
};

CMS_HD WinCropAt win_crop_at(size_t idx, int c, int Hv, int Wv, int gy, int gx, int eh, int ew, int sh, int sw) {
    const int x = (int)(idx % ew);
    size_t t = idx / ew;
    const int y = (int)(t % eh);
    t /= eh;
    const int ch = (int)(t % c);
    t /= c;
    const int i = (int)(t % gx);
    t /= gx;
    const int j = (int)(t % gy);
    const size_t n = t / gy;
    WinCropAt a;
    a.plane = n * c + ch;
    a.vy = win_origin(j, sh, Hv, eh) + y;
    a.vx = win_origin(i, sw, Wv, ew) + x;
    return a;
}

// one element of cms_window_crop: the element (vy, vx) of cms_tta_resize's view, `ld(i)` being element i of the source plane
template <class L>
CMS_HD float win_crop_pixel(L ld, int H, int W, int Hv, int Wv, int flip, int vy, int vx) {
    return tta_resize_pixel(ld, H, W, Hv, Wv, vy, flip ? Wv - 1 - vx : vx);
}

}  // namespace cms
