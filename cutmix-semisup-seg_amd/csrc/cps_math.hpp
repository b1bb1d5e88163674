// Cross pseudo supervision labels (csrc/cps.hip): descriptor validation, the launch geometry and the per-pixel / per-thread arithmetic.
// Everything here is plain C++ / `__host__ __device__`, so tests/hostcheck_cps drives the very code the kernel is made of on the
// host; the product never runs it there. Taps, gathers, the box parity and the softmax are pixel_math.hpp's, the argmax order
// tta_math.hpp's, under their `fp contract(off)` discipline: nothing of them is restated here.
//
// Per output pixel p = (y, x) of sample n, for the two networks k = a, b:
//   m          "take image 1": box_mask_bit(ranges[n], y, x, invert) with a box table, mask[n, y, x] >= 0.5 with a mask
//   u_k(c)     the bilinear sample at p of l1_k[n, c] if m, else of l0_k[n, c] (read without interpolation when (h, w) == (H, W))
//   pred_k     argmax_c u_k(c): larger wins, the first index keeps a tie, NaN counts as maximal
//   conf_k     softmax(u_k)[pred_k]
//   valid      (m ? um1 : um0)[n, y, x] >= 0.5, a NULL map counting as all valid
//   label_k    pred_k if valid and (tau <= 0 or conf_k >= tau), else 255
//   stats      n_valid, kept_a, kept_b (labels != 255), agree (valid pixels with pred_a == pred_b, whatever tau is)
// The mask bit, the validity and the taps are worked out once per pixel and serve all four logit tensors.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/cutmixseg.h"
#include "classmix_math.hpp"

namespace cms {

constexpr int kCpsBlock = 256;          // threads per workgroup
constexpr int kCpsMaxSamples = 65535;   // blockIdx.y is the sample
constexpr int kCpsIgnore = 255;

// the descriptor plus the two scales, worked out once on the host
struct CpsArgs {
    cms_cps_desc d;
    float sy, sx;
};

struct CpsCounts {
    int n_valid, kept_a, kept_b, agree;
};

// NULL when cms_cps_labels accepts the descriptor, else what is wrong with it
inline const char* cps_check(const cms_cps_desc* d) {
    if (!d) return "NULL descriptor";
    if (!d->l0_a || !d->l1_a || !d->l0_b || !d->l1_b) return "logits NULL";
    if (!d->label_a || !d->label_b) return "label output NULL";
    if (!d->stats) return "stats NULL";
    if (d->c < 1 || d->c > kTtaMaxClasses) return "1 <= num_classes <= 64";
    if (d->n < 1 || d->h < 1 || d->w < 1 || d->H < 1 || d->W < 1) return "bad geometry (n, h, w, H, W >= 1)";
    if (d->n > kCpsMaxSamples) return "more than 65535 samples";
    if (d->h > d->H || d->w > d->W) return "logits larger than the output (h <= H, w <= W)";
    if (!tta_count_ok(d->n, d->H, d->W)) return "more than 2^31 - 1 output pixels";
    if (!tta_count_ok(d->n, d->c, d->h, d->w)) return "more than 2^31 - 1 logits";
    if ((d->ranges != nullptr) == (d->mask != nullptr)) return "exactly one of ranges / mask";
    if (d->ranges && d->n_boxes < 1) return "ranges without a box (n_boxes >= 1)";
    if (d->ranges && !tta_count_ok(d->n, d->n_boxes, 4)) return "more than 2^31 - 1 range entries";
    if (((uintptr_t)d->stats & 7) != 0) return "stats not 8-byte aligned";
    return nullptr;
}

inline void cps_make_args(const cms_cps_desc* d, CpsArgs* a) {
    a->d = *d;
    a->sy = bilin_scale(d->h, d->H, d->align_corners != 0);
    a->sx = bilin_scale(d->w, d->W, d->align_corners != 0);
}

// Workgroups per sample: a thread owns one group of four labels whose FLAT index (over the whole (n, H, W) tensor) is a multiple of
// four -- classmix_split's groups --, and a sample has at most H * W / 4 of them whatever its start is; the at most three labels
// before the first group and after the last are workgroup 0's. A workgroup never straddles two samples.
inline unsigned cps_blocks(long long hw) {
    const long long groups = hw / 4;
    const long long b = (groups + kCpsBlock - 1) / kCpsBlock;
    return (unsigned)(b < 1 ? 1 : b);
}

// the specialised class counts: the logits of a pixel are gathered ONCE into registers (Pascal VOC's 21, Cityscapes' 19); any other
// count re-gathers per use (CT == 0). The arithmetic is the same functions in the same order either way.
inline int cps_ct(int c) { return (c == 19 || c == 21) ? c : 0; }

// One network's pixel: `base` is sample n of the tensor the mask bit chose. -> the prediction; `confident`: tau <= 0 or conf >= tau
// (a NaN confidence fails the comparison).
template <int CT, bool IDENT>
CMS_HD int cps_net_pixel(const float* base, int crt, int w, size_t plane, size_t off, const Tap& ty, const Tap& tx, float tau,
                         bool& confident) {
    const int C = CT > 0 ? CT : crt;
    float u[CT > 0 ? CT : 1];
    auto gather = [&](int c) { return IDENT ? base[(size_t)c * plane + off] : bilin_gather(base + (size_t)c * plane, w, ty, tx); };
    if (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) u[c] = gather(c);
    }
    auto logit = [&](int c) { return CT > 0 ? u[CT > 0 ? c : 0] : gather(c); };
    int best = 0;
    float bv = logit(0);
#pragma unroll
    for (int c = 1; c < C; ++c) {
        const float v = logit(c);
        if (tta_beats(v, bv)) {
            bv = v;
            best = c;
        }
    }
    confident = true;
    if (tau > 0.0f) {
        SoftmaxRegs<CT> s;
        softmax_regs<CT>(logit, crt, s);
        float conf = 0.0f;
        if (CT > 0) {
            // (a register array is indexed by constants only: pick the winner's probability in an unrolled loop)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float p = softmax_prob<CT>(s, logit, c);
                if (c == best) conf = p;
            }
        } else {
            conf = softmax_prob<CT>(s, logit, best);
        }
        confident = conf >= tau;
    }
    return best;
}

// One output pixel: both labels, and what it adds to the counts. An invalid pixel reads no logits.
template <int CT, bool IDENT>
CMS_HD void cps_pixel(const CpsArgs& a, int n, int y, int x, uint8_t& la, uint8_t& lb, CpsCounts& k) {
    const cms_cps_desc& d = a.d;
    const size_t q = ((size_t)n * d.H + y) * d.W + x;
    const bool m = d.ranges ? box_mask_bit(d.ranges + (size_t)n * d.n_boxes * 4, d.n_boxes, y, x, d.invert != 0) : d.mask[q] >= 0.5f;
    const float* um = m ? d.um1 : d.um0;
    const bool valid = um ? um[q] >= 0.5f : true;
    la = lb = (uint8_t)kCpsIgnore;
    if (!valid) return;
    const bool align = d.align_corners != 0;
    const size_t plane = (size_t)d.h * d.w, sample = (size_t)n * d.c * plane;
    Tap ty = {0, 0, 0.0f, 0.0f}, tx = {0, 0, 0.0f, 0.0f};
    size_t off = 0;
    if (IDENT) {
        off = (size_t)y * d.w + x;
    } else {
        ty = bilin_tap(y, a.sy, d.h, align);
        tx = bilin_tap(x, a.sx, d.w, align);
    }
    bool ca, cb;
    const int pa = cps_net_pixel<CT, IDENT>((m ? d.l1_a : d.l0_a) + sample, d.c, d.w, plane, off, ty, tx, d.conf_thresh, ca);
    const int pb = cps_net_pixel<CT, IDENT>((m ? d.l1_b : d.l0_b) + sample, d.c, d.w, plane, off, ty, tx, d.conf_thresh, cb);
    if (ca) la = (uint8_t)pa;
    if (cb) lb = (uint8_t)pb;
    k.n_valid += 1;
    k.kept_a += ca ? 1 : 0;
    k.kept_b += cb ? 1 : 0;
    k.agree += pa == pb ? 1 : 0;
}

// What thread `tid` of workgroup `block` of sample n does: its group of four labels (one 4-byte store per map with VEC: the label
// pointers are 4-byte aligned), and in workgroup 0 one label of the sample's head or tail. Adds to `k`.
template <int CT, bool IDENT, bool VEC>
CMS_HD void cps_thread(const CpsArgs& a, int n, unsigned block, int tid, CpsCounts& k) {
    const cms_cps_desc& d = a.d;
    const size_t hw = (size_t)d.H * d.W, start = (size_t)n * hw, end = start + hw;
    const CmSplit sp = classmix_split(start, end);
    auto one = [&](size_t i, uint8_t& la, uint8_t& lb) {
        const size_t p = i - start;
        const int y = (int)(p / d.W), x = (int)(p - (size_t)y * d.W);
        cps_pixel<CT, IDENT>(a, n, y, x, la, lb, k);
    };
    const size_t g = sp.vec_lo / 4 + (size_t)block * kCpsBlock + tid;
    if (g < sp.vec_hi / 4) {
        uint8_t la[4], lb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) one(4 * g + j, la[j], lb[j]);
        if (VEC) {
            reinterpret_cast<uint32_t*>(d.label_a)[g] = (uint32_t)la[0] | (uint32_t)la[1] << 8 | (uint32_t)la[2] << 16 | (uint32_t)la[3] << 24;
            reinterpret_cast<uint32_t*>(d.label_b)[g] = (uint32_t)lb[0] | (uint32_t)lb[1] << 8 | (uint32_t)lb[2] << 16 | (uint32_t)lb[3] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) d.label_a[4 * g + j] = la[j], d.label_b[4 * g + j] = lb[j];
        }
    }
    if (block == 0) {      // at most three labels before the first group and three after the last
        const size_t head = sp.vec_lo - start, tail = end - sp.vec_hi;
        size_t i = end;
        if ((size_t)tid < head) i = start + tid;
        else if ((size_t)tid - head < tail) i = sp.vec_hi + ((size_t)tid - head);
        if (i < end) {
            uint8_t la, lb;
            one(i, la, lb);
            d.label_a[i] = la, d.label_b[i] = lb;
        }
    }
}

}  // namespace cms
