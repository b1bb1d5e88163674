// Per-pixel arithmetic of the augmentation-consistency loss (the classic mean teacher between two differently augmented
// views), shared by the kernels of aug_loss.hip and driven on the host by tests/hostcheck_aug. Same conventions as
// pixel_math.hpp / ict_math.hpp: `__host__ __device__`, compile-time class count with the class axis in registers,
// contraction off and explicit fmaf where two evaluations of the same expression must agree bit for bit (a pixel's target is
// computed by the forward and the backward launch, from LDS or from global memory).
//
// Reference behaviour restated here (train_seg_semisup_aug_mt.py of the upstream repository):
//   warp                 :302        F.affine_grid(xf0_to_1, align_corners=True) + the un-normalisation of F.grid_sample,
//                                    folded on the host into ONE pixel-space matrix per sample (ops.aug_pixel_matrices)
//   sampling             :304-312    F.grid_sample(bilinear, zero padding): four taps, weights not renormalised
//   teacher in student   :304, 309, 312   warped logits / warped softmax; the teacher's full-resolution logits are themselves
//                                    the bilinear upsample of its low-resolution head output (bilin_tap / bilin_gather)
//   loss mask            :306        grid_sample(um0) * um1
//   confidence           :347        max_c of the WARPED probabilities
//   consistency losses   :366-387    with the warped targets; `logits_var` as evidently intended (the reference's branch raises:
//                                    it reads `delta_prob` before assignment): sum_c (delta logits)^2 / sqrt(C)
#pragma once
#include "pixel_math.hpp"

namespace cms {

// The four grid_sample taps of one student pixel: teacher pixels (Y0 + (k >> 1), X0 + (k & 1)), k = 0..3 (nw, ne, sw, se), with
// weight w[k]; w[k] == 0 marks a tap that contributes nothing (outside the image: zero padding, or weight zero). Only taps with
// w[k] != 0 may be dereferenced: those have 0 <= X <= W-1 and 0 <= Y <= H-1.
struct AugTaps {
    int X0, Y0;
    float w[4];
};

// student pixel (x, y) of view 1 -> sampling position in the teacher's full-resolution map of view 0; xf = [a00 a01 a02 a10 a11 a12]
CMS_HD void aug_map(const float* xf, int x, int y, float& ix, float& iy) {
    ix = fmaf(xf[0], (float)x, fmaf(xf[1], (float)y, xf[2]));
    iy = fmaf(xf[3], (float)x, fmaf(xf[4], (float)y, xf[5]));
}

// clamp to [-2, size + 1]: every position out there has both taps outside, and the float -> int conversion below is defined
// for any input. A NaN fails both comparisons' negations and lands on -2: outside.
CMS_HD float aug_clamp(float v, int size) {
    if (!(v >= -2.0f)) v = -2.0f;
    if (!(v <= (float)(size + 1))) v = (float)(size + 1);
    return v;
}

CMS_HD AugTaps aug_taps(const float* xf, int x, int y, int H, int W) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float ix, iy;
    aug_map(xf, x, y, ix, iy);
    ix = aug_clamp(ix, W);
    iy = aug_clamp(iy, H);
    const float fx = floorf(ix), fy = floorf(iy);
    AugTaps t;
    t.X0 = (int)fx;
    t.Y0 = (int)fy;
    // grid_sample: nw = (x_se - ix) * (y_se - iy), ne = (ix - x_sw) * (y_sw - iy), sw = (x_ne - ix) * (iy - y_ne), se = ...
    const float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix;
    const float wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    const bool x0in = t.X0 >= 0 && t.X0 <= W - 1, x1in = t.X0 + 1 >= 0 && t.X0 + 1 <= W - 1;
    const bool y0in = t.Y0 >= 0 && t.Y0 <= H - 1, y1in = t.Y0 + 1 >= 0 && t.Y0 + 1 <= H - 1;
    t.w[0] = (x0in && y0in) ? wx0 * wy0 : 0.0f;
    t.w[1] = (x1in && y0in) ? wx1 * wy0 : 0.0f;
    t.w[2] = (x0in && y1in) ? wx0 * wy1 : 0.0f;
    t.w[3] = (x1in && y1in) ? wx1 * wy1 : 0.0f;
    return t;
}

// warped validity mask of view 0 at a student pixel (:306, before the product with um1); `um0` = the (H,W) mask of the sample or
// NULL (all ones, still zero-padded: the sum of the in-range weights)
CMS_HD float aug_warp_mask(const AugTaps& t, const float* um0, int W) {
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (t.w[k] != 0.0f) {
            const float u = um0 ? um0[(size_t)(t.Y0 + (k >> 1)) * W + (t.X0 + (k & 1))] : 1.0f;
            m = fmaf(t.w[k], u, m);
        }
    }
    return m;
}

// The teacher's prediction warped to a student pixel. `tea(k)` -> a callable int -> float with the teacher's (upsampled) logits
// at tap k; it is asked only for taps with a non-zero weight. The target vectors are accumulated tap by tap: one tap's logits and
// exponentials are live at a time. CT == 0 (run-time class count): only the taps' softmax statistics are kept and a class's
// target is re-gathered on demand -- the same operations in the same order, so both forms give the same values.
template <int CT>
struct AugTarget {
    float p[CT > 0 ? CT : 1];   // sum_k w_k softmax(L_k)[c]                    (need_prob)
    float l[CT > 0 ? CT : 1];   // sum_k w_k L_k[c]                             (need_logit)
    float mx[4], rz[4];         // CT == 0: per-tap softmax statistics
    float w[4];
    float conf;                 // max_c p[c] (need_prob), else 0
};

template <int CT, class TEA>
CMS_HD float aug_target_prob(const AugTarget<CT>& t, TEA tea, int c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (CT > 0) return t.p[CT > 0 ? c : 0];
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (t.w[k] != 0.0f) {
            const float pr = expf(tea(k)(c) - t.mx[k]) * t.rz[k];
            acc = fmaf(t.w[k], pr, acc);
        }
    }
    return acc;
}

template <int CT, class TEA>
CMS_HD float aug_target_logit(const AugTarget<CT>& t, TEA tea, int c) {
    if (CT > 0) return t.l[CT > 0 ? c : 0];
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (t.w[k] != 0.0f) acc = fmaf(t.w[k], tea(k)(c), acc);
    }
    return acc;
}

template <int CT, class TEA>
CMS_HD void aug_target_build(AugTarget<CT>& t, const AugTaps& taps, TEA tea, int crt, bool need_prob, bool need_logit) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
    for (int k = 0; k < 4; ++k) t.w[k] = taps.w[k];
    if (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) t.p[c] = t.l[c] = 0.0f;
        // a rolled loop over the taps (the weight picked with selects, not indexed): the registers of ONE tap's gathers
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const float wk = k == 0 ? taps.w[0] : (k == 1 ? taps.w[1] : (k == 2 ? taps.w[2] : taps.w[3]));
            if (wk != 0.0f) {
                auto g = tea(k);
                float lv[CT > 0 ? CT : 1];
#pragma unroll
                for (int c = 0; c < CT; ++c) lv[c] = g(c);
                if (need_logit) {
#pragma unroll
                    for (int c = 0; c < CT; ++c) t.l[c] = fmaf(wk, lv[c], t.l[c]);
                }
                if (need_prob) {
                    float mx = -INFINITY;
#pragma unroll
                    for (int c = 0; c < CT; ++c) mx = fmaxf(mx, lv[c]);
                    float z = 0.0f;
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        lv[c] = expf(lv[c] - mx);
                        z += lv[c];
                    }
                    const float rz = 1.0f / z;
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const float pr = lv[c] * rz;
                        t.p[c] = fmaf(wk, pr, t.p[c]);
                    }
                }
            }
        }
    } else if (need_prob) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t.mx[k] = 0.0f;
            t.rz[k] = 0.0f;
            if (t.w[k] != 0.0f) {
                float z;
                softmax_stats<0>(tea(k), crt, t.mx[k], z);
                t.rz[k] = 1.0f / z;
            }
        }
    }
    t.conf = 0.0f;
    if (need_prob) {
        const int C = CT > 0 ? CT : crt;
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < C; ++c) m = fmaxf(m, aug_target_prob<CT>(t, tea, c));
        t.conf = m;
    }
}

// the student's logits of one pixel: read into registers once (compile-time class count) or re-gathered per use
template <int CT, class LS>
struct AugStudent {
    float v[CT > 0 ? CT : 1];
    LS ls;
    CMS_HD explicit AugStudent(LS src) : ls(src) {
#pragma unroll
        for (int c = 0; c < CT; ++c) v[c] = src(c);
    }
    CMS_HD float operator()(int c) const { return CT > 0 ? v[CT > 0 ? c : 0] : ls(c); }
};

CMS_HD bool aug_loss_on_logits(int loss_fn) { return loss_fn == LOSS_LOGITS_VAR || loss_fn == LOSS_LOGITS_SMOOTHL1; }

// forward: per-pixel loss (summed over classes, / sqrt(C) where applicable) + the warped confidence. `ls`: callable int -> float
// for the student's (upsampled) logits. `thresh`: a confidence threshold is in force (else the confidence is not needed).
template <int CT, class LS0, class TEA>
CMS_HD PixelFwd aug_pixel_fwd(LS0 ls0, const AugTaps& taps, TEA tea, int crt, int loss_fn, float inv_root_c, bool thresh) {
    const int C = CT > 0 ? CT : crt;
    const bool on_logits = aug_loss_on_logits(loss_fn);
    AugTarget<CT> t;
    aug_target_build<CT>(t, taps, tea, crt, !on_logits || thresh, on_logits);
    // the student's logits only now: they are not live while the taps are gathered
    const AugStudent<CT, LS0> ls(ls0);
    PixelFwd out;
    out.conf = t.conf;
    float acc = 0.0f;
    if (loss_fn == LOSS_LOGITS_VAR) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = ls(c) - aug_target_logit<CT>(t, tea, c);
            acc += d * d;
        }
        out.loss = acc * inv_root_c;
        return out;
    }
    if (loss_fn == LOSS_LOGITS_SMOOTHL1) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc += smooth_l1(ls(c) - aug_target_logit<CT>(t, tea, c));
        out.loss = acc * inv_root_c;
        return out;
    }
    SoftmaxRegs<CT> ss;
    softmax_regs<CT>(ls, crt, ss);
    if (loss_fn == LOSS_VAR) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = softmax_prob<CT>(ss, ls, c) - aug_target_prob<CT>(t, tea, c);
            acc += d * d;
        }
    } else if (loss_fn == LOSS_BCE) {
        const float eps = 1e-6f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float p = softmax_prob<CT>(ss, ls, c), tc = aug_target_prob<CT>(t, tea, c);
            acc += -(tc * logf(p + eps) + (1.0f - tc) * logf(1.0f - p + eps));
        }
    } else {  // LOSS_KLD: t * (log t - log_softmax(ls)); 0 where t == 0. A blend of softmaxes has no logit form: log t is a logf
        const float log_zs = logf(ss.z);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float tc = aug_target_prob<CT>(t, tea, c);
            const float logp = (ls(c) - ss.mx) - log_zs;
            acc += tc > 0.0f ? tc * (logf(tc) - logp) : 0.0f;
        }
    }
    out.loss = acc;
    return out;
}

// backward: factor * d(per-pixel loss)/d(student logit k) through `emit(k, value)`, factor = `factor_of_conf(conf)` with the
// warped confidence (0 without `thresh` for the logit losses) -- known once the target is built, so no gradient vector is
// kept. The teacher carries no gradient, so this is consistency_pixel_bwd's  p_k * (f'_k - sum_c f'_c p_c)  with t = the
// warped probabilities (logits for the logit losses).
template <int CT, class LS0, class TEA, class F, class E>
CMS_HD void aug_pixel_bwd(LS0 ls0, const AugTaps& taps, TEA tea, int crt, int loss_fn, float inv_root_c, bool thresh,
                          F factor_of_conf, E emit) {
    const int C = CT > 0 ? CT : crt;
    const bool on_logits = aug_loss_on_logits(loss_fn);
    AugTarget<CT> t;
    aug_target_build<CT>(t, taps, tea, crt, !on_logits || thresh, on_logits);
    const AugStudent<CT, LS0> ls(ls0);
    const float f = factor_of_conf(t.conf);
    if (loss_fn == LOSS_LOGITS_VAR) {
#pragma unroll
        for (int k = 0; k < C; ++k) emit(k, f * (2.0f * (ls(k) - aug_target_logit<CT>(t, tea, k)) * inv_root_c));
        return;
    }
    if (loss_fn == LOSS_LOGITS_SMOOTHL1) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const float d = ls(k) - aug_target_logit<CT>(t, tea, k);
            const float g = fabsf(d) < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
            emit(k, f * (g * inv_root_c));
        }
        return;
    }
    SoftmaxRegs<CT> ss;
    softmax_regs<CT>(ls, crt, ss);
    const float eps = 1e-6f;
    float dot = 0.0f;
    float tsum = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float p = softmax_prob<CT>(ss, ls, c), tc = aug_target_prob<CT>(t, tea, c);
        float fp;
        if (loss_fn == LOSS_VAR) {
            fp = 2.0f * (p - tc);
        } else if (loss_fn == LOSS_BCE) {
            fp = -tc / (p + eps) + (1.0f - tc) / (1.0f - p + eps);
        } else {
            fp = 0.0f;
        }
        dot += fp * p;
        tsum += tc;
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const float p = softmax_prob<CT>(ss, ls, k), tc = aug_target_prob<CT>(t, tea, k);
        float g;
        if (loss_fn == LOSS_VAR) {
            g = p * (2.0f * (p - tc) - dot);
        } else if (loss_fn == LOSS_BCE) {
            g = p * ((-tc / (p + eps) + (1.0f - tc) / (1.0f - p + eps)) - dot);
        } else {  // KLD: -t_k + p_k * sum_c t_c (the warped probabilities need not sum to one: zero padding)
            g = p * tsum - tc;
        }
        emit(k, f * g);
    }
}

// ---- the rectangle of teacher PIXELS a tile of student pixels samples: the tile's four corners through the (affine) map, the
// bounding box padded by one pixel per side (the taps floor(i), floor(i) + 1 and the rounding of the fmaf chain), clipped to the
// image. Empty (hi < lo) when the tile looks wholly outside. Used by the kernels and restated by tests/test_aug_cpu.py.
struct AugBox {
    int x_lo, x_hi, y_lo, y_hi;     // inclusive
};

CMS_HD AugBox aug_tile_box(const float* xf, int x0, int y0, int tw, int th, int H, int W) {
    float ixmin = INFINITY, ixmax = -INFINITY, iymin = INFINITY, iymax = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float ix, iy;
        aug_map(xf, x0 + ((k & 1) ? tw - 1 : 0), y0 + ((k >> 1) ? th - 1 : 0), ix, iy);
        ix = aug_clamp(ix, W);
        iy = aug_clamp(iy, H);
        ixmin = fminf(ixmin, ix); ixmax = fmaxf(ixmax, ix);
        iymin = fminf(iymin, iy); iymax = fmaxf(iymax, iy);
    }
    AugBox b;
    b.x_lo = (int)floorf(ixmin) - 1; b.x_hi = (int)floorf(ixmax) + 2;
    b.y_lo = (int)floorf(iymin) - 1; b.y_hi = (int)floorf(iymax) + 2;
    if (b.x_lo < 0) b.x_lo = 0;
    if (b.y_lo < 0) b.y_lo = 0;
    if (b.x_hi > W - 1) b.x_hi = W - 1;
    if (b.y_hi > H - 1) b.y_hi = H - 1;
    return b;
}

}  // namespace cms
