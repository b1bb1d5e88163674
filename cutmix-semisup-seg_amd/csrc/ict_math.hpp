// Per-pixel arithmetic of the ICT (interpolation consistency training) loss, shared by the loss kernels of
// ict.hip and driven on the host by tests/hostcheck_ict. Same conventions as pixel_math.hpp: `__host__ __device__`,
// compile-time class count with the exponentials in registers, contraction off where two evaluations of the same
// expression must agree bit for bit (the confidence of a pixel is computed by up to three launches).
//
// Reference behaviour restated here (train_seg_semisup_ict.py of the upstream repository):
//   mix factors          :306-307   lambda ~ Beta(alpha, alpha) per sample, float32; 1 - lambda in float32
//   blends               :310-311, 328-329, 341   a * (1 - lambda) + b * lambda: two rounded products, then their sum
//   confidence           :336-343   max_c softmax(L0) * (1 - lambda) + max_c softmax(L1) * lambda
//   consistency losses   :360-380   with the BLENDED probabilities (var / bce / kld) or logits (logits_var / logits_smoothl1)
#pragma once
#include "pixel_math.hpp"

namespace cms {

// a * (1 - lambda) + b * lambda as torch evaluates it: three roundings, never an FMA. `oml` = 1.0f - lam.
CMS_HD float ict_mix(float a, float b, float oml, float lam) {
#if defined(__clang__)
#pragma clang fp contract(off)
    const float x = a * oml;
    const float y = b * lam;
    return x + y;
#else
    volatile float x = a * oml;
    volatile float y = b * lam;
    return x + y;
#endif
}

// blended confidence of the two teacher predictions (:338-341); max_c softmax(l)_c = exp(0) / z = 1 / z
template <int CT>
CMS_HD float ict_conf_of(const SoftmaxRegs<CT>& s0, const SoftmaxRegs<CT>& s1, float oml, float lam) {
    return ict_mix(s0.rz, s1.rz, oml, lam);
}

template <int CT, class L0, class L1>
CMS_HD float ict_conf(L0 l0, L1 l1, float lam, int crt) {
    SoftmaxRegs<CT> s0, s1;
    softmax_regs<CT>(l0, crt, s0);
    softmax_regs<CT>(l1, crt, s1);
    return ict_conf_of<CT>(s0, s1, 1.0f - lam, lam);
}

// blended teacher probability of class c (:329)
template <int CT, class L0, class L1>
CMS_HD float ict_target_prob(const SoftmaxRegs<CT>& s0, L0 l0, const SoftmaxRegs<CT>& s1, L1 l1, int c, float oml, float lam) {
    return ict_mix(softmax_prob<CT>(s0, l0, c), softmax_prob<CT>(s1, l1, c), oml, lam);
}

// forward: per-pixel loss (summed over classes, / sqrt(C) where applicable) + blended teacher confidence.
// ls / l0 / l1: callables int -> float for the student's and the two teachers' (upsampled) logits.
template <int CT, class LS, class L0, class L1>
CMS_HD PixelFwd ict_pixel_fwd(LS ls, L0 l0, L1 l1, float lam, int crt, int loss_fn, float inv_root_c) {
    const int C = CT > 0 ? CT : crt;
    const float oml = 1.0f - lam;
    SoftmaxRegs<CT> ss, s0, s1;
    softmax_regs<CT>(l0, crt, s0);
    softmax_regs<CT>(l1, crt, s1);
    PixelFwd out;
    out.conf = ict_conf_of<CT>(s0, s1, oml, lam);
    float acc = 0.0f;
    if (loss_fn == LOSS_LOGITS_VAR) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = ls(c) - ict_mix(l0(c), l1(c), oml, lam);
            acc += d * d;
        }
        out.loss = acc * inv_root_c;
        return out;
    }
    if (loss_fn == LOSS_LOGITS_SMOOTHL1) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc += smooth_l1(ls(c) - ict_mix(l0(c), l1(c), oml, lam));
        out.loss = acc * inv_root_c;
        return out;
    }
    softmax_regs<CT>(ls, crt, ss);
    if (loss_fn == LOSS_VAR) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = softmax_prob<CT>(ss, ls, c) - ict_target_prob<CT>(s0, l0, s1, l1, c, oml, lam);
            acc += d * d;
        }
    } else if (loss_fn == LOSS_BCE) {
        const float eps = 1e-6f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float p = softmax_prob<CT>(ss, ls, c), t = ict_target_prob<CT>(s0, l0, s1, l1, c, oml, lam);
            acc += -(t * logf(p + eps) + (1.0f - t) * logf(1.0f - p + eps));
        }
    } else {  // LOSS_KLD: t * (log t - log_softmax(ls)); 0 where t == 0. The blend has no logit form: log t is a logf
        const float log_zs = logf(ss.z);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float t = ict_target_prob<CT>(s0, l0, s1, l1, c, oml, lam);
            const float logp = (ls(c) - ss.mx) - log_zs;
            acc += t > 0.0f ? t * (logf(t) - logp) : 0.0f;
        }
    }
    out.loss = acc;
    return out;
}

// backward: d(per-pixel loss)/d(student logit k) through `emit(k, value)`. The teachers carry no gradient, so this is
// consistency_pixel_bwd's  p_k * (f'_k - sum_c f'_c p_c)  with t = the blended probabilities (logits for the logit losses).
template <int CT, class LS, class L0, class L1, class E>
CMS_HD void ict_pixel_bwd(LS ls, L0 l0, L1 l1, float lam, int crt, int loss_fn, float inv_root_c, E emit) {
    const int C = CT > 0 ? CT : crt;
    const float oml = 1.0f - lam;
    if (loss_fn == LOSS_LOGITS_VAR) {
#pragma unroll
        for (int k = 0; k < C; ++k) emit(k, 2.0f * (ls(k) - ict_mix(l0(k), l1(k), oml, lam)) * inv_root_c);
        return;
    }
    if (loss_fn == LOSS_LOGITS_SMOOTHL1) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const float d = ls(k) - ict_mix(l0(k), l1(k), oml, lam);
            const float g = fabsf(d) < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
            emit(k, g * inv_root_c);
        }
        return;
    }
    SoftmaxRegs<CT> ss, s0, s1;
    softmax_regs<CT>(l0, crt, s0);
    softmax_regs<CT>(l1, crt, s1);
    softmax_regs<CT>(ls, crt, ss);
    const float eps = 1e-6f;
    float dot = 0.0f;
    float tsum = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float p = softmax_prob<CT>(ss, ls, c), t = ict_target_prob<CT>(s0, l0, s1, l1, c, oml, lam);
        float fp;
        if (loss_fn == LOSS_VAR) {
            fp = 2.0f * (p - t);
        } else if (loss_fn == LOSS_BCE) {
            fp = -t / (p + eps) + (1.0f - t) / (1.0f - p + eps);
        } else {
            fp = 0.0f;
        }
        dot += fp * p;
        tsum += t;
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const float p = softmax_prob<CT>(ss, ls, k), t = ict_target_prob<CT>(s0, l0, s1, l1, k, oml, lam);
        float g;
        if (loss_fn == LOSS_VAR) {
            g = p * (2.0f * (p - t) - dot);
        } else if (loss_fn == LOSS_BCE) {
            g = p * ((-t / (p + eps) + (1.0f - t) / (1.0f - p + eps)) - dot);
        } else {  // KLD: -t_k + p_k * sum_c t_c
            g = p * tsum - t;
        }
        emit(k, g);
    }
}

}  // namespace cms
