// Per-pixel and per-update arithmetic of the class-threshold consistency (cthresh.hip), `__host__ __device__` like pixel_math.hpp so
// that tests/test_cthresh_hostcheck.py can drive the very same code on the host; the product never runs it there.
//
// Definition (include/cutmixseg.h). For the pasted, upsampled teacher logit row t of a pixel, with m = max t,
// z = sum exp(t_k - m), conf = 1 / z (the float the consistency kernels compare with conf_thresh):
//   k*        the SMALLEST index with t_k == m (0 when no logit compares equal to m: a row of NaNs)
//   pass bit  conf >= thr[k*] in fp32 (a NaN fails)
//   q_c       exp(t_c - m) * (1 / z), the rounded product softmax_prob returns
//   fixed point  rint(v * 2^24) as an unsigned integer, v clamped to [0, 1], NaN -> 0: sums of such integers do not depend on
//             the order of the additions, which float sums do
#pragma once
#include "pixel_math.hpp"

namespace cms {

constexpr float CT_FIX_ONE = 16777216.0f;       // 2^24

CMS_HD uint32_t ct_fix24(float v) {
    if (!(v > 0.0f)) return 0u;                 // NaN, zero and negatives
    if (v >= 1.0f) return 1u << 24;
    return (uint32_t)rintf(v * CT_FIX_ONE);     // exact product (a power of two), one rounding to the nearest integer, ties to even
}

CMS_HD bool ct_pass(float conf, float thr) { return conf >= thr; }

// k* of a logit row with maximum `mx` (softmax_stats / softmax_regs: a chain of fmaxf, which skips NaNs)
template <int CT, class L>
CMS_HD int ct_argmax(L l, int crt, float mx) {
    const int C = CT > 0 ? CT : crt;
    int k = 0;
#pragma unroll
    for (int c = C - 1; c >= 0; --c) k = (l(c) == mx) ? c : k;
    return k;
}

// k* from the row alone: the maximum by the fmaxf chain of softmax_stats / softmax_regs, then the tie rule
template <int CT, class L>
CMS_HD int ct_kstar(L l, int crt) {
    const int C = CT > 0 ? CT : crt;
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, l(c));
    return ct_argmax<CT>(l, crt, mx);
}

// The statistics of one pixel from its teacher row: conf, and through `emit(c, fixed-point q_c)` the class distribution.
// Same functions on the same values as consistency_pixel_fwd's teacher half, so conf is bit for bit the loss kernels' float.
template <int CT, class L, class E>
CMS_HD void ct_pixel_stats(L lt, int crt, float& conf, E emit) {
    const int C = CT > 0 ? CT : crt;
    SoftmaxRegs<CT> st;
    softmax_regs<CT>(lt, crt, st);
    conf = st.rz;
#pragma unroll
    for (int c = 0; c < C; ++c) emit(c, ct_fix24(softmax_prob<CT>(st, lt, c)));
}

// ---- the table of one iteration: unsigned 64-bit integers, [n_valid | S_conf | S_c x C | N_pred x C | N_pass x C]
CMS_HD int ct_table_len(int C) { return 2 + 3 * C; }
CMS_HD int ct_slot_s(int C, int c) { (void)C; return 2 + c; }
CMS_HD int ct_slot_pred(int C, int c) { return 2 + C + c; }
CMS_HD int ct_slot_pass(int C, int c) { return 2 + 2 * C + c; }
// the epoch table: [n_valid | N_pred x C | N_pass x C]
CMS_HD int ct_epoch_len(int C) { return 1 + 2 * C; }

// The fold of one iteration's table, by one thread in fp64. `state` = [tau | p~ x C]. Adaptive mode with n_valid > 0:
//   mu = S_conf / (2^24 n_valid), pi_c = S_c / (2^24 n_valid); tau <- lam tau + (1 - lam) mu; p~_c <- lam p~_c + (1 - lam) pi_c;
//   thr_c = fp32(min(ceil, max(floor, tau * p~_c / max_j p~_j))).
// Both modes: N_pred, N_pass and n_valid are added into the epoch table and the iteration table is zeroed.
CMS_HD void ct_update(int C, int adaptive, double lam, double floor_v, double ceil_v, double* state, float* thr,
                      unsigned long long* table, unsigned long long* epoch) {
    // (no contraction: the host restatement rounds every product and every sum)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const unsigned long long n_valid = table[0];
    if (adaptive && n_valid > 0) {
        const double den = 16777216.0 * (double)n_valid;
        const double one_m = 1.0 - lam;
        const double mu = (double)table[1] / den;
        const double a = lam * state[0];
        const double b = one_m * mu;
        state[0] = a + b;
        double pmax = 0.0;
        for (int c = 0; c < C; ++c) {
            const double pi = (double)table[ct_slot_s(C, c)] / den;
            const double pa = lam * state[1 + c];
            const double pb = one_m * pi;
            state[1 + c] = pa + pb;
            pmax = state[1 + c] > pmax ? state[1 + c] : pmax;
        }
        for (int c = 0; c < C; ++c) {
            const double num = state[0] * state[1 + c];
            double v = num / pmax;
            v = v > floor_v ? v : floor_v;
            v = v < ceil_v ? v : ceil_v;
            thr[c] = (float)v;
        }
    }
    epoch[0] += n_valid;
    for (int c = 0; c < C; ++c) {
        epoch[1 + c] += table[ct_slot_pred(C, c)];
        epoch[1 + C + c] += table[ct_slot_pass(C, c)];
    }
    const int len = ct_table_len(C);
    for (int i = 0; i < len; ++i) table[i] = 0ull;
}

}  // namespace cms
