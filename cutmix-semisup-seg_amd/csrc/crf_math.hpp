// CRF refinement (csrc/crf.hip): descriptor validation, the pair-weight tables and the per-pixel arithmetic of the truncated,
// dilated-window mean-field inference (include/cutmixseg.h states the definition). Everything here is plain C++ /
// `__host__ __device__`, so tests/hostcheck_crf drives the very code the kernels are made of on the host; the product never runs it
// there. The unary term is the vote of tta_math.hpp.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/cutmixseg.h"
#include "tta_math.hpp"

namespace cms {

constexpr int kCrfMaxRadius = 5, kCrfMaxDilation = 16, kCrfMaxIters = 32;
constexpr int kCrfMaxTaps = (2 * kCrfMaxRadius + 1) * (2 * kCrfMaxRadius + 1);
constexpr int kCrfTileW = 32, kCrfTileH = 8;              // sublattice pixels of a workgroup: a wavefront reads two rows of 32
constexpr int kCrfGroup = 32;                             // samples per launch: their rectangles travel as kernel arguments
constexpr int kCrfChunk = 32;                             // classes a workgroup holds in LDS at a time

// what depends on the offset (dy, dx) alone, indexed (dy + R) * (2R + 1) + (dx + R), worked out once on the host in fp64
struct CrfTables {
    float arg_a[kCrfMaxTaps];       // -|p - q|^2 / (2 theta_alpha^2)
    float k_g[kCrfMaxTaps];         // w_g exp(-|p - q|^2 / (2 theta_gamma^2))
};

struct CrfRects {
    int top[kCrfGroup], left[kCrfGroup], h[kCrfGroup], w[kCrfGroup];
};

inline bool crf_weight_ok(float v) { return v >= 0.0f && v <= FLT_MAX; }         // finite, >= 0 (NaN fails)
inline bool crf_theta_ok(float v) { return v > 0.0f && v <= FLT_MAX; }

inline size_t crf_align(size_t v) { return (v + 255) & ~(size_t)255; }

// bytes of workspace: log P, two ping-pong Q (fp32, (n, c, H, W) each) and the uint8 unary argmax; 0 for sizes crf_check refuses
inline size_t crf_workspace_bytes(int n, int c, int H, int W) {
    if (n < 1 || c < 1 || c > kTtaMaxClasses || H < 1 || W < 1 || !tta_count_ok(n, H, W)) return 0;
    const size_t pix = (size_t)n * H * W;
    return 3 * crf_align(pix * c * sizeof(float)) + crf_align(pix);
}

// NULL when cms_crf_refine accepts the descriptor, else what is wrong with it
inline const char* crf_check(const cms_crf_desc* d, const void* workspace, size_t workspace_bytes) {
    if (!d) return "NULL descriptor";
    if (d->k < 1 || d->k > CMS_TTA_MAX_VIEWS) return "1 <= k <= 16 views";
    if (d->c < 1 || d->c > kTtaMaxClasses) return "1 <= num_classes <= 64";
    if (d->n < 1 || d->H < 1 || d->W < 1) return "bad geometry (n, H, W >= 1)";
    for (int i = 0; i < d->k; ++i) {
        if (d->h[i] < 1 || d->w[i] < 1) return "bad geometry (a view below 1 x 1)";
        if (!d->logits[i]) return "logits NULL";
    }
    if (!d->rgb) return "rgb NULL";
    if (!d->rect) return "rect NULL";
    if (!d->stats) return "stats NULL";
    if (((uintptr_t)d->stats & 7) != 0) return "stats misaligned";
    if (d->radius < 1 || d->radius > kCrfMaxRadius) return "1 <= radius <= 5";
    if (d->dilation < 1 || d->dilation > kCrfMaxDilation) return "1 <= dilation <= 16";
    if (d->iters < 1 || d->iters > kCrfMaxIters) return "1 <= iters <= 32";
    if (!crf_weight_ok(d->bi_w) || !crf_weight_ok(d->pos_w)) return "the kernel weights must be finite and >= 0";
    if (!crf_theta_ok(d->bi_xy) || !crf_theta_ok(d->bi_rgb) || !crf_theta_ok(d->pos_xy)) return "every theta must be finite and > 0";
    if (d->cm && !d->labels) return "cm given without labels";
    if (!d->cm && !d->pred_out && !d->q_out) return "nothing to produce (cm, pred_out and q_out NULL)";
    if (d->labels && d->label_dtype != CMS_LABEL_U8 && d->label_dtype != CMS_LABEL_I64) return "bad label dtype";
    if (!tta_count_ok(d->n, d->H, d->W)) return "more than 2^31 - 1 output pixels";
    for (int i = 0; i < d->n; ++i) {
        const int32_t* r = d->rect + 4 * (size_t)i;
        if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1) return "a rectangle with a negative corner or an empty side";
        if (r[0] >= d->H || r[1] >= d->W || r[2] > d->H - r[0] || r[3] > d->W - r[1]) return "a rectangle leaves the canvas";
    }
    if (!workspace) return "workspace NULL";
    if (((uintptr_t)workspace & 15) != 0) return "workspace misaligned";
    if (workspace_bytes < crf_workspace_bytes(d->n, d->c, d->H, d->W)) return "workspace too small";
    return nullptr;
}

inline void crf_make_tables(int R, int S, float bi_xy, float pos_w, float pos_xy, CrfTables* t) {
    for (int i = 0; i < kCrfMaxTaps; ++i) t->arg_a[i] = t->k_g[i] = 0.0f;
    const int side = 2 * R + 1;
    for (int dy = -R; dy <= R; ++dy) {
        for (int dx = -R; dx <= R; ++dx) {
            const double d2 = (double)S * S * (dy * dy + dx * dx);
            const int i = (dy + R) * side + dx + R;
            t->arg_a[i] = (float)(-d2 / (2.0 * (double)bi_xy * (double)bi_xy));
            t->k_g[i] = (float)((double)pos_w * exp(-d2 / (2.0 * (double)pos_xy * (double)pos_xy)));
        }
    }
}

inline float crf_inv2b(float bi_rgb) { return (float)(1.0 / (2.0 * (double)bi_rgb * (double)bi_rgb)); }

// the chunk of classes the mean-field launch is instantiated for: the smallest of 4, 8, 16, 24, 32 that holds min(C, 32)
inline int crf_chunk_for(int C) {
    const int sizes[5] = {4, 8, 16, 24, 32};
    for (int i = 0; i < 5; ++i)
        if (C <= sizes[i]) return sizes[i];
    return kCrfChunk;
}

// offsets d in [-R, R] with 0 <= u + S d < len
CMS_HD int crf_axis_count(int u, int len, int R, int S) {
    const int lo = u / S, hi = (len - 1 - u) / S;
    return (lo < R ? lo : R) + (hi < R ? hi : R) + 1;
}

// n(p): the neighbours of the pixel (u, v) of an h x w rectangle, an exact integer
CMS_HD int crf_neighbours(int u, int v, int h, int w, int R, int S) {
    return crf_axis_count(u, h, R, S) * crf_axis_count(v, w, R, S) - 1;
}

// a pixel's colour in one word; bit 24 says "inside the rectangle", so 0 is "not a neighbour"
CMS_HD uint32_t crf_pack_rgb(uint8_t r, uint8_t g, uint8_t b) {
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | (1u << 24);
}

// n(p) k(p, q) for the neighbour at table index idx: w_b exp(arg_a - |I_p - I_q|^2 / (2 theta_beta^2)) + k_g
CMS_HD float crf_pair_weight(const CrfTables& t, int idx, float w_b, float inv2b, uint32_t p, uint32_t q) {
    if (!(q >> 24)) return 0.0f;
    const int dr = (int)(p & 255u) - (int)(q & 255u), dg = (int)((p >> 8) & 255u) - (int)((q >> 8) & 255u),
              db = (int)((p >> 16) & 255u) - (int)((q >> 16) & 255u);
    const float d2 = (float)(dr * dr + dg * dg + db * db);            // <= 195075: exact
    const float arg = fmaf(-d2, inv2b, t.arg_a[idx]);
    return fmaf(w_b, expf(arg), t.k_g[idx]);
}

// n(p) times the message of CC classes of one pixel: the window in row-major (dy, dx) order, the centre left out.
// rgb(dy, dx) -> the neighbour's packed colour, 0 where it is none; q(dy, dx, c) -> its Q^t of class c of the chunk, 0 where it is none
template <int CC, class RGB, class Q>
CMS_HD void crf_message(const CrfTables& t, int R, float w_b, float inv2b, RGB rgb, Q q, float (&acc)[CC]) {
#pragma unroll
    for (int c = 0; c < CC; ++c) acc[c] = 0.0f;
    const uint32_t p = rgb(0, 0);
    int idx = 0;
    for (int dy = -R; dy <= R; ++dy) {
        for (int dx = -R; dx <= R; ++dx, ++idx) {
            if (dy == 0 && dx == 0) continue;
            const float wq = crf_pair_weight(t, idx, w_b, inv2b, p, rgb(dy, dx));
#pragma unroll
            for (int c = 0; c < CC; ++c) acc[c] = fmaf(wq, q(dy, dx, c), acc[c]);
        }
    }
}

// log P(c) + message(c): the division by the neighbour count happens here, once per class; no neighbour, no message
CMS_HD float crf_energy(float logp, float acc, int n_nb) { return n_nb > 0 ? logp + acc / (float)n_nb : logp; }

// v(c) (a float lvalue per class): in, log P + message; out, Q^{t+1} = softmax_c of it -> the first index of the largest Q.
// CC > 0: v is backed by registers and the loops are unrolled over CC with c < C guarded; CC == 0: run-time loops.
template <int CC, class V>
CMS_HD int crf_softmax_argmax(int C, V v) {
    float mx = -INFINITY;
    if (CC > 0) {
#pragma unroll
        for (int c = 0; c < (CC > 0 ? CC : 1); ++c)
            if (c < C) mx = fmaxf(mx, v(c));
    } else {
        for (int c = 0; c < C; ++c) mx = fmaxf(mx, v(c));
    }
    float z = 0.0f;
    if (CC > 0) {
#pragma unroll
        for (int c = 0; c < (CC > 0 ? CC : 1); ++c) {
            if (c < C) {
                const float e = expf(v(c) - mx);
                v(c) = e;
                z += e;
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float e = expf(v(c) - mx);
            v(c) = e;
            z += e;
        }
    }
    const float rz = 1.0f / z;
    int best = 0;
    float bv = -INFINITY;
    if (CC > 0) {
#pragma unroll
        for (int c = 0; c < (CC > 0 ? CC : 1); ++c) {
            if (c < C) {
                const float qv = v(c) * rz;
                v(c) = qv;
                if (c == 0 || tta_beats(qv, bv)) {
                    bv = qv;
                    best = c;
                }
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const float qv = v(c) * rz;
            v(c) = qv;
            if (c == 0 || tta_beats(qv, bv)) {
                bv = qv;
                best = c;
            }
        }
    }
    return best;
}

// the unary term of one class from its vote score (the sum of k probabilities): P and log max(P, FLT_MIN)
CMS_HD void crf_unary_value(float score, int k, float* p, float* logp) {
    const float pv = score / (float)k;
    *p = pv;
    *logp = logf(fmaxf(pv, FLT_MIN));
}

}  // namespace cms
