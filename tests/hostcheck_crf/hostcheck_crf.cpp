// test infrastructure: a stand-alone host driver of the product's CRF arithmetic (csrc/crf_math.hpp, and through it the vote of
// csrc/tta_math.hpp and the taps, gathers and softmax of csrc/pixel_math.hpp), the very functions the kernels of csrc/crf.hip call,
// walked sample by sample and pixel by pixel ("thread by thread") in the launch's order: the unary pass, then `iters` Jacobi passes
// over two ping-pong buffers with the class chunks the launch would take.
//
//   hostcheck_crf REQUEST RESULT
//
// REQUEST, little-endian: int32 n, c, H, W, k, align_corners, radius, dilation, iters; float32 bi_w, bi_xy, bi_rgb, pos_w, pos_xy;
// per view int32 h, w, flip; then per view its (n, c, h, w) float32 logits; the (n, 3, H, W) uint8 image; the (n, 4) int32 rectangles.
// RESULT: (n, c, H, W) float32 Q (P outside the rectangles), n * H * W uint8 pred, the same of the unary prediction, 2 int64 counts.
// Every tensor lives in an exactly-sized heap block and the outputs are filled with 0xA5 before use, so a sanitizer build sees every
// byte outside them and an element the walk does not write shows in the result. Exit code 2 for a request the product refuses (the
// refusal is the product's own check).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cutmix-semisup-seg_amd/csrc/crf_math.hpp"
#include "../hostcheck_common.hpp"

using namespace cms;

struct Walk {
    const cms_crf_desc* d;
    CrfTables tab;
    float inv2b;
    const float* logp;
    size_t plane;
};

// one Jacobi pass over the pixels of every rectangle: the body of crf_meanfield_kernel for one thread, LDS replaced by the arrays
template <int CC>
static void iterate(const Walk& k, const float* q_src, float* q_dst, bool last, const uint8_t* uarg, uint8_t* pred, int64_t* stats) {
    const cms_crf_desc* d = k.d;
    const int C = d->c, R = d->radius, S = d->dilation, W = d->W;
    const size_t plane = k.plane;
    const bool one_chunk = C <= CC;
    for (int n = 0; n < d->n; ++n) {
        const int32_t* r = d->rect + 4 * n;
        const int top = r[0], left = r[1], h = r[2], w = r[3];
        const uint8_t* img = d->rgb + (size_t)n * 3 * plane;
        for (int u = 0; u < h; ++u)
            for (int v = 0; v < w; ++v) {
                const size_t pix = (size_t)(top + u) * W + left + v, base = (size_t)n * C * plane + pix;
                const int n_nb = crf_neighbours(u, v, h, w, R, S);
                auto inside = [&](int dy, int dx) {
                    const int uu = u + S * dy, vv = v + S * dx;
                    return uu >= 0 && uu < h && vv >= 0 && vv < w;
                };
                auto at = [&](int dy, int dx) { return (size_t)(top + u + S * dy) * W + left + v + S * dx; };
                auto rgb = [&](int dy, int dx) -> uint32_t {
                    if (!inside(dy, dx)) return 0;
                    const size_t o = at(dy, dx);
                    return crf_pack_rgb(img[o], img[plane + o], img[2 * plane + o]);
                };
                float acc[CC];
                for (int c0 = 0; c0 < C; c0 += CC) {
                    auto q = [&](int dy, int dx, int c) -> float {
                        if (!inside(dy, dx) || c0 + c >= C) return 0.0f;
                        return q_src[((size_t)n * C + c0 + c) * plane + at(dy, dx)];
                    };
                    crf_message<CC>(k.tab, R, d->bi_w, k.inv2b, rgb, q, acc);
                    if (!one_chunk)
                        for (int c = 0; c < CC; ++c)
                            if (c0 + c < C) q_dst[base + (size_t)(c0 + c) * plane] = acc[c];
                }
                int best;
                if (one_chunk) {
                    for (int c = 0; c < CC; ++c)
                        if (c < C) acc[c] = crf_energy(k.logp[base + (size_t)c * plane], acc[c], n_nb);
                    best = crf_softmax_argmax<CC>(C, [&](int c) -> float& { return acc[c]; });
                    for (int c = 0; c < CC; ++c)
                        if (c < C) q_dst[base + (size_t)c * plane] = acc[c];
                } else {
                    for (int c = 0; c < C; ++c) {
                        const size_t o = base + (size_t)c * plane;
                        q_dst[o] = crf_energy(k.logp[o], q_dst[o], n_nb);
                    }
                    best = crf_softmax_argmax<0>(C, [&](int c) -> float& { return q_dst[base + (size_t)c * plane]; });
                }
                if (last) {
                    const size_t idx = (size_t)n * plane + pix;
                    pred[idx] = (uint8_t)best;
                    stats[0] += 1;
                    stats[1] += best != (int)uarg[idx];
                }
            }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_crf REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[9];
    float prm[5];
    if (fread(head, sizeof(int32_t), 9, f) != 9 || fread(prm, sizeof(float), 5, f) != 5) return 1;
    cms_crf_desc d;
    memset(&d, 0, sizeof(d));
    d.n = head[0], d.c = head[1], d.H = head[2], d.W = head[3], d.k = head[4], d.align_corners = head[5];
    d.radius = head[6], d.dilation = head[7], d.iters = head[8];
    d.bi_w = prm[0], d.bi_xy = prm[1], d.bi_rgb = prm[2], d.pos_w = prm[3], d.pos_xy = prm[4];
    if (d.k < 1 || d.k > CMS_TTA_MAX_VIEWS || d.n < 1 || d.c < 1 || d.c > kTtaMaxClasses || d.H < 1 || d.W < 1 ||
        !tta_count_ok(d.n, d.H, d.W))
        return 2;
    for (int i = 0; i < d.k; ++i) {
        int32_t v[3];
        if (fread(v, sizeof(int32_t), 3, f) != 3) return 1;
        d.h[i] = v[0], d.w[i] = v[1], d.flip[i] = v[2];
        if (v[0] < 1 || v[1] < 1 || !tta_count_ok(d.n, d.c, v[0], v[1])) return 2;
    }
    for (int i = 0; i < d.k; ++i) d.logits[i] = (const float*)read_block(f, (size_t)d.n * d.c * d.h[i] * d.w[i] * sizeof(float));
    const size_t plane = (size_t)d.H * d.W, pix = (size_t)d.n * plane, elems = pix * d.c;
    d.rgb = (const uint8_t*)read_block(f, pix * 3);
    d.rect = (const int32_t*)read_block(f, (size_t)d.n * 4 * sizeof(int32_t));
    fclose(f);
    int64_t stats[2] = {0, 0};
    uint8_t* pred = (uint8_t*)malloc(pix);
    uint8_t* uarg = (uint8_t*)malloc(pix);
    float* qout = (float*)malloc(elems * sizeof(float));
    d.stats = stats, d.pred_out = pred, d.q_out = qout;
    const size_t ws_bytes = crf_workspace_bytes(d.n, d.c, d.H, d.W);
    void* ws = ws_bytes ? aligned_alloc(256, ws_bytes) : nullptr;
    if (crf_check(&d, ws, ws_bytes)) return 2;
    float* logp = (float*)malloc(elems * sizeof(float));
    float* qa = (float*)malloc(elems * sizeof(float));
    float* qb = (float*)malloc(elems * sizeof(float));
    memset(pred, 0xA5, pix), memset(uarg, 0xA5, pix);
    memset(qout, 0xA5, elems * sizeof(float)), memset(logp, 0xA5, elems * sizeof(float));
    memset(qa, 0xA5, elems * sizeof(float)), memset(qb, 0xA5, elems * sizeof(float));

    // ---- the unary pass (crf_unary_kernel, one thread per canvas pixel)
    cms_tta_desc td;
    memset(&td, 0, sizeof(td));
    for (int i = 0; i < d.k; ++i) td.logits[i] = d.logits[i], td.h[i] = d.h[i], td.w[i] = d.w[i], td.flip[i] = d.flip[i];
    td.n = d.n, td.c = d.c, td.H = d.H, td.W = d.W, td.k = d.k, td.align_corners = d.align_corners;
    TtaViews v;
    tta_make_views(&td, &v);
    float score[kTtaMaxClasses];
    for (int n = 0; n < d.n; ++n)
        for (int y = 0; y < d.H; ++y)
            for (int x = 0; x < d.W; ++x) {
                const int best = tta_vote_pixel(v, d.k, n, d.c, y, x, d.align_corners != 0, [&](int c) -> float& { return score[c]; });
                const int32_t* r = d.rect + 4 * n;
                const int u = y - r[0], vv = x - r[1];
                const bool inside = u >= 0 && u < r[2] && vv >= 0 && vv < r[3];
                const size_t idx = (size_t)n * plane + (size_t)y * d.W + x, base = (size_t)n * d.c * plane + (size_t)y * d.W + x;
                for (int c = 0; c < d.c; ++c) {
                    float p, lp;
                    crf_unary_value(score[c], d.k, &p, &lp);
                    logp[base + c * plane] = lp, qa[base + c * plane] = p;
                    if (!inside) qout[base + c * plane] = p;
                }
                uarg[idx] = (uint8_t)best;
                if (!inside) pred[idx] = (uint8_t)best;
            }

    // ---- the iterations
    Walk k;
    k.d = &d, k.logp = logp, k.plane = plane, k.inv2b = crf_inv2b(d.bi_rgb);
    crf_make_tables(d.radius, d.dilation, d.bi_xy, d.pos_w, d.pos_xy, &k.tab);
    const int cc = crf_chunk_for(d.c);
    for (int t = 0; t < d.iters; ++t) {
        const bool last = t == d.iters - 1;
        const float* src = t % 2 == 0 ? qa : qb;
        float* dst = last ? qout : (t % 2 == 0 ? qb : qa);
        switch (cc) {
            case 4: iterate<4>(k, src, dst, last, uarg, pred, stats); break;
            case 8: iterate<8>(k, src, dst, last, uarg, pred, stats); break;
            case 16: iterate<16>(k, src, dst, last, uarg, pred, stats); break;
            case 24: iterate<24>(k, src, dst, last, uarg, pred, stats); break;
            default: iterate<32>(k, src, dst, last, uarg, pred, stats); break;
        }
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(qout, sizeof(float), elems, o);
    fwrite(pred, 1, pix, o);
    fwrite(uarg, 1, pix, o);
    fwrite(stats, sizeof(int64_t), 2, o);
    fclose(o);
    for (int i = 0; i < d.k; ++i) free((void*)d.logits[i]);
    free((void*)d.rgb), free((void*)d.rect), free(pred), free(uarg), free(qout), free(logp), free(qa), free(qb), free(ws);
    return 0;
}
