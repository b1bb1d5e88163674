// test infrastructure: a stand-alone host driver of the product's test-time augmentation arithmetic (csrc/tta_math.hpp), the very
// functions the kernels of csrc/tta.hip call, walked block by block and thread by thread as the launch walks them.
//
//   hostcheck_tta REQUEST RESULT
//
// REQUEST, little-endian int32 words then float32 data:
//   op = 0 (vote):   n, c, H, W, k, align_corners, then k x (h, w, flip), then the k logit tensors (n, c, h_i, w_i)
//                    RESULT: n * H * W uint8 predictions
//   op = 1 (resize): n, c, H, W, Hs, Ws, flip, then the (n, c, H, W) source
//                    RESULT: n * c * Hs * Ws float32
// Every tensor and the score table of a block ([c][256] floats, NaN before use) live in exactly-sized heap blocks, so a sanitizer
// build sees every byte outside them. Exit code 2 for a request the product refuses (the refusal is the product's own check).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cutmix-semisup-seg_amd/csrc/tta_math.hpp"

using namespace cms;

static const int kBlock = 256, kMaxBlocks = 1024;      // csrc/tta.hip: kTtaBlock, grid_for(P, 256, 1024)

static bool read_ints(FILE* f, int32_t* dst, size_t count) { return fread(dst, sizeof(int32_t), count, f) == count; }

static float* read_floats(FILE* f, size_t count) {
    float* p = (float*)malloc(count * sizeof(float));
    if (!p || fread(p, sizeof(float), count, f) != count) exit(1);
    return p;
}

static int vote(FILE* f, const char* result) {
    int32_t head[6];
    if (!read_ints(f, head, 6)) return 1;
    cms_tta_desc d;
    memset(&d, 0, sizeof(d));
    d.n = head[0], d.c = head[1], d.H = head[2], d.W = head[3], d.k = head[4], d.align_corners = head[5];
    uint8_t dummy = 0;
    d.pred_out = &dummy;                                   // "something to produce"; the predictions go to `pred` below
    if (d.k < 1 || d.k > CMS_TTA_MAX_VIEWS) return tta_check_vote(&d) ? 2 : 3;      // no view table to read: the product's verdict
    const int k_read = d.k;
    for (int i = 0; i < k_read; ++i) {
        int32_t v[3];
        if (!read_ints(f, v, 3)) return 1;
        d.h[i] = v[0], d.w[i] = v[1], d.flip[i] = v[2];
    }
    // the product's verdict on the sizes before anything is read or allocated by them
    float probe = 0.0f;
    for (int i = 0; i < k_read; ++i) d.logits[i] = &probe;
    if (tta_check_vote(&d)) return 2;
    std::vector<float*> data;
    for (int i = 0; i < k_read; ++i) {
        data.push_back(read_floats(f, (size_t)d.n * d.c * d.h[i] * d.w[i]));
        d.logits[i] = data.back();
    }
    if (tta_check_vote(&d)) return 2;
    TtaViews v;
    tta_make_views(&d, &v);
    const size_t P = (size_t)d.n * d.H * d.W;
    uint8_t* pred = (uint8_t*)malloc(P);
    size_t blocks = (P + kBlock - 1) / kBlock;
    if (blocks > (size_t)kMaxBlocks) blocks = kMaxBlocks;
    const int mode = d.k >= 2 ? 2 : (d.h[0] == d.H && d.w[0] == d.W ? 0 : 1);
    for (size_t b = 0; b < blocks; ++b) {
        const size_t score_elems = mode == 2 ? (size_t)d.c * kBlock : 0;
        float* score = (float*)malloc(score_elems ? score_elems * sizeof(float) : 1);
        for (size_t i = 0; i < score_elems; ++i) score[i] = NAN;
        for (int tid = 0; tid < kBlock; ++tid)
            for (size_t idx = b * kBlock + tid; idx < P; idx += blocks * kBlock) {
                const int x = (int)(idx % d.W);
                const size_t t = idx / d.W;
                const int y = (int)(t % d.H), n = (int)(t / d.H);
                int best;
                if (mode == 2) best = tta_vote_pixel(v, d.k, n, d.c, y, x, d.align_corners != 0,
                                                     [&](int c) -> float& { return score[(size_t)c * kBlock + tid]; });
                else if (mode == 0) best = tta_single_pixel<true>(v, n, d.c, y, x, d.align_corners != 0);
                else best = tta_single_pixel<false>(v, n, d.c, y, x, d.align_corners != 0);
                pred[idx] = (uint8_t)best;
            }
        free(score);
    }
    FILE* g = fopen(result, "wb");
    if (!g || fwrite(pred, 1, P, g) != P) return 1;
    fclose(g);
    free(pred);
    for (float* p : data) free(p);
    return 0;
}

static int resize(FILE* f, const char* result) {
    int32_t head[7];
    if (!read_ints(f, head, 7)) return 1;
    const int n = head[0], c = head[1], H = head[2], W = head[3], Hs = head[4], Ws = head[5], flip = head[6];
    float probe = 0.0f;
    if (tta_check_resize(&probe, &probe, n, c, H, W, Hs, Ws, CMS_F32)) return 2;
    const size_t planes = (size_t)n * c, total = planes * Hs * Ws;
    float* src = read_floats(f, planes * H * W);
    float* dst = (float*)malloc(total * sizeof(float));
    for (size_t i = 0; i < total; ++i) dst[i] = NAN;
    for (size_t idx = 0; idx < total; ++idx) {
        const int xd = (int)(idx % Ws);
        const size_t t = idx / Ws;
        const int y = (int)(t % Hs);
        const size_t p = t / Hs;
        const int x = flip ? Ws - 1 - xd : xd;
        const float* plane = src + p * ((size_t)H * W);
        dst[idx] = tta_resize_pixel([&](size_t i) { return plane[i]; }, H, W, Hs, Ws, y, x);
    }
    FILE* g = fopen(result, "wb");
    if (!g || fwrite(dst, sizeof(float), total, g) != total) return 1;
    fclose(g);
    free(src);
    free(dst);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_tta REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t op;
    if (!read_ints(f, &op, 1)) return 1;
    const int rc = op == 0 ? vote(f, argv[2]) : (op == 1 ? resize(f, argv[2]) : 1);
    fclose(f);
    return rc;
}
