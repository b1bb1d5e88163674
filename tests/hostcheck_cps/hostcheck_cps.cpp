// test infrastructure: a stand-alone host driver of the product's cross-pseudo-supervision arithmetic (csrc/cps_math.hpp, and through
// it the taps, gathers, box parity and softmax of csrc/pixel_math.hpp and the argmax order of csrc/tta_math.hpp), the very functions
// the kernel of csrc/cps.hip calls, walked sample by sample, workgroup by workgroup and thread by thread as the launch walks them.
//
//   hostcheck_cps REQUEST RESULT
//
// REQUEST, little-endian: int32 n, c, h, w, H, W, align_corners, n_boxes (0: a mask follows instead of a box table), invert, has_um0,
// has_um1, vec (0: the label maps start at an odd address and are written byte by byte); float32 conf_thresh; then the four
// (n, c, h, w) float32 logit tensors l0_a, l1_a, l0_b, l1_b; then the (n, n_boxes, 4) int32 box table or the (n, H, W) float32 mask;
// then, as announced, the (n, H, W) float32 maps um0 and um1.
// RESULT: n * H * W uint8 label_a, the same of label_b, 4 int64 counts (n_valid, kept_a, kept_b, agree).
// Every tensor lives in an exactly-sized heap block and the label maps are filled with 0xA5 before use, so a sanitizer build sees
// every byte outside them and a label the walk does not write shows in the result. Exit code 2 for a request the product refuses
// (the refusal is the product's own check).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cutmix-semisup-seg_amd/csrc/cps_math.hpp"
#include "../hostcheck_common.hpp"

using namespace cms;

template <int CT, bool IDENT, bool VEC>
static void walk(const CpsArgs& a, int64_t* stats) {
    const unsigned blocks = cps_blocks((long long)a.d.H * a.d.W);
    for (int n = 0; n < a.d.n; ++n)
        for (unsigned b = 0; b < blocks; ++b)
            for (int tid = 0; tid < kCpsBlock; ++tid) {
                CpsCounts k = {0, 0, 0, 0};
                cps_thread<CT, IDENT, VEC>(a, n, b, tid, k);
                stats[0] += k.n_valid, stats[1] += k.kept_a, stats[2] += k.kept_b, stats[3] += k.agree;
            }
}

template <int CT>
static void walk_ct(const CpsArgs& a, bool ident, bool vec, int64_t* stats) {
    if (ident) vec ? walk<CT, true, true>(a, stats) : walk<CT, true, false>(a, stats);
    else vec ? walk<CT, false, true>(a, stats) : walk<CT, false, false>(a, stats);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_cps REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[12];
    float tau;
    if (fread(head, sizeof(int32_t), 12, f) != 12 || fread(&tau, sizeof(float), 1, f) != 1) return 1;
    cms_cps_desc d;
    memset(&d, 0, sizeof(d));
    d.n = head[0], d.c = head[1], d.h = head[2], d.w = head[3], d.H = head[4], d.W = head[5], d.align_corners = head[6];
    d.n_boxes = head[7], d.invert = head[8], d.conf_thresh = tau;
    const bool has_um0 = head[9] != 0, has_um1 = head[10] != 0, vec = head[11] != 0;
    // the product's verdict on the sizes before anything is read or allocated by them
    alignas(16) static char probe[16];
    d.l0_a = d.l1_a = d.l0_b = d.l1_b = (const float*)probe;
    d.label_a = d.label_b = (uint8_t*)probe, d.stats = (int64_t*)probe;
    if (d.n_boxes > 0) d.ranges = (const int32_t*)probe;
    else d.mask = (const float*)probe;
    if (cps_check(&d)) return 2;
    const size_t pix = (size_t)d.n * d.H * d.W, lg = (size_t)d.n * d.c * d.h * d.w * sizeof(float);
    float* l[4];
    for (int i = 0; i < 4; ++i) l[i] = (float*)read_block(f, lg);
    int32_t* ranges = d.n_boxes > 0 ? (int32_t*)read_block(f, (size_t)d.n * d.n_boxes * 4 * sizeof(int32_t)) : nullptr;
    float* mask = d.n_boxes > 0 ? nullptr : (float*)read_block(f, pix * sizeof(float));
    float* um0 = has_um0 ? (float*)read_block(f, pix * sizeof(float)) : nullptr;
    float* um1 = has_um1 ? (float*)read_block(f, pix * sizeof(float)) : nullptr;
    fclose(f);
    const size_t skew = vec ? 0 : 1;
    uint8_t* la = (uint8_t*)malloc(pix + skew);
    uint8_t* lb = (uint8_t*)malloc(pix + skew);
    memset(la, 0xA5, pix + skew), memset(lb, 0xA5, pix + skew);
    int64_t stats[4] = {0, 0, 0, 0};
    d.l0_a = l[0], d.l1_a = l[1], d.l0_b = l[2], d.l1_b = l[3];
    d.ranges = ranges, d.mask = mask, d.um0 = um0, d.um1 = um1;
    d.label_a = la + skew, d.label_b = lb + skew, d.stats = stats;
    if (cps_check(&d)) return 2;

    CpsArgs a;
    cps_make_args(&d, &a);
    const bool ident = d.h == d.H && d.w == d.W;
    switch (cps_ct(d.c)) {
        case 19: walk_ct<19>(a, ident, vec, stats); break;
        case 21: walk_ct<21>(a, ident, vec, stats); break;
        default: walk_ct<0>(a, ident, vec, stats); break;
    }

    FILE* g = fopen(argv[2], "wb");
    if (!g) return 1;
    if (fwrite(la + skew, 1, pix, g) != pix || fwrite(lb + skew, 1, pix, g) != pix || fwrite(stats, 8, 4, g) != 4) return 1;
    fclose(g);
    for (int i = 0; i < 4; ++i) free(l[i]);
    free(ranges), free(mask), free(um0), free(um1), free(la), free(lb);
    return 0;
}
