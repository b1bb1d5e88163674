// test infrastructure: a stand-alone host driver of the product's ClassMix arithmetic (csrc/classmix_math.hpp, and through it the
// single-view pixel of csrc/tta_math.hpp), the very functions the kernels of csrc/classmix.hip call, walked sample by sample,
// workgroup by workgroup and thread by thread as the two launches walk them.
//
//   hostcheck_classmix REQUEST RESULT
//
// REQUEST, little-endian: int32 n, c, h, w, H, W, align_corners, has_valid; then n * c float64 keys; then the (n, c, h, w) float32
// logits; then, with has_valid, the (n, H, W) float32 validity map.
// RESULT: n * H * W uint8 predictions, n uint64 present sets, n uint64 chosen sets, n * H * W float32 mask.
// Every tensor and the workspace live in exactly-sized heap blocks, and the workspace is filled with 0xA5 before use, so a
// sanitizer build sees every byte outside them and a slot word that pass 2 reads without pass 1 having written it shows in the
// result. Exit code 2 for a request the product refuses (the refusal is the product's own check).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cutmix-semisup-seg_amd/csrc/classmix_math.hpp"
#include "../hostcheck_common.hpp"

using namespace cms;

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_classmix REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[8];
    if (fread(head, sizeof(int32_t), 8, f) != 8) return 1;
    cms_classmix_desc d;
    memset(&d, 0, sizeof(d));
    d.n = head[0], d.c = head[1], d.h = head[2], d.w = head[3], d.H = head[4], d.W = head[5], d.align_corners = head[6];
    const bool has_valid = head[7] != 0;
    // the product's verdict on the sizes before anything is read or allocated by them
    alignas(16) static char probe[16];
    d.logits = (const float*)probe, d.keys = (const double*)probe, d.mask_out = (float*)probe, d.workspace = probe;
    d.workspace_bytes = (size_t)-1;
    if (classmix_check(&d)) return 2;
    const size_t hw = (size_t)d.H * d.W, pix = (size_t)d.n * hw;
    double* keys = (double*)read_block(f, (size_t)d.n * d.c * sizeof(double));
    float* logits = (float*)read_block(f, (size_t)d.n * d.c * d.h * d.w * sizeof(float));
    float* valid = has_valid ? (float*)read_block(f, pix * sizeof(float)) : nullptr;
    fclose(f);
    const size_t ws_bytes = classmix_workspace_bytes(d.n, d.H, d.W);
    unsigned char* ws = (unsigned char*)aligned_alloc(16, ws_bytes);
    memset(ws, 0xA5, ws_bytes);
    float* mask = (float*)malloc(pix * sizeof(float));
    unsigned long long* present_out = (unsigned long long*)malloc(d.n * sizeof(unsigned long long));
    unsigned long long* chosen_out = (unsigned long long*)malloc(d.n * sizeof(unsigned long long));
    d.logits = logits, d.keys = keys, d.valid = valid, d.mask_out = mask, d.workspace = ws, d.workspace_bytes = ws_bytes;
    if (classmix_check(&d)) return 2;

    TtaViews v;
    classmix_views(&d, &v);
    const int chunk = classmix_chunk((long long)hw), nslots = classmix_slots((long long)hw);
    unsigned long long* slots = (unsigned long long*)ws;
    uint8_t* pred = ws + classmix_pred_offset(d.n);
    const bool ident = d.h == d.H && d.w == d.W;

    // ---- pass 1: grid (nslots, n), 256 threads
    for (int n = 0; n < d.n; ++n)
        for (int b = 0; b < nslots; ++b) {
            const size_t base = (size_t)n * hw, lo = (size_t)b * chunk, hi = lo + chunk < hw ? lo + chunk : hw;
            unsigned long long wave_bits[kCmBlock / 64] = {0, 0, 0, 0};
            for (int tid = 0; tid < kCmBlock; ++tid) {
                unsigned long long bits = 0ull;
                for (size_t p = lo + tid; p < hi; p += kCmBlock) {
                    const int y = (int)(p / d.W), x = (int)(p - (size_t)y * d.W);
                    const int best = ident ? tta_single_pixel<true>(v, n, d.c, y, x, d.align_corners != 0)
                                           : tta_single_pixel<false>(v, n, d.c, y, x, d.align_corners != 0);
                    pred[base + p] = (uint8_t)best;
                    bits |= classmix_bit(best, valid ? valid[base + p] != 0.0f : true);
                }
                wave_bits[tid / 64] |= bits;
            }
            slots[(size_t)n * kCmMaxSlots + b] = wave_bits[0] | wave_bits[1] | wave_bits[2] | wave_bits[3];
        }

    // ---- pass 2: grid (nslots, n), 256 threads
    for (int n = 0; n < d.n; ++n)
        for (int b = 0; b < nslots; ++b) {
            unsigned long long present = 0ull, chosen = 0ull;
            for (int lane = 0; lane < 64; ++lane)
                for (int i = lane; i < nslots; i += 64) present |= slots[(size_t)n * kCmMaxSlots + i];
            const double* krow = keys + (size_t)n * d.c;
            for (int lane = 0; lane < 64; ++lane)
                if (classmix_is_chosen(present, [&](int c) { return krow[c]; }, d.c, lane)) chosen |= 1ull << lane;
            if (b == 0) present_out[n] = present, chosen_out[n] = chosen;
            const size_t start = (size_t)n * hw, end = start + hw;
            auto one = [&](size_t i) { mask[i] = classmix_mask_value(chosen, pred[i], valid ? valid[i] != 0.0f : true); };
            const CmSplit sp = classmix_split(start, end);
            for (int tid = 0; tid < kCmBlock; ++tid) {
                for (size_t g = sp.vec_lo / 4 + (size_t)b * kCmBlock + tid; g < sp.vec_hi / 4; g += (size_t)nslots * kCmBlock)
                    for (int j = 0; j < 4; ++j) one(4 * g + j);
                if (b == 0) {
                    const size_t head_n = sp.vec_lo - start, tail_n = end - sp.vec_hi;
                    if ((size_t)tid < head_n) one(start + tid);
                    else if (tid - head_n < tail_n) one(sp.vec_hi + (tid - head_n));
                }
            }
        }

    FILE* g = fopen(argv[2], "wb");
    if (!g) return 1;
    if (fwrite(pred, 1, pix, g) != pix || fwrite(present_out, 8, d.n, g) != (size_t)d.n || fwrite(chosen_out, 8, d.n, g) != (size_t)d.n ||
        fwrite(mask, 4, pix, g) != pix)
        return 1;
    fclose(g);
    free(keys), free(logits), free(valid), free(ws), free(mask), free(present_out), free(chosen_out);
    return 0;
}
