// TEST INFRASTRUCTURE (never shipped, never imported by the product package).
//
// Drives the staging arithmetic of cutmix-semisup-seg_amd/csrc/stage_math.hpp on the host the way stage_kernel runs it for a batch
// of PAIRS of views (DeviceAugmenter.stage_pair): 2n rows over n entries of a ragged pool, no teacher output (out0 == NULL), the
// colour output serving both views, and the validity mask through stage_mask (params slot 23, the mask mode) -- so that the rows
// aug_pairs.pair_rows writes and the mask mode can be checked against oracle/augment.py on a CPU-only machine. The kernels'
// indexing and launch geometry are covered by the `-m gpu` tests.
//
// Build: tests/_hostcheck.py (shared object for the tests; `--sanitize`: a stand-alone driver under ASan + UBSan over an exactly
// sized pool whose last entry ends at the end of its allocation).
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../cutmix-semisup-seg_amd/csrc/stage_math.hpp"

using namespace cms;

namespace {

struct Entry {           // == cms_stage_entry
    long long img_off, lab_off;
    int hs, ws;
};

const int kParams = 24;  // == CMS_AUG_PARAMS

bool view_of(const uint8_t* pool_img, const Entry* entries, int n_entries, int e, StageSrc& sv) {
    sv.img = nullptr; sv.lab = nullptr; sv.Hs = 0; sv.Ws = 0;
    if ((unsigned)e >= (unsigned)n_entries) return false;
    const Entry& ent = entries[e];
    if (ent.hs <= 0 || ent.ws <= 0 || ent.img_off < 0) return false;
    sv.img = stage_entry_base(pool_img, ent.img_off);
    sv.Hs = ent.hs;
    sv.Ws = ent.ws;
    return true;
}

}  // namespace

extern "C" {

// stage_kernel<float> without labels: out0 / out1 (n,3,H,W) or NULL, out_mask (n,H,W)
void hc_pair_stage_batch(const uint8_t* pool_img, const void* entries, int n_entries, const int* index, int n, int H, int W,
                         const float* params, const float* mean, const float* std_, float* out0, float* out1, float* out_mask) {
    const size_t plane = (size_t)H * W;
    float inv_std[3];
    for (int c = 0; c < 3; ++c) inv_std[c] = 1.0f / std_[c];
    for (int s = 0; s < n; ++s) {
        StageSrc sv;
        const bool ok = view_of(pool_img, (const Entry*)entries, n_entries, index[s], sv);
        const float* p = params + (size_t)s * kParams;
        for (int i = 0; i < H * W; ++i) {
            const int oy = i / W, ox = i - oy * W;
            float rgb[3] = {0.0f, 0.0f, 0.0f};
            float alpha = 0.0f, img_alpha = 0.0f;
            int ny = -1, nx = -1;
            if (ok) {
                int cy, cx;
                stage_unflip(p, H, W, ox, oy, cx, cy);
                sample_source(sv, H, W, p, cx, cy, rgb, alpha, img_alpha, ny, nx);
            }
            float r = rgb[0] * (1.0f / 255.0f), g = rgb[1] * (1.0f / 255.0f), b = rgb[2] * (1.0f / 255.0f);
            const size_t o = (size_t)s * 3 * plane + (size_t)i;
            if (out0) {
                out0[o] = (r - mean[0] * img_alpha) * inv_std[0];
                out0[o + plane] = (g - mean[1] * img_alpha) * inv_std[1];
                out0[o + 2 * plane] = (b - mean[2] * img_alpha) * inv_std[2];
            }
            if (out1) {
                colour_chain(p, r, g, b);
                out1[o] = (r - mean[0] * img_alpha) * inv_std[0];
                out1[o + plane] = (g - mean[1] * img_alpha) * inv_std[1];
                out1[o + 2 * plane] = (b - mean[2] * img_alpha) * inv_std[2];
            }
            if (out_mask) out_mask[(size_t)s * plane + i] = ok ? stage_mask(sv, p, alpha, ny, nx) : 0.0f;
        }
    }
}

}  // extern "C"

#ifdef HC_STAGE_PAIR_MAIN
// Stand-alone driver for the host sanitizers: pairs of rows over a ragged pool in an EXACTLY sized heap allocation, both mask
// modes, windows past every edge and larger than the source (Hung pairs of a small source), a one-pixel source, warps thrown far
// outside, every flip, an out-of-range index and an empty entry. In mask mode 1 every mask value must be exactly 0 or 1.
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    const int sizes[][2] = {{37, 53}, {60, 70}, {48, 64}, {20, 90}, {90, 20}, {5, 3}, {1, 1}};
    const int n_real = 7;
    std::vector<Entry> ent(n_real + 1);
    long long ip = 0;
    for (int e = 0; e < n_real; ++e) {
        ip = (ip + 15) / 16 * 16;
        ent[e] = {ip, -1, sizes[e][0], sizes[e][1]};
        ip += (long long)sizes[e][0] * sizes[e][1] * 3;
    }
    ent[n_real] = {0, -1, 0, 0};                                  // an empty entry: stages as an empty source
    uint8_t* img = (uint8_t*)malloc((size_t)ip);                  // exactly sized: the last entry ends the allocation
    uint32_t seed = 4321u;
    for (long long i = 0; i < ip; ++i) img[i] = (uint8_t)lcg(seed);
    const int half[] = {6, 0, 3, 3, 1, 5, 2, 4, 99, -1, 7};
    const int n = (int)(sizeof(half) / sizeof(half[0]));
    std::vector<int> index(2 * n);
    for (int s = 0; s < 2 * n; ++s) index[s] = half[s % n];       // view-major: the n entries twice
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    double checksum = 0.0;
    int runs = 0;
    for (int H = 1; H <= 48; H += 47) {
        for (int sq = 0; sq < 2; ++sq) {
            const int W = sq ? H : (H == 1 ? 3 : 64);
            std::vector<float> o1((size_t)2 * n * 3 * H * W), mk((size_t)2 * n * H * W);
            for (int mode = 0; mode < 3; ++mode) {                // crop pair, Hung pair, warp pair
                std::vector<float> prm((size_t)2 * n * kParams, 0.0f);
                for (int s = 0; s < 2 * n; ++s) {
                    float* p = &prm[(size_t)s * kParams];
                    const int e = index[s], v = s / n;
                    const int hs = (e >= 0 && e < n_real) ? sizes[e][0] : 4, ws = (e >= 0 && e < n_real) ? sizes[e][1] : 4;
                    p[7] = p[8] = p[9] = 1.0f;
                    if (mode < 2) {
                        const int k = 5 + (int)(lcg(seed) % 11u);                     // Hung: f_scale = k / 10
                        const int sh = (mode == 1 && v == 1) ? (H * 10 + k / 2) / k : H, sw = (mode == 1 && v == 1) ? (W * 10 + k / 2) / k : W;
                        p[0] = (float)((int)(lcg(seed) % (unsigned)(hs + sh + 1)) - sh);
                        p[1] = (float)((int)(lcg(seed) % (unsigned)(ws + sw + 1)) - sw);
                        p[2] = (float)sh; p[3] = (float)sw;
                        p[23] = (float)(mode == 1 && v == 1);
                    } else {
                        const float th = 0.6f * (float)s - 2.0f, sc = 0.4f + 0.35f * (float)(s % 5);
                        p[15] = 1.0f; p[22] = 1.0f;
                        p[16] = sc * cosf(th); p[17] = sc * sinf(th); p[18] = (float)((int)(lcg(seed) % 400u) - 200);
                        p[19] = -sc * sinf(th); p[20] = sc * cosf(th); p[21] = (float)((int)(lcg(seed) % 400u) - 200);
                        p[2] = (float)H; p[3] = (float)W;
                        p[23] = (float)(s & 1);                                      // the mask mode is legal in warp rows too
                    }
                    p[4] = (float)(lcg(seed) & 1u); p[5] = (float)(lcg(seed) & 1u); p[6] = sq ? (float)(lcg(seed) & 1u) : 0.0f;
                    if (v == 1) {                                                     // the colour change of view 1
                        p[7] = 0.6f + 0.1f * (float)(s % 8); p[8] = 1.4f - 0.1f * (float)(s % 8); p[9] = 0.7f + 0.1f * (float)(s % 6);
                        p[10] = 0.02f * (float)(s % 7) - 0.06f; p[11] = (float)(s % 4 == 0); p[12] = (float)(s % 3 != 0);
                        p[13] = (float)0x1B; p[14] = 0.4f;
                    }
                }
                hc_pair_stage_batch(img, ent.data(), n_real + 1, index.data(), 2 * n, H, W, prm.data(), mean, sd, nullptr,
                                    o1.data(), mk.data());
                for (int s = 0; s < 2 * n; ++s) {
                    if (prm[(size_t)s * kParams + 23] == 0.0f) continue;
                    for (size_t i = 0; i < (size_t)H * W; ++i) {
                        const float m = mk[(size_t)s * H * W + i];
                        if (m != 0.0f && m != 1.0f) { printf("FAIL: mask mode 1 gave %g\n", (double)m); return 1; }
                    }
                }
                for (size_t i = 0; i < o1.size(); ++i) checksum += (double)o1[i];
                for (size_t i = 0; i < mk.size(); ++i) checksum += (double)mk[i];
                ++runs;
            }
        }
    }
    free(img);
    if (checksum != checksum) { printf("FAIL: NaN in the outputs\n"); return 1; }
    printf("hostcheck_stage_pair: %d runs over %d rows, checksum %.6f, no sanitizer report\n", runs, 2 * n, checksum);
    return 0;
}
#endif
