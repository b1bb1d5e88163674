// TEST INFRASTRUCTURE (never shipped, never imported by the product package).
//
// Drives the `__host__ __device__` per-pixel arithmetic of cutmix-semisup-seg_amd/csrc/stage_math.hpp -- the code the dense and
// the ragged staging kernels (augment.hip, stage.hip) inline -- in plain host loops over a RAGGED pool: every batch sample is read
// from its own entry (own size, own 64-bit byte offset), exactly as stage_kernel / stage_luma_kernel do, so that the geometry, the
// bounds handling and the colour chain can be checked against oracle/augment.py on a CPU-only machine. The kernels' indexing and
// launch geometry are covered by the `-m gpu` tests.
//
// Build: tests/_hostcheck.py (shared object for the tests; `--sanitize`: a stand-alone driver under ASan + UBSan over an exactly
// sized pool whose last entry ends at the end of its allocation).
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../cutmix-semisup-seg_amd/csrc/stage_math.hpp"

using namespace cms;

namespace {

struct Entry {           // == cms_stage_entry
    long long img_off, lab_off;
    int hs, ws;
};

const int kParams = 24;  // == CMS_AUG_PARAMS

bool view_of(const uint8_t* pool_img, const uint8_t* pool_lab, const Entry* entries, int n_entries, int e, StageSrc& sv) {
    sv.img = nullptr; sv.lab = nullptr; sv.Hs = 0; sv.Ws = 0;
    if ((unsigned)e >= (unsigned)n_entries) return false;
    const Entry& ent = entries[e];
    if (ent.hs <= 0 || ent.ws <= 0 || ent.img_off < 0) return false;
    sv.img = stage_entry_base(pool_img, ent.img_off);
    sv.lab = (pool_lab && ent.lab_off >= 0) ? stage_entry_base(pool_lab, ent.lab_off) : nullptr;
    sv.Hs = ent.hs;
    sv.Ws = ent.ws;
    return true;
}

}  // namespace

extern "C" {

// the byte address of an entry, as an integer: no memory is touched
unsigned long long hc_stage_entry_address(unsigned long long pool_base, long long byte_off) {
    return (unsigned long long)(uintptr_t)stage_entry_base((const uint8_t*)(uintptr_t)pool_base, byte_off);
}

// luma[n] = mean luminance of sample n after its geometric transform (stage_luma_kernel; sequential fp32 sum here)
void hc_stage_luma(const uint8_t* pool_img, const void* entries, int n_entries, const int* index, int n, int H, int W,
                   const float* params, float* luma) {
    for (int s = 0; s < n; ++s) {
        StageSrc sv;
        const bool ok = view_of(pool_img, nullptr, (const Entry*)entries, n_entries, index[s], sv);
        const float* p = params + (size_t)s * kParams;
        double acc = 0.0;
        if (ok) {
            for (int i = 0; i < H * W; ++i) {
                float rgb[3], alpha, img_alpha;
                int ny, nx;
                sample_source(sv, H, W, p, i % W, i / W, rgb, alpha, img_alpha, ny, nx);
                acc += (double)(gray_of(rgb[0], rgb[1], rgb[2]) * (1.0f / 255.0f));
            }
        }
        luma[s] = (float)(acc / (double)(H * W));
    }
}

// stage_kernel<float>: out0 / out1 (n,3,H,W) or NULL, out_labels (n,H,W) or NULL, out_mask (n,H,W) or NULL
void hc_stage_batch(const uint8_t* pool_img, const uint8_t* pool_lab, const void* entries, int n_entries, const int* index, int n,
                    int H, int W, const float* params, const float* mean, const float* std_, float* out0, float* out1,
                    uint8_t* out_labels, float* out_mask) {
    const size_t plane = (size_t)H * W;
    float inv_std[3];
    for (int c = 0; c < 3; ++c) inv_std[c] = 1.0f / std_[c];
    for (int s = 0; s < n; ++s) {
        StageSrc sv;
        const bool ok = view_of(pool_img, pool_lab, (const Entry*)entries, n_entries, index[s], sv);
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
            if (out_mask) out_mask[(size_t)s * plane + i] = alpha;
            if (out_labels) out_labels[(size_t)s * plane + i] = ok ? stage_label(sv, ny, nx) : (uint8_t)255;
        }
    }
}

}  // extern "C"

#ifdef HC_STAGE_MAIN
// Stand-alone driver for the host sanitizers: a ragged pool in EXACTLY sized heap allocations (the last entry ends at the end of
// the buffer, so any read past an entry's Hs * Ws pixels is a heap overflow ASan reports), every geometry the kernels have --
// windows reaching past all four edges, windows larger than the source, a one-pixel source, warps (nearest and bilinear) thrown
// far outside, every flip, the colour chain, the evaluation canvas -- plus an out-of-range index and an empty entry.
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    const int sizes[][2] = {{37, 53}, {60, 70}, {48, 64}, {20, 90}, {90, 20}, {5, 3}, {1, 1}};
    const int n_real = 7;
    std::vector<Entry> ent(n_real + 1);
    long long ip = 0, lp = 0;
    for (int e = 0; e < n_real; ++e) {
        ip = (ip + 15) / 16 * 16; lp = (lp + 15) / 16 * 16;
        ent[e] = {ip, lp, sizes[e][0], sizes[e][1]};
        ip += (long long)sizes[e][0] * sizes[e][1] * 3;
        lp += (long long)sizes[e][0] * sizes[e][1];
    }
    ent[n_real] = {0, 0, 0, 0};                                   // an empty entry: stages as an empty source
    uint8_t* img = (uint8_t*)malloc((size_t)ip);                  // exactly sized: the last entry ends the allocation
    uint8_t* lab = (uint8_t*)malloc((size_t)lp);
    uint32_t seed = 12345u;
    for (long long i = 0; i < ip; ++i) img[i] = (uint8_t)lcg(seed);
    for (long long i = 0; i < lp; ++i) lab[i] = (uint8_t)(lcg(seed) % 21);
    const int index[] = {6, 0, 3, 3, 1, 5, 2, 4, 6, 5, 99, -1, 7};
    const int n = (int)(sizeof(index) / sizeof(index[0]));
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    double checksum = 0.0;
    int runs = 0;
    for (int H = 1; H <= 48; H += 47) {
        for (int sq = 0; sq < 2; ++sq) {
            const int W = sq ? H : (H == 1 ? 3 : 64);
            std::vector<float> o0((size_t)n * 3 * H * W), o1(o0.size()), mk((size_t)n * H * W), luma(n);
            std::vector<uint8_t> ol((size_t)n * H * W);
            for (int mode = 0; mode < 6; ++mode) {
                std::vector<float> prm((size_t)n * kParams, 0.0f);
                for (int s = 0; s < n; ++s) {
                    float* p = &prm[(size_t)s * kParams];
                    const int e = index[s];
                    const int hs = (e >= 0 && e < n_real) ? sizes[e][0] : 4, ws = (e >= 0 && e < n_real) ? sizes[e][1] : 4;
                    p[7] = p[8] = p[9] = 1.0f;
                    if (mode < 3) {                 // windows: inside / past every edge / much larger than the source
                        const int sh = mode == 0 ? H : (mode == 1 ? 2 * H : (H + 1) / 2), sw = mode == 0 ? W : (mode == 1 ? 2 * W : (W + 1) / 2);
                        p[0] = (float)((int)(lcg(seed) % (unsigned)(hs + sh + 1)) - sh);
                        p[1] = (float)((int)(lcg(seed) % (unsigned)(ws + sw + 1)) - sw);
                        p[2] = (float)sh; p[3] = (float)sw;
                    } else if (mode < 5) {          // warps: rotate + scale about a point that may lie far outside
                        const float th = 0.6f * (float)s - 2.0f, sc = 0.4f + 0.35f * (float)(s % 5);
                        p[15] = 1.0f;
                        p[16] = sc * cosf(th); p[17] = sc * sinf(th); p[18] = (float)((int)(lcg(seed) % 400u) - 200);
                        p[19] = -sc * sinf(th); p[20] = sc * cosf(th); p[21] = (float)((int)(lcg(seed) % 400u) - 200);
                        p[22] = (float)(mode - 3);
                        p[2] = (float)H; p[3] = (float)W;
                    } else {                        // evaluation canvas: negative origin, scale 1
                        p[0] = -(float)((H - hs) / 2); p[1] = -(float)((W - ws) / 2); p[2] = (float)H; p[3] = (float)W;
                    }
                    p[4] = (float)(lcg(seed) & 1u); p[5] = (float)(lcg(seed) & 1u); p[6] = sq ? (float)(lcg(seed) & 1u) : 0.0f;
                    p[7] = 0.6f + 0.1f * (float)(s % 8); p[8] = 1.4f - 0.1f * (float)(s % 8); p[9] = 0.7f + 0.1f * (float)(s % 6);
                    p[10] = 0.02f * (float)(s % 7) - 0.06f; p[11] = (float)(s % 4 == 0); p[12] = (float)(s % 3 != 0);
                    const int perms[4] = {0x1B, 0xE4, 0x4E, 0xB1};        // 0123, 3210, 1032, 2301
                    p[13] = (float)perms[s % 4];
                }
                hc_stage_luma(img, ent.data(), n_real + 1, index, n, H, W, prm.data(), luma.data());
                for (int s = 0; s < n; ++s) prm[(size_t)s * kParams + 14] = luma[s];
                hc_stage_batch(img, lab, ent.data(), n_real + 1, index, n, H, W, prm.data(), mean, sd, o0.data(), o1.data(),
                               ol.data(), mk.data());
                hc_stage_batch(img, nullptr, ent.data(), n_real + 1, index, n, H, W, prm.data(), mean, sd, o0.data(), nullptr,
                               ol.data(), nullptr);
                for (size_t i = 0; i < o0.size(); ++i) checksum += (double)o0[i] + (double)o1[i];
                for (size_t i = 0; i < mk.size(); ++i) checksum += (double)mk[i] + (double)ol[i];
                ++runs;
            }
        }
    }
    // 64-bit addressing: an entry above 2^32 (address arithmetic only)
    const unsigned long long base = 0x7f0000000000ull, off = (5ull << 32) + 48ull;
    if (hc_stage_entry_address(base, (long long)off) != base + off) { printf("FAIL: 64-bit entry address\n"); return 1; }
    free(img);
    free(lab);
    if (checksum != checksum) { printf("FAIL: NaN in the outputs\n"); return 1; }
    printf("hostcheck_stage: %d runs over %d samples, checksum %.6f, no sanitizer report\n", runs, n, checksum);
    return 0;
}
#endif
