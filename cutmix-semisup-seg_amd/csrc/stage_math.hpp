// Per-pixel arithmetic of the device-side input staging, shared by the dense kernel (augment.hip: one source size for the whole
// batch) and the ragged kernel (stage.hip: every sample gathered from its own entry of a resident pool), and driven on the host
// by tests/hostcheck_stage. Same conventions as pixel_math.hpp / aug_math.hpp / ict_math.hpp: `__host__ __device__`, no state.
//
// Reference behaviour restated here (paths relative to the upstream repository; see augment.hip's header for the whole chain):
//   crop / pad           datapipe/seg_transforms_cv.py:29-133    window with a zero-padded alpha channel
//   random-scale crop    :169-231                                cv2.resize: INTER_LINEAR image, INTER_NEAREST labels
//   rotate + scale crop  :306-372                                cv2.warpAffine: REFLECT_101 image, labels 255 / mask 0 outside
//   flips                :452-497                                x flip, y flip, transpose -- applied after the crop
//   colour               :541-585                                torchvision ColorJitter / RandomGrayscale
//   standardise          :587-623                                (x - mean * alpha) / std, NCHW
//
// Addressing: a source is described by its base pointer and its own (Hs, Ws); rows are dense (3 * Ws bytes). Every tap is either
// bounds-tested against (Hs, Ws) (window mode) or reflected into it (warp mode), so nothing outside the Hs * Ws pixels of the
// source is read. A pool entry's base is `pool + byte offset` with a 64-bit offset (stage_entry_base): pools exceed 4 GB.
#pragma once
#include "pixel_math.hpp"

namespace cms {

// one source image: `img` [Hs][Ws][3] uint8, `lab` [Hs][Ws] uint8 or NULL
struct StageSrc {
    const uint8_t* img;
    const uint8_t* lab;
    int Hs, Ws;
};

// byte address of a pool entry (64-bit offsets; never narrowed)
CMS_HD const uint8_t* stage_entry_base(const uint8_t* pool, long long byte_off) {
    return pool + (size_t)(unsigned long long)byte_off;
}

CMS_HD int stage_imin(int a, int b) { return a < b ? a : b; }

CMS_HD float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

CMS_HD float gray_of(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

CMS_HD void hue_shift(float& r, float& g, float& b, float dh) {
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
    const float d = mx - mn;
    float h = 0.0f;
    if (d > 0.0f) {
        if (mx == r) h = (g - b) / d;
        else if (mx == g) h = 2.0f + (b - r) / d;
        else h = 4.0f + (r - g) / d;
        h *= (1.0f / 6.0f);
        if (h < 0.0f) h += 1.0f;
    }
    const float s = mx > 0.0f ? d / mx : 0.0f, v = mx;
    h += dh;
    h -= floorf(h);
    const float hf = h * 6.0f;
    const int i = (int)hf % 6;
    const float f = hf - floorf(hf);
    const float p = v * (1.0f - s), q = v * (1.0f - s * f), t = v * (1.0f - s * (1.0f - f));
    switch (i) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
    }
}

// cv2.BORDER_REFLECT_101: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ... (period 2n - 2), any distance outside
CMS_HD int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// AFFINE WARP geometry (params slot 15 == 1): source position of (flip-undone) output pixel (cx, cy)
CMS_HD void warp_src(const float* p, int cx, int cy, float& sx, float& sy) {
    sx = fmaf(p[16], (float)cx, fmaf(p[17], (float)cy, p[18]));
    sy = fmaf(p[19], (float)cx, fmaf(p[20], (float)cy, p[21]));
}

// undo the flips of output pixel (ox, oy) (applied after the crop in the reference: x flip, y flip, transpose)
CMS_HD void stage_unflip(const float* p, int H, int W, int ox, int oy, int& cx, int& cy) {
    cy = oy;
    cx = ox;
    if (p[6] != 0.0f) { const int t = cy; cy = cx; cx = t; }
    if (p[5] != 0.0f) cy = H - 1 - cy;
    if (p[4] != 0.0f) cx = W - 1 - cx;
}

// The geometric half of the transform for ONE (flip-undone) output pixel (cx, cy) of an (H, W) crop from source `s`:
// interpolated source colour (0..255), validity weight `alpha`, `img_alpha` = factor of the mean in the standardisation (window
// mode: zero padding), (ny, nx) = nearest source pixel for the labels. Shared by the image kernels and the luminance pre-passes,
// so that the contrast pivot is the mean of exactly the pixels the image kernel produces (same taps, same weights).
CMS_HD void sample_source(const StageSrc& s, int H, int W, const float* p, int cx, int cy, float (&rgb)[3], float& alpha,
                          float& img_alpha, int& ny, int& nx) {
    const uint8_t* img = s.img;
    const int Hs = s.Hs, Ws = s.Ws;
    const float y0 = p[0], x0 = p[1], sh = p[2], sw = p[3];
    const bool warp = p[15] != 0.0f;
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    alpha = 0.0f;
    img_alpha = 1.0f;
    ny = nx = 0;
    if (warp) {
        // datapipe/seg_transforms_cv.py:344-362: cv2.warpAffine(image, local_xf, crop, flags=interp, BORDER_REFLECT_101),
        // labels INTER_NEAREST / constant 255, mask constant 0
        float sx, sy;
        warp_src(p, cx, cy, sx, sy);
        nx = (int)floorf(sx + 0.5f);
        ny = (int)floorf(sy + 0.5f);
        if (p[22] == 0.0f) {
            const uint8_t* q = img + ((size_t)reflect101(ny, Hs) * Ws + reflect101(nx, Ws)) * 3;
            rgb[0] = (float)q[0]; rgb[1] = (float)q[1]; rgb[2] = (float)q[2];
            alpha = ((unsigned)ny < (unsigned)Hs && (unsigned)nx < (unsigned)Ws) ? 1.0f : 0.0f;
        } else {
            const int ix0 = (int)floorf(sx), iy0 = (int)floorf(sy);
            const float wx = sx - (float)ix0, wy = sy - (float)iy0;
            auto wtap = [&](int Y, int X, float w) {
                const uint8_t* q = img + ((size_t)reflect101(Y, Hs) * Ws + reflect101(X, Ws)) * 3;
                rgb[0] += w * (float)q[0];
                rgb[1] += w * (float)q[1];
                rgb[2] += w * (float)q[2];
                if ((unsigned)Y < (unsigned)Hs && (unsigned)X < (unsigned)Ws) alpha += w;
            };
            wtap(iy0, ix0, (1.0f - wy) * (1.0f - wx));
            wtap(iy0, ix0 + 1, (1.0f - wy) * wx);
            wtap(iy0 + 1, ix0, wy * (1.0f - wx));
            wtap(iy0 + 1, ix0 + 1, wy * wx);
        }
    } else {
        // bilinear tap positions inside the source window (cv2.INTER_LINEAR: half-pixel centres, border replicated)
        float fy = ((float)cy + 0.5f) * (sh / (float)H) - 0.5f, fx = ((float)cx + 0.5f) * (sw / (float)W) - 0.5f;
        fy = fminf(fmaxf(fy, 0.0f), sh - 1.0f);
        fx = fminf(fmaxf(fx, 0.0f), sw - 1.0f);
        const int iy0 = (int)floorf(fy), ix0 = (int)floorf(fx);
        const float wy = fy - (float)iy0, wx = fx - (float)ix0;
        const int iy1 = stage_imin(iy0 + 1, (int)sh - 1), ix1 = stage_imin(ix0 + 1, (int)sw - 1);
        const int Y0 = iy0 + (int)y0, Y1 = iy1 + (int)y0, X0 = ix0 + (int)x0, X1 = ix1 + (int)x0;
        auto tap = [&](int Y, int X, float w) {
            if (w != 0.0f && (unsigned)Y < (unsigned)Hs && (unsigned)X < (unsigned)Ws) {
                const uint8_t* q = img + ((size_t)Y * Ws + X) * 3;
                rgb[0] += w * (float)q[0];
                rgb[1] += w * (float)q[1];
                rgb[2] += w * (float)q[2];
                alpha += w;
            }
        };
        tap(Y0, X0, (1.0f - wy) * (1.0f - wx));
        tap(Y0, X1, (1.0f - wy) * wx);
        tap(Y1, X0, wy * (1.0f - wx));
        tap(Y1, X1, wy * wx);
        img_alpha = alpha;
        // cv2.INTER_NEAREST: floor(dst * scale)
        ny = stage_imin((int)((float)cy * (sh / (float)H)), (int)sh - 1) + (int)y0;
        nx = stage_imin((int)((float)cx * (sw / (float)W)), (int)sw - 1) + (int)x0;
    }
}

// label of the nearest source pixel (ny, nx) from sample_source; 255 outside the source or without a label map
CMS_HD uint8_t stage_label(const StageSrc& s, int ny, int nx) {
    if (s.lab && (unsigned)ny < (unsigned)s.Hs && (unsigned)nx < (unsigned)s.Ws) return s.lab[(size_t)ny * s.Ws + nx];
    return 255;
}

// The validity mask of one output pixel from what sample_source returned (params slot 23, the mask mode): 0 = `alpha`, the
// in-bounds weight of the image taps (cv2.INTER_LINEAR of the mask: single views, :215, and warps); 1 = whether the NEAREST source
// pixel (ny, nx) lies inside the source (cv2.INTER_NEAREST of the mask: view 1 of a Hung pair, :272). The image's `img_alpha` is
// the linear weight in both modes (the reference resizes the image's alpha channel linearly). No memory is read.
CMS_HD float stage_mask(const StageSrc& s, const float* p, float alpha, int ny, int nx) {
    if (p[23] == 0.0f) return alpha;
    return ((unsigned)ny < (unsigned)s.Hs && (unsigned)nx < (unsigned)s.Ws) ? 1.0f : 0.0f;
}

// The colour half (student view): RandomApply(ColorJitter) in the drawn order, then RandomGrayscale; r, g, b in [0, 1]
CMS_HD void colour_chain(const float* p, float& r, float& g, float& b) {
    if (p[12] != 0.0f) {                       // ColorJitter applied (RandomApply, p = aug_colour_prob)
        const int order = (int)p[13];          // permutation index of (brightness, contrast, saturation, hue)
        // decode the permutation: order = ((i0 * 4 + i1) * 4 + i2) * 4 + i3
        const int ops[4] = {(order >> 6) & 3, (order >> 4) & 3, (order >> 2) & 3, order & 3};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            switch (ops[k]) {
            case 0: r = clamp01(r * p[7]); g = clamp01(g * p[7]); b = clamp01(b * p[7]); break;
            case 1: {
                const float m = p[14];          // mean luminance at the time contrast is applied (pre-pass)
                r = clamp01((r - m) * p[8] + m); g = clamp01((g - m) * p[8] + m); b = clamp01((b - m) * p[8] + m);
                break;
            }
            case 2: {
                const float gr = gray_of(r, g, b);
                r = clamp01((r - gr) * p[9] + gr); g = clamp01((g - gr) * p[9] + gr); b = clamp01((b - gr) * p[9] + gr);
                break;
            }
            default: if (p[10] != 0.0f) hue_shift(r, g, b, p[10]); break;
            }
        }
    }
    if (p[11] != 0.0f) {                       // RandomGrayscale
        const float gr = gray_of(r, g, b);
        r = g = b = gr;
    }
}

}  // namespace cms
