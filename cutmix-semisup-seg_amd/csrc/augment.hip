// Device-side input staging: crop (+ random scale), flip, colour augmentation, standardisation -- the per-sample CPU work
// of the reference's loader workers (datapipe/seg_transforms_cv.py:29-133 pad + crop, :169-231 random-scale crop,
// :452-497 flips, :541-585 torchvision ColorJitter / RandomGrayscale through PIL, :587-623 standardise + NCHW;
// wiring: train_seg_semisup_mask_mt.py:150-183) as ONE gather kernel over uint8 source images that already sit in HBM.
//
// Per output pixel: undo the flips, map into the source window (bilinear, cv2.INTER_LINEAR's half-pixel convention;
// nearest = floor for labels, cv2.INTER_NEAREST), zero / 255 / 0 outside the source image (the reference pads with an alpha
// channel so that padding is exactly 0 after standardisation, :46-52, 600-608), colour operations on the interpolated RGB,
// standardise, write NCHW. The paired layout of the unsupervised stream (SegTransformToPair + colour on sample 1 only)
// comes out of the same pass: `out0` = weakly augmented (teacher), `out1` = colour-augmented (student), same geometry.
//
// HBM-bound: reads <= 4 source pixels x 3 bytes per output pixel (L2-local), writes 3 * s bytes per output (x2 when
// paired). Random parameters are drawn on the host in the reference's order (device_pipeline.py) and arrive as a small
// table; nothing else crosses PCIe.
#include "common.hpp"
#include "stage_math.hpp"

namespace cms {

struct AugArgs {
    const uint8_t* src;         // [N][Hs][Ws][3]
    const uint8_t* src_labels;  // [N][Hs][Ws] or NULL
    void* out0;                 // (N,3,H,W) or NULL
    void* out1;                 // (N,3,H,W) colour-augmented copy or NULL
    uint8_t* out_labels;        // (N,H,W) or NULL
    float* out_mask;            // (N,1,H,W) or NULL
    const float* params;        // [N][CMS_AUG_PARAMS]
    float mean[3], inv_std[3];
    int N, Hs, Ws, H, W;
};

template <class T>
__global__ __launch_bounds__(256) void augment_kernel(AugArgs a) {
    const size_t total = (size_t)a.N * a.H * a.W;
    const size_t plane = (size_t)a.H * a.W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % a.W);
        const size_t t0 = i / a.W;
        const int oy = (int)(t0 % a.H);
        const int n = (int)(t0 / a.H);
        const float* p = a.params + (size_t)n * CMS_AUG_PARAMS;
        int cy, cx;
        stage_unflip(p, a.H, a.W, ox, oy, cx, cy);
        const StageSrc sv = {a.src + (size_t)n * a.Hs * a.Ws * 3, a.src_labels ? a.src_labels + (size_t)n * a.Hs * a.Ws : nullptr, a.Hs, a.Ws};
        float rgb[3];
        float alpha, img_alpha;
        int ny, nx;
        sample_source(sv, a.H, a.W, p, cx, cy, rgb, alpha, img_alpha, ny, nx);
        float r = rgb[0] * (1.0f / 255.0f), g = rgb[1] * (1.0f / 255.0f), b = rgb[2] * (1.0f / 255.0f);
        const size_t o = (size_t)n * 3 * plane + (size_t)oy * a.W + ox;
        if (a.out0) {
            put_as<T>(a.out0, o, (r - a.mean[0] * img_alpha) * a.inv_std[0]);
            put_as<T>(a.out0, o + plane, (g - a.mean[1] * img_alpha) * a.inv_std[1]);
            put_as<T>(a.out0, o + 2 * plane, (b - a.mean[2] * img_alpha) * a.inv_std[2]);
        }
        if (a.out1) {
            colour_chain(p, r, g, b);
            put_as<T>(a.out1, o, (r - a.mean[0] * img_alpha) * a.inv_std[0]);
            put_as<T>(a.out1, o + plane, (g - a.mean[1] * img_alpha) * a.inv_std[1]);
            put_as<T>(a.out1, o + 2 * plane, (b - a.mean[2] * img_alpha) * a.inv_std[2]);
        }
        if (a.out_mask) a.out_mask[(size_t)n * plane + (size_t)oy * a.W + ox] = stage_mask(sv, p, alpha, ny, nx);
        if (a.out_labels) a.out_labels[(size_t)n * plane + (size_t)oy * a.W + ox] = stage_label(sv, ny, nx);
    }
}

// mean luminance of the geometrically transformed image (the pivot of ColorJitter's contrast), one block per sample
__global__ __launch_bounds__(256) void augment_luma_kernel(AugArgs a, float* __restrict__ luma) {
    __shared__ float red[16];
    const int n = blockIdx.x;
    const float* p = a.params + (size_t)n * CMS_AUG_PARAMS;
    const StageSrc sv = {a.src + (size_t)n * a.Hs * a.Ws * 3, nullptr, a.Hs, a.Ws};
    float acc = 0.0f;
    for (int i = threadIdx.x; i < a.H * a.W; i += blockDim.x) {
        const int cy = i / a.W, cx = i % a.W;           // (flips do not change the mean)
        float rgb[3], alpha, img_alpha;
        int ny, nx;
        sample_source(sv, a.H, a.W, p, cx, cy, rgb, alpha, img_alpha, ny, nx);  // the image kernel's own taps and weights
        acc += gray_of(rgb[0], rgb[1], rgb[2]) * (1.0f / 255.0f);
    }
    float v[1] = {acc};
    block_sum<1>(v, red);
    if (threadIdx.x == 0) luma[n] = v[0] / (float)(a.H * a.W);
}

}  // namespace cms

using namespace cms;

static int aug_fill(AugArgs& a, const cms_augment_desc* d) {
    CMS_REQUIRE(d && d->src && d->params && (d->out0 || d->out1), "augment: NULL pointer");
    CMS_REQUIRE(d->n > 0 && d->hs > 0 && d->ws > 0 && d->h > 0 && d->w > 0, "augment: bad geometry");
    CMS_REQUIRE(d->out_dtype == CMS_F32 || d->out_dtype == CMS_BF16, "augment: bad output dtype");
    CMS_REQUIRE(d->std_[0] > 0 && d->std_[1] > 0 && d->std_[2] > 0, "augment: std must be positive");
    a.src = d->src; a.src_labels = d->src_labels; a.out0 = d->out0; a.out1 = d->out1; a.out_labels = d->out_labels;
    a.out_mask = d->out_mask; a.params = d->params;
    for (int i = 0; i < 3; ++i) { a.mean[i] = d->mean[i]; a.inv_std[i] = 1.0f / d->std_[i]; }
    a.N = d->n; a.Hs = d->hs; a.Ws = d->ws; a.H = d->h; a.W = d->w;
    return CMS_OK;
}

extern "C" int cms_augment_batch(const cms_augment_desc* d, void* stream) {
    AugArgs a;
    const int rc = aug_fill(a, d);
    if (rc) return rc;
    const size_t total = (size_t)a.N * a.H * a.W;
    hipStream_t s = (hipStream_t)stream;
    if (d->out_dtype == CMS_F32) hipLaunchKernelGGL(augment_kernel<float>, dim3(grid_for(total, 256, 256 * 16)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(augment_kernel<uint16_t>, dim3(grid_for(total, 256, 256 * 16)), dim3(256), 0, s, a);
    return launch_status("cms_augment_batch");
}

extern "C" int cms_augment_luma(const cms_augment_desc* d, float* luma, void* stream) {
    AugArgs a;
    CMS_REQUIRE(luma != nullptr, "augment_luma: NULL pointer");
    cms_augment_desc dd = *d;
    if (!dd.out0 && !dd.out1) dd.out0 = (void*)luma;      // (geometry check only)
    const int rc = aug_fill(a, &dd);
    if (rc) return rc;
    hipLaunchKernelGGL(augment_luma_kernel, dim3(a.N), dim3(256), 0, (hipStream_t)stream, a, luma);
    return launch_status("cms_augment_luma");
}
