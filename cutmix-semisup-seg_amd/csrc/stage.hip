// Ragged device-side input staging: augment.hip's gather, with every batch sample read from its OWN entry of a pool of
// variable-sized uint8 images resident in HBM (resident_pool.py) -- real data sets (Pascal VOC) have no common image size, and
// cms_augment_batch takes one (hs, ws) and a dense [N][hs][ws][3] source for the whole batch.
//
//   pool_img    one byte buffer; entry e holds [hs_e][ws_e][3] uint8 at byte offset entries[e].img_off (dense rows, 3 * ws_e bytes)
//   pool_labels one byte buffer; entry e holds [hs_e][ws_e] uint8 at entries[e].lab_off            (NULL: no labels)
//   index[n]    pool entry of batch sample n (any order, repeats allowed)
//
// The per-pixel arithmetic is stage_math.hpp's (the very functions augment.hip calls), so a pool whose entries all have one size
// gives cms_augment_batch's output bit for bit. Evaluation staging (whole images centred on a padded canvas) is the same kernel
// in window mode with a negative origin and scale 1.
//
// Work decomposition: blockIdx.y = batch sample, so the sample's table entry and its 24 parameters are wave-uniform and are read
// once per thread block into scalar registers before any store; blockIdx.x strides over the sample's H * W output pixels, one
// pixel per thread per trip, consecutive lanes on consecutive ox (coalesced plane writes; the <= 4 taps x 3 bytes per pixel are
// neighbours of the neighbouring lanes' taps and come from L2 / TCP). HBM-bound like the dense kernel: no LDS, no reuse to stage.
// All pool addressing is 64-bit (stage_entry_base): the augmented Pascal set is ~7 GB of pixels.
//
// Bounds: an index outside [0, n_entries) or an entry with a non-positive size stages as an EMPTY source (image 0, labels 255,
// mask 0) and reads nothing; otherwise window taps are bounds-tested and warp taps reflected into the entry's hs x ws pixels.
#include "common.hpp"
#include "stage_math.hpp"

namespace cms {

struct StageArgs {
    const uint8_t* pool_img;
    const uint8_t* pool_labels;     // or NULL
    const cms_stage_entry* entries;
    const int* index;               // [N]
    void* out0;
    void* out1;
    uint8_t* out_labels;
    float* out_mask;
    const float* params;            // [N][CMS_AUG_PARAMS]
    float mean[3], inv_std[3];
    int N, n_entries, H, W;
};

// the source view of batch sample n; false (and an empty view) when its index or entry is unusable
__device__ __forceinline__ bool stage_view(const StageArgs& a, int n, StageSrc& sv) {
    sv.img = nullptr; sv.lab = nullptr; sv.Hs = 0; sv.Ws = 0;
    const int e = a.index[n];
    if ((unsigned)e >= (unsigned)a.n_entries) return false;
    const cms_stage_entry ent = a.entries[e];
    if (ent.hs <= 0 || ent.ws <= 0 || ent.img_off < 0) return false;
    sv.img = stage_entry_base(a.pool_img, ent.img_off);
    sv.lab = (a.pool_labels && ent.lab_off >= 0) ? stage_entry_base(a.pool_labels, ent.lab_off) : nullptr;
    sv.Hs = ent.hs;
    sv.Ws = ent.ws;
    return true;
}

template <class T>
__global__ __launch_bounds__(256) void stage_kernel(StageArgs a) {
    const int n = blockIdx.y;
    // everything per sample is read here, before any store: uniform addresses, scalar loads
    StageSrc sv;
    const bool ok = stage_view(a, n, sv);
    float p[CMS_AUG_PARAMS];
#pragma unroll
    for (int k = 0; k < CMS_AUG_PARAMS; ++k) p[k] = a.params[(size_t)n * CMS_AUG_PARAMS + k];
    const int plane_i = a.H * a.W;
    const size_t plane = (size_t)plane_i;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plane_i; i += gridDim.x * blockDim.x) {
        const int oy = i / a.W, ox = i - oy * a.W;
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        float alpha = 0.0f, img_alpha = 0.0f;
        int ny = -1, nx = -1;
        if (ok) {
            int cy, cx;
            stage_unflip(p, a.H, a.W, ox, oy, cx, cy);
            sample_source(sv, a.H, a.W, p, cx, cy, rgb, alpha, img_alpha, ny, nx);
        }
        float r = rgb[0] * (1.0f / 255.0f), g = rgb[1] * (1.0f / 255.0f), b = rgb[2] * (1.0f / 255.0f);
        const size_t o = (size_t)n * 3 * plane + (size_t)i;
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
        if (a.out_mask) a.out_mask[(size_t)n * plane + (size_t)i] = ok ? stage_mask(sv, p, alpha, ny, nx) : 0.0f;
        if (a.out_labels) a.out_labels[(size_t)n * plane + (size_t)i] = ok ? stage_label(sv, ny, nx) : (uint8_t)255;
    }
}

// mean luminance of the geometrically transformed image (ColorJitter's contrast pivot), one block per sample: the summation
// order of augment_luma_kernel, so that a uniform pool gives its value bit for bit
__global__ __launch_bounds__(256) void stage_luma_kernel(StageArgs a, float* __restrict__ luma) {
    __shared__ float red[16];
    const int n = blockIdx.x;
    StageSrc sv;
    const bool ok = stage_view(a, n, sv);
    const float* p = a.params + (size_t)n * CMS_AUG_PARAMS;
    float acc = 0.0f;
    if (ok) {
        for (int i = threadIdx.x; i < a.H * a.W; i += blockDim.x) {
            const int cy = i / a.W, cx = i % a.W;           // (flips do not change the mean)
            float rgb[3], alpha, img_alpha;
            int ny, nx;
            sample_source(sv, a.H, a.W, p, cx, cy, rgb, alpha, img_alpha, ny, nx);  // the image kernel's own taps and weights
            acc += gray_of(rgb[0], rgb[1], rgb[2]) * (1.0f / 255.0f);
        }
    }
    float v[1] = {acc};
    block_sum<1>(v, red);
    if (threadIdx.x == 0) luma[n] = v[0] / (float)(a.H * a.W);
}

}  // namespace cms

using namespace cms;

static int stage_fill(StageArgs& a, const cms_stage_desc* d, bool need_out) {
    CMS_REQUIRE(d && d->pool_img && d->entries && d->index && d->params, "stage: NULL pointer");
    CMS_REQUIRE(!need_out || d->out0 || d->out1, "stage: no image output");
    CMS_REQUIRE(d->n > 0 && d->n <= 65535 && d->n_entries > 0 && d->h > 0 && d->w > 0, "stage: bad geometry");
    CMS_REQUIRE((long long)d->h * d->w < (1ll << 30), "stage: crop too large");
    CMS_REQUIRE(d->out_dtype == CMS_F32 || d->out_dtype == CMS_BF16, "stage: bad output dtype");
    CMS_REQUIRE(d->std_[0] > 0 && d->std_[1] > 0 && d->std_[2] > 0, "stage: std must be positive");
    a.pool_img = d->pool_img; a.pool_labels = d->pool_labels; a.entries = d->entries; a.index = d->index;
    a.out0 = d->out0; a.out1 = d->out1; a.out_labels = d->out_labels; a.out_mask = d->out_mask; a.params = d->params;
    for (int i = 0; i < 3; ++i) { a.mean[i] = d->mean[i]; a.inv_std[i] = 1.0f / d->std_[i]; }
    a.N = d->n; a.n_entries = d->n_entries; a.H = d->h; a.W = d->w;
    return CMS_OK;
}

extern "C" int cms_stage_batch(const cms_stage_desc* d, void* stream) {
    StageArgs a;
    const int rc = stage_fill(a, d, true);
    if (rc) return rc;
    const dim3 grid(grid_for((size_t)a.H * a.W, 256, 4096), a.N);
    hipStream_t s = (hipStream_t)stream;
    if (d->out_dtype == CMS_F32) hipLaunchKernelGGL(stage_kernel<float>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(stage_kernel<uint16_t>, grid, dim3(256), 0, s, a);
    return launch_status("cms_stage_batch");
}

extern "C" int cms_stage_luma(const cms_stage_desc* d, float* luma, void* stream) {
    StageArgs a;
    CMS_REQUIRE(luma != nullptr, "stage_luma: NULL pointer");
    const int rc = stage_fill(a, d, false);
    if (rc) return rc;
    hipLaunchKernelGGL(stage_luma_kernel, dim3(a.N), dim3(256), 0, (hipStream_t)stream, a, luma);
    return launch_status("cms_stage_luma");
}
