// Test-time augmentation kernels (gfx950): the resize that makes a scaled / mirrored view's input, and the fused vote over the
// views' low-resolution logits. The reference evaluates at one scale without a flip (train_seg_semisup_mask_mt.py:510-514); written
// with tensor operations, a vote over K views materialises K tensors of (N, C, H, W) probabilities. Here a thread owns an output
// pixel: per view it gathers the view's logits (L2-resident low-resolution maps) three times -- maximum, normaliser, probabilities --
// and adds the probabilities into its column of an LDS score table [C][256]; only the uint8 prediction and the C x C histogram
// (csrc/eval.hip's: LDS integer atomics, one 64-bit atomic per non-empty bin) leave the kernel. With one view the scores are the
// logits themselves and the kernel is eval.hip's, bit for bit. The arithmetic is csrc/tta_math.hpp's.
#include "common.hpp"
#include "tta_math.hpp"

namespace cms {

constexpr int kTtaBlock = 256;

// MODE 0: one view of the output's size (no interpolation), 1: one view, resampled, 2: the vote over k >= 2 views
template <int MODE>
__global__ __launch_bounds__(kTtaBlock) void tta_vote_kernel(const TtaViews v, int k, const void* labels, int label_dtype,
                                                             int ignore_index, int N, int C, int H, int W, int align,
                                                             unsigned long long* __restrict__ cm,
                                                             uint8_t* __restrict__ pred_out) {
    extern __shared__ __attribute__((aligned(16))) float tta_smem[];
    float* score = tta_smem;                                                             // MODE 2: [C][kTtaBlock]
    unsigned int* hist = reinterpret_cast<unsigned int*>(tta_smem + (MODE == 2 ? C * kTtaBlock : 0));   // [C][C]
    const bool count = labels != nullptr && cm != nullptr;
    if (count) {
        for (int i = threadIdx.x; i < C * C; i += kTtaBlock) hist[i] = 0;
    }
    __syncthreads();
    const size_t P = (size_t)N * H * W;
    for (size_t idx = (size_t)blockIdx.x * kTtaBlock + threadIdx.x; idx < P; idx += (size_t)gridDim.x * kTtaBlock) {
        const int x = (int)(idx % W);
        const size_t t = idx / W;
        const int y = (int)(t % H);
        const int n = (int)(t / H);
        int best = 0;
        if (MODE == 2) {
            best = tta_vote_pixel(v, k, n, C, y, x, align != 0, [&](int c) -> float& { return score[c * kTtaBlock + threadIdx.x]; });
        } else {
            best = tta_single_pixel<MODE == 0>(v, n, C, y, x, align != 0);
        }
        if (pred_out) pred_out[idx] = (uint8_t)best;
        if (count) {
            const int tr = tta_label(labels, label_dtype, idx);
            if (tr != ignore_index && tr >= 0 && tr < C) atomicAdd(&hist[tr * C + best], 1u);
        }
    }
    __syncthreads();
    if (count) {
        for (int i = threadIdx.x; i < C * C; i += kTtaBlock) {
            const unsigned int val = hist[i];
            if (val) atomicAdd(&cm[i], (unsigned long long)val);
        }
    }
}

// one thread per element of dst; T = float or uint16_t (bf16 bits)
template <class T>
__global__ __launch_bounds__(256) void tta_resize_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t planes, int H, int W,
                                                         int Hs, int Ws, int flip) {
    const size_t total = planes * Hs * Ws;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int xd = (int)(idx % Ws);
        const size_t t = idx / Ws;
        const int y = (int)(t % Hs);
        const size_t p = t / Hs;
        const int x = flip ? Ws - 1 - xd : xd;
        const T* plane = src + p * ((size_t)H * W);
        const float val = tta_resize_pixel(
            [&](size_t i) {
                if constexpr (sizeof(T) == 4) return plane[i];
                else return bf16_to_f32(plane[i]);
            },
            H, W, Hs, Ws, y, x);
        put_as<T>(dst, idx, val);
    }
}

}  // namespace cms

using namespace cms;

extern "C" int cms_tta_resize(const void* src, void* dst, int n, int c, int H, int W, int Hs, int Ws, int dtype, int flip,
                              void* stream) {
    const char* why = tta_check_resize(src, dst, n, c, H, W, Hs, Ws, dtype);
    CMS_REQUIRE(!why, "tta_resize: %s", why);
    const size_t planes = (size_t)n * c;
    const int grid = grid_for(planes * Hs * Ws, 256, 4096);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CMS_F32) {
        hipLaunchKernelGGL(tta_resize_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)src, (float*)dst, planes, H, W, Hs, Ws,
                           flip != 0);
    } else {
        hipLaunchKernelGGL(tta_resize_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, (const uint16_t*)src, (uint16_t*)dst, planes, H, W,
                           Hs, Ws, flip != 0);
    }
    return launch_status("cms_tta_resize");
}

template <int MODE>
static int tta_launch(const cms_tta_desc* d, const TtaViews& v, hipStream_t s) {
    const size_t P = (size_t)d->n * d->H * d->W;
    const size_t lds = ((MODE == 2 ? (size_t)d->c * kTtaBlock : 0) + (size_t)d->c * d->c) * sizeof(float);
    auto kern = tta_vote_kernel<MODE>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid_for(P, kTtaBlock, 1024)), dim3(kTtaBlock), lds, s, v, d->k, d->labels, d->label_dtype,
                       d->ignore_index, d->n, d->c, d->H, d->W, d->align_corners, (unsigned long long*)d->cm, d->pred_out);
    return launch_status("cms_tta_vote");
}

extern "C" int cms_tta_vote(const cms_tta_desc* d, void* stream) {
    const char* why = tta_check_vote(d);
    CMS_REQUIRE(!why, "tta_vote: %s", why);
    TtaViews v;
    tta_make_views(d, &v);
    hipStream_t s = (hipStream_t)stream;
    if (d->k >= 2) return tta_launch<2>(d, v, s);
    if (d->h[0] == d->H && d->w[0] == d->W) return tta_launch<0>(d, v, s);
    return tta_launch<1>(d, v, s);
}
