// Sliding-window evaluation kernels (gfx950): the crop that makes all windows of one view from the canvas image, and the fused
// stitch-and-vote over the windows' low-resolution logits. The reference evaluates whole images (train_seg_semisup_mask_mt.py:510-514);
// written with tensor operations, stitching upsamples every window's logits to (C, wh, ww), soft-maxes them and adds them into a
// (N, C, Hv, Wv) canvas per view beside a count map, then resizes and sums the views. Here a thread owns an output pixel, as in
// csrc/tta.hip: the window grid is regular, so the thread works out arithmetically which windows hold its pixel (at most five per
// axis) and gathers them -- no canvas, no count map, no atomics on floats. Per covering window it gathers the window's logits (L2-
// resident low-resolution maps) three times -- maximum, normaliser, probabilities -- and adds the probabilities, divided by the number
// of covering windows, into its column of an LDS score table [C][256]; only the uint8 prediction and the C x C histogram (LDS
// integer atomics, one 64-bit atomic per non-empty bin) leave the kernel. The arithmetic is csrc/window_math.hpp's.
#include "common.hpp"
#include "window_math.hpp"

namespace cms {

constexpr int kWinBlock = 256;

__global__ __launch_bounds__(kWinBlock) void window_vote_kernel(const WinViews v, int k, const void* labels, int label_dtype,
                                                               int ignore_index, int N, int C, int H, int W, int align,
                                                               unsigned long long* __restrict__ cm, uint8_t* __restrict__ pred_out) {
    extern __shared__ __attribute__((aligned(16))) float win_smem[];
    float* score = win_smem;                                                             // [C][kWinBlock]
    unsigned int* hist = reinterpret_cast<unsigned int*>(win_smem + C * kWinBlock);      // [C][C]
    const bool count = labels != nullptr && cm != nullptr;
    if (count) {
        for (int i = threadIdx.x; i < C * C; i += kWinBlock) hist[i] = 0;
    }
    __syncthreads();
    const size_t P = (size_t)N * H * W;
    for (size_t idx = (size_t)blockIdx.x * kWinBlock + threadIdx.x; idx < P; idx += (size_t)gridDim.x * kWinBlock) {
        const int x = (int)(idx % W);
        const size_t t = idx / W;
        const int y = (int)(t % H);
        const int n = (int)(t / H);
        const int best = win_vote_pixel(v, k, n, C, H, W, y, x, align != 0,
                                        [&](int c) -> float& { return score[c * kWinBlock + threadIdx.x]; });
        if (pred_out) pred_out[idx] = (uint8_t)best;
        if (count) {
            const int tr = tta_label(labels, label_dtype, idx);
            if (tr != ignore_index && tr >= 0 && tr < C) atomicAdd(&hist[tr * C + best], 1u);
        }
    }
    __syncthreads();
    if (count) {
        for (int i = threadIdx.x; i < C * C; i += kWinBlock) {
            const unsigned int val = hist[i];
            if (val) atomicAdd(&cm[i], (unsigned long long)val);
        }
    }
}

// one thread per element of dst (n * gy * gx, c, eh, ew); T = float or uint16_t (bf16 bits). COPY: the view is the canvas itself.
template <class T, bool COPY>
__global__ __launch_bounds__(256) void window_crop_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t total, int c, int H,
                                                          int W, int Hv, int Wv, int flip, int gy, int gx, int eh, int ew, int sh,
                                                          int sw) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const WinCropAt a = win_crop_at(idx, c, Hv, Wv, gy, gx, eh, ew, sh, sw);
        const T* plane = src + a.plane * ((size_t)H * W);
        if (COPY) {
            dst[idx] = plane[(size_t)a.vy * W + a.vx];
        } else {
            const float val = win_crop_pixel(
                [&](size_t i) {
                    if constexpr (sizeof(T) == 4) return plane[i];
                    else return bf16_to_f32(plane[i]);
                },
                H, W, Hv, Wv, flip, a.vy, a.vx);
            put_as<T>(dst, idx, val);
        }
    }
}

template <class T, bool COPY>
static void crop_launch(const void* src, void* dst, size_t total, int c, int H, int W, int Hv, int Wv, int flip, int gy, int gx, int eh,
                        int ew, int sh, int sw, hipStream_t s) {
    hipLaunchKernelGGL((window_crop_kernel<T, COPY>), dim3(grid_for(total, 256, 4096)), dim3(256), 0, s, (const T*)src, (T*)dst, total, c,
                       H, W, Hv, Wv, flip, gy, gx, eh, ew, sh, sw);
}

}  // namespace cms

using namespace cms;

extern "C" int cms_window_crop(const void* src, void* dst, int n, int c, int H, int W, int Hv, int Wv, int flip, int wh, int ww, int sh,
                               int sw, int dtype, void* stream) {
    const char* why = win_check_crop(src, dst, n, c, H, W, Hv, Wv, wh, ww, sh, sw, dtype);
    CMS_REQUIRE(!why, "window_crop: %s", why);
    const int gy = win_count(Hv, wh, sh), gx = win_count(Wv, ww, sw), eh = win_extent(Hv, wh), ew = win_extent(Wv, ww);
    const size_t total = (size_t)n * gy * gx * c * eh * ew;
    const bool copy = Hv == H && Wv == W && !flip;
    const int fl = flip != 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CMS_F32) {
        if (copy) crop_launch<float, true>(src, dst, total, c, H, W, Hv, Wv, fl, gy, gx, eh, ew, sh, sw, s);
        else crop_launch<float, false>(src, dst, total, c, H, W, Hv, Wv, fl, gy, gx, eh, ew, sh, sw, s);
    } else {
        if (copy) crop_launch<uint16_t, true>(src, dst, total, c, H, W, Hv, Wv, fl, gy, gx, eh, ew, sh, sw, s);
        else crop_launch<uint16_t, false>(src, dst, total, c, H, W, Hv, Wv, fl, gy, gx, eh, ew, sh, sw, s);
    }
    return launch_status("cms_window_crop");
}

extern "C" int cms_window_vote(const cms_window_desc* d, void* stream) {
    const char* why = win_check_vote(d);
    CMS_REQUIRE(!why, "window_vote: %s", why);
    if (win_all_single(d)) {
        // no view has more than one window: the vote over whole views, its single-view argmax of the logits included
        cms_tta_desc t;
        win_tta_desc(d, &t);
        return cms_tta_vote(&t, stream);
    }
    WinViews v;
    win_make_views(d, &v);
    const size_t P = (size_t)d->n * d->H * d->W;
    const size_t lds = ((size_t)d->c * kWinBlock + (size_t)d->c * d->c) * sizeof(float);
    auto kern = window_vote_kernel;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid_for(P, kWinBlock, 1024)), dim3(kWinBlock), lds, (hipStream_t)stream, v, d->k, d->labels,
                       d->label_dtype, d->ignore_index, d->n, d->c, d->H, d->W, d->align_corners, (unsigned long long*)d->cm,
                       d->pred_out);
    return launch_status("cms_window_vote");
}
