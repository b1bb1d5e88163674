// ICT (interpolation consistency training) input blend (gfx950): out = x0 * (1 - lam[n]) + x1 * lam[n] per sample,
// train_seg_semisup_ict.py:310-311 -- the student's image and the loss's validity mask. HBM-bound: two tensors read, one
// written, 16 bytes per lane per access. The interpolation LOSS kernels live at the end of losses.hip, next to the tile
// helpers they share with the CutMix consistency; the per-pixel arithmetic of both is csrc/ict_math.hpp.
#include <algorithm>
#include "common.hpp"
#include "ict_math.hpp"

namespace cms {

template <typename T>
struct BlendElem;
template <>
struct BlendElem<float> {
    static __device__ __forceinline__ float load(float v) { return v; }
    static __device__ __forceinline__ float store(float v) { return v; }
};
template <>
struct BlendElem<uint16_t> {      // bf16: fp32 arithmetic, ONE rounding of the sum
    static __device__ __forceinline__ float load(uint16_t v) { return bf16_to_f32(v); }
    static __device__ __forceinline__ uint16_t store(float v) { return f32_to_bf16(v); }
};

// The tensors are walked FLAT in vectors of VEC elements (VEC * sizeof(T) = 16 bytes), so the accesses stay aligned when
// `chw` is no multiple of VEC; a vector that straddles a sample boundary switches its factor on the way. The last
// total % VEC elements are the scalar tail. IDX32: the element count fits 32 bits (one 32-bit division per vector).
template <typename T, int VEC, bool IDX32>
__global__ __launch_bounds__(256) void ict_blend_kernel(const T* __restrict__ x0, const T* __restrict__ x1, T* __restrict__ out,
                                                        const float* __restrict__ lam, size_t total, size_t chw) {
    struct alignas(VEC * sizeof(T)) Vec {
        T v[VEC];
    };
    const size_t nvec = total / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e0 = i * VEC;
        size_t s, rem;
        if (IDX32) {
            const uint32_t q = (uint32_t)e0 / (uint32_t)chw;
            s = q;
            rem = (uint32_t)e0 - q * (uint32_t)chw;
        } else {
            s = e0 / chw;
            rem = e0 - s * chw;
        }
        const Vec a = reinterpret_cast<const Vec*>(x0)[i], b = reinterpret_cast<const Vec*>(x1)[i];
        Vec o;
        float l = lam[s];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            o.v[j] = BlendElem<T>::store(ict_mix(BlendElem<T>::load(a.v[j]), BlendElem<T>::load(b.v[j]), 1.0f - l, l));
            if (++rem == chw && j + 1 < VEC && e0 + j + 1 < total) {
                rem = 0;
                l = lam[++s];
            }
        }
        reinterpret_cast<Vec*>(out)[i] = o;
    }
    const size_t tail = nvec * VEC + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tail < total) {
        const float l = lam[tail / chw];
        out[tail] = BlendElem<T>::store(ict_mix(BlendElem<T>::load(x0[tail]), BlendElem<T>::load(x1[tail]), 1.0f - l, l));
    }
}

template <typename T, int VEC>
static void blend_launch(const void* x0, const void* x1, void* out, const float* lam, size_t total, size_t chw, hipStream_t s) {
    const int grid = grid_for(total / VEC + 1, 256, 256 * 16);
    if (total < ((size_t)1 << 32))
        hipLaunchKernelGGL((ict_blend_kernel<T, VEC, true>), dim3(grid), dim3(256), 0, s, (const T*)x0, (const T*)x1, (T*)out, lam,
                           total, chw);
    else
        hipLaunchKernelGGL((ict_blend_kernel<T, VEC, false>), dim3(grid), dim3(256), 0, s, (const T*)x0, (const T*)x1, (T*)out, lam,
                           total, chw);
}

}  // namespace cms

using namespace cms;

extern "C" int cms_ict_blend(const void* x0, const void* x1, void* out, int dtype, const float* lam, int n, long long chw,
                             void* stream) {
    CMS_REQUIRE(x0 && x1 && out && lam, "ict_blend: NULL argument");
    CMS_REQUIRE(dtype == CMS_F32 || dtype == CMS_BF16, "ict_blend: unknown dtype %d", dtype);
    CMS_REQUIRE(n > 0 && chw > 0, "ict_blend: bad geometry");
    const size_t total = (size_t)n * (size_t)chw;
    const bool aligned = (((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)out) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CMS_F32) {
        if (aligned) blend_launch<float, 4>(x0, x1, out, lam, total, (size_t)chw, s);
        else blend_launch<float, 1>(x0, x1, out, lam, total, (size_t)chw, s);
    } else {
        if (aligned) blend_launch<uint16_t, 8>(x0, x1, out, lam, total, (size_t)chw, s);
        else blend_launch<uint16_t, 1>(x0, x1, out, lam, total, (size_t)chw, s);
    }
    return launch_status("cms_ict_blend");
}
