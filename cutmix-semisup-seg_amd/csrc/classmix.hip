// ClassMix masks (gfx950): the mixing mask of a batch cut along the class regions the teacher predicts for image 1 (Olsson et al.,
// "ClassMix: Segmentation-Based Data Augmentation for Semi-Supervised Learning", WACV 2021). Written with tensor operations this is
// an upsample to (N, C, H, W), an argmax, a `unique` per sample (with a host synchronisation each) and an `isin`; here it is two
// stream-ordered launches that write five bytes per pixel and read one of them back:
//   pass 1  a workgroup owns a run of one sample's pixels (blockIdx.y = sample, blockIdx.x = slot): each thread gathers the
//           low-resolution logits (L2-resident) of its pixels, stores the uint8 prediction and ORs 1 << pred into a 64-bit word; the
//           wave ORs its lanes across lanes, the workgroup its waves through LDS, and one word goes to the sample's slot table
//   pass 2  every workgroup ORs its sample's slot words (at most 256), wave 0 ranks the present classes by their keys, lane c
//           deciding class c, and every thread turns four predictions into one 16-byte store of the mask
// No atomics and nothing to initialise: every slot word pass 2 reads was written by pass 1 of the same call. The arithmetic is
// csrc/classmix_math.hpp's, the prediction csrc/tta_math.hpp's single-view pixel, bit for bit cms_tta_vote's for k == 1.
#include "common.hpp"
#include "classmix_math.hpp"

namespace cms {

// OR over the 64 lanes of a wavefront; the result is valid in every lane
__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}

template <bool IDENT>
__global__ __launch_bounds__(kCmBlock) void classmix_pred_kernel(const TtaViews v, const float* __restrict__ valid, int C, int H, int W,
                                                                 int align, int chunk, uint8_t* __restrict__ pred,
                                                                 unsigned long long* __restrict__ slots) {
    __shared__ unsigned long long wave_bits[kCmBlock / kWave];
    const int n = blockIdx.y;
    const size_t hw = (size_t)H * W, base = (size_t)n * hw;
    const size_t lo = (size_t)blockIdx.x * chunk;
    const size_t hi = lo + chunk < hw ? lo + chunk : hw;
    unsigned long long bits = 0ull;
    for (size_t p = lo + threadIdx.x; p < hi; p += kCmBlock) {
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        const int best = tta_single_pixel<IDENT>(v, n, C, y, x, align != 0);
        pred[base + p] = (uint8_t)best;
        bits |= classmix_bit(best, valid ? valid[base + p] != 0.0f : true);
    }
    bits = wave_or(bits);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_bits[threadIdx.x / kWave] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0ull;
#pragma unroll
        for (int i = 0; i < kCmBlock / kWave; ++i) all |= wave_bits[i];
        slots[(size_t)n * kCmMaxSlots + blockIdx.x] = all;
    }
}

// VEC: mask, valid and pred are aligned for 16-, 16- and 4-byte accesses at flat indices that are multiples of four
template <bool VEC>
__global__ __launch_bounds__(kCmBlock) void classmix_mask_kernel(const uint8_t* __restrict__ pred, const float* __restrict__ valid,
                                                                 const double* __restrict__ keys,
                                                                 const unsigned long long* __restrict__ slots, int nslots, int C,
                                                                 size_t hw, float* __restrict__ mask,
                                                                 unsigned long long* __restrict__ present_out,
                                                                 unsigned long long* __restrict__ chosen_out) {
    __shared__ double s_keys[kTtaMaxClasses];
    __shared__ unsigned long long s_chosen;
    const int n = blockIdx.y;
    if ((int)threadIdx.x < C) s_keys[threadIdx.x] = keys[(size_t)n * C + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < kWave) {
        const int lane = threadIdx.x;
        unsigned long long mine = 0ull;
        for (int i = lane; i < nslots; i += kWave) mine |= slots[(size_t)n * kCmMaxSlots + i];
        const unsigned long long present = wave_or(mine);
        const bool in = classmix_is_chosen(present, [&](int c) { return s_keys[c]; }, C, lane);
        const unsigned long long chosen = __ballot(in);
        if (lane == 0) {
            s_chosen = chosen;
            if (blockIdx.x == 0) {
                if (present_out) present_out[n] = present;
                if (chosen_out) chosen_out[n] = chosen;
            }
        }
    }
    __syncthreads();
    const unsigned long long chosen = s_chosen;
    const size_t start = (size_t)n * hw, end = start + hw;
    auto one = [&](size_t i) { mask[i] = classmix_mask_value(chosen, pred[i], valid ? valid[i] != 0.0f : true); };
    if (VEC) {
        const CmSplit sp = classmix_split(start, end);
        const size_t g_hi = sp.vec_hi / 4;
        for (size_t g = sp.vec_lo / 4 + (size_t)blockIdx.x * kCmBlock + threadIdx.x; g < g_hi; g += (size_t)gridDim.x * kCmBlock) {
            const uint32_t p4 = reinterpret_cast<const uint32_t*>(pred)[g];
            float4 ok = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (valid) ok = reinterpret_cast<const float4*>(valid)[g];
            float4 m;
            m.x = classmix_mask_value(chosen, (int)(p4 & 255u), ok.x != 0.0f);
            m.y = classmix_mask_value(chosen, (int)((p4 >> 8) & 255u), ok.y != 0.0f);
            m.z = classmix_mask_value(chosen, (int)((p4 >> 16) & 255u), ok.z != 0.0f);
            m.w = classmix_mask_value(chosen, (int)(p4 >> 24), ok.w != 0.0f);
            reinterpret_cast<float4*>(mask)[g] = m;
        }
        if (blockIdx.x == 0) {      // at most three elements before the first group and three after the last
            const size_t head = sp.vec_lo - start, tail = end - sp.vec_hi;
            if (threadIdx.x < head) one(start + threadIdx.x);
            else if (threadIdx.x - head < tail) one(sp.vec_hi + (threadIdx.x - head));
        }
    } else {
        for (size_t i = start + (size_t)blockIdx.x * kCmBlock + threadIdx.x; i < end; i += (size_t)gridDim.x * kCmBlock) one(i);
    }
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_classmix_workspace_bytes(int n, int H, int W) { return classmix_workspace_bytes(n, H, W); }

extern "C" int cms_classmix(const cms_classmix_desc* d, void* stream) {
    const char* why = classmix_check(d);
    CMS_REQUIRE(!why, "classmix: %s", why);
    TtaViews v;
    classmix_views(d, &v);
    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)d->H * d->W;
    const int chunk = classmix_chunk((long long)hw), nslots = classmix_slots((long long)hw);
    unsigned long long* slots = (unsigned long long*)d->workspace;
    uint8_t* pred = d->pred_out ? d->pred_out : (uint8_t*)d->workspace + classmix_pred_offset(d->n);
    const dim3 grid(nslots, d->n), block(kCmBlock);
    if (d->h == d->H && d->w == d->W) {
        hipLaunchKernelGGL(classmix_pred_kernel<true>, grid, block, 0, s, v, d->valid, d->c, d->H, d->W, d->align_corners, chunk, pred,
                           slots);
    } else {
        hipLaunchKernelGGL(classmix_pred_kernel<false>, grid, block, 0, s, v, d->valid, d->c, d->H, d->W, d->align_corners, chunk, pred,
                           slots);
    }
    int rc = launch_status("cms_classmix (pass 1)");
    if (rc != CMS_OK) return rc;
    const bool vec = ((uintptr_t)d->mask_out & 15) == 0 && ((uintptr_t)d->valid & 15) == 0 && ((uintptr_t)pred & 3) == 0;
    unsigned long long* present = (unsigned long long*)d->present_out;
    unsigned long long* chosen = (unsigned long long*)d->chosen_out;
    if (vec) {
        hipLaunchKernelGGL(classmix_mask_kernel<true>, grid, block, 0, s, pred, d->valid, d->keys, slots, nslots, d->c, hw, d->mask_out,
                           present, chosen);
    } else {
        hipLaunchKernelGGL(classmix_mask_kernel<false>, grid, block, 0, s, pred, d->valid, d->keys, slots, nslots, d->c, hw, d->mask_out,
                           present, chosen);
    }
    return launch_status("cms_classmix (pass 2)");
}
