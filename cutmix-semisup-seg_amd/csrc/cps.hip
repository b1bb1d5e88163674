// Cross pseudo supervision labels (gfx950): the hard pseudo-labels that two networks give each other on a CutMix-ed pair (Chen, Yuan,
// Zeng, Wang, "Semi-Supervised Semantic Segmentation with Cross Pseudo Supervision", CVPR 2021). Written with tensor operations this
// is four upsamples to (N, C, H, W), two selects by the mask, two softmax / max passes and two compares; here it is ONE launch that
// reads the four low-resolution logit tensors (L2-resident), the mask or box table and the validity maps, and writes two uint8 label
// maps and four exact counts:
//   a thread owns four consecutive labels of one sample (blockIdx.y = sample) whose flat index is a multiple of four: the mask bit,
//   the validity and the bilinear taps of a pixel are worked out once and serve both networks; both maps get one 4-byte store per
//   thread, the at most three labels in front of a sample's first group and behind its last are workgroup 0's, byte by byte;
//   the counts are summed across the lanes of a wave, across the waves through LDS, and one 64-bit integer atomic per workgroup and
//   non-zero count goes to `stats`, which a 32-byte memset in front of the launch has cleared (integers: the order does not matter)
// The logits are not staged in LDS: a sample's four tensors are at most 4 x 19 x 65 x 129 floats. The arithmetic is
// csrc/cps_math.hpp's.
#include "common.hpp"
#include "cps_math.hpp"

namespace cms {

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <int CT, bool IDENT, bool VEC>
__global__ __launch_bounds__(kCpsBlock) void cps_labels_kernel(const CpsArgs a) {
    __shared__ int wave_counts[kCpsBlock / kWave][4];
    CpsCounts k = {0, 0, 0, 0};
    cps_thread<CT, IDENT, VEC>(a, (int)blockIdx.y, blockIdx.x, (int)threadIdx.x, k);
    int v[4] = {k.n_valid, k.kept_a, k.kept_b, k.agree};
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = wave_sum_int(v[i]);
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wave_counts[threadIdx.x / kWave][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        int sum = 0;
#pragma unroll
        for (int wv = 0; wv < kCpsBlock / kWave; ++wv) sum += wave_counts[wv][threadIdx.x];
        if (sum != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.d.stats) + threadIdx.x, (unsigned long long)sum);
    }
}

template <int CT>
static void cps_launch(const CpsArgs& a, bool ident, bool vec, dim3 grid, hipStream_t s) {
    const dim3 block(kCpsBlock);
    if (ident) {
        if (vec) hipLaunchKernelGGL((cps_labels_kernel<CT, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cps_labels_kernel<CT, true, false>), grid, block, 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((cps_labels_kernel<CT, false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cps_labels_kernel<CT, false, false>), grid, block, 0, s, a);
    }
}

}  // namespace cms

using namespace cms;

extern "C" int cms_cps_labels(const cms_cps_desc* d, void* stream) {
    const char* why = cps_check(d);
    CMS_REQUIRE(!why, "cps_labels: %s", why);
    CpsArgs a;
    cps_make_args(d, &a);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d->stats, 0, 4 * sizeof(int64_t), s) != hipSuccess) return launch_status("cms_cps_labels (memset)");
    const bool ident = d->h == d->H && d->w == d->W;
    const bool vec = (((uintptr_t)d->label_a | (uintptr_t)d->label_b) & 3) == 0;
    const dim3 grid(cps_blocks((long long)d->H * d->W), d->n);
    switch (cps_ct(d->c)) {
        case 19: cps_launch<19>(a, ident, vec, grid, s); break;
        case 21: cps_launch<21>(a, ident, vec, grid, s); break;
        default: cps_launch<0>(a, ident, vec, grid, s); break;
    }
    return launch_status("cms_cps_labels");
}
