// Downsampling of the Cityscapes converter (gfx950): convert_cityscapes.py:17-24, 44-46 of the reference on the device.
//   cms_downsample_image_u8    (n, h, w, 3) uint8 -> (n, h / d, w / d, 3): floor of the mean of each d x d block, per channel
//   cms_downsample_labels_u8   (n, h, w)    uint8 -> (n, h / d, w / d):    the most frequent value of each d x d block, the lowest
//                                                                          value among equally frequent ones
// The arithmetic is convert_math.hpp's (integers only; no atomics, no LDS, plain vector stores: every output byte is written once,
// by one thread, from the same inputs on every run). One thread per group of kCvtGroup consecutive output pixels of one output
// row, groups in row-major order over a grid-stride loop: the lanes of a wave read one contiguous stretch from each of the d
// source rows under their groups -- as 32-bit words wherever the row pitch and the base keep every piece 4-byte aligned -- and
// write one contiguous stretch of the output row. The last group of a row may be short; it is loaded and stored byte by byte,
// bounded by the row end.
#include "common.hpp"
#include "convert_math.hpp"

namespace cms {

// C = 3: images, C = 1: labels
template <int D, int C>
__global__ __launch_bounds__(256) void downsample_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int ho,
                                                     int wo, int in_words, int out_words) {
    const size_t total = cvt_work_items(n, ho, wo);
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x)
        cvt_work_item<D, C>(src, dst, idx, wo, in_words != 0, out_words != 0);
}

template <int C>
static int downsample_launch(const char* what, const uint8_t* src, int n, int h, int w, int d, uint8_t* dst, void* stream) {
    CMS_REQUIRE(src && dst, "%s: NULL pointer", what);
    CMS_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad geometry n=%d h=%d w=%d", what, n, h, w);
    CMS_REQUIRE(d >= 1 && d <= kCvtMaxD, "%s: d=%d, 1..%d are built", what, d, kCvtMaxD);
    CMS_REQUIRE(h % d == 0 && w % d == 0, "%s: %dx%d is not divisible by d=%d", what, h, w, d);
    // n * h * w * C <= 2^31 - 1, tested factor by factor so that no product overflows (the output is the smaller tensor)
    CMS_REQUIRE(n <= 0x7fffffff / h && n * h <= 0x7fffffff / w && n * h * w <= 0x7fffffff / C,
                "%s: more than 2^31 - 1 bytes per tensor", what);
    const int ho = h / d, wo = w / d;
    // every piece starts at base + row * pitch + 4 * (group * d * C): word loads need the base and the pitch on 4 bytes
    const int in_words = cvt_words_ok(src, (size_t)w * C), out_words = cvt_words_ok(dst, (size_t)wo * C);
    const dim3 grid(grid_for(cvt_work_items(n, ho, wo), 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (d) {
#define CMS_CVT_CASE(D) \
    case D: hipLaunchKernelGGL((downsample_u8<D, C>), grid, block, 0, s, src, dst, n, ho, wo, in_words, out_words); break;
        CMS_CVT_CASE(1) CMS_CVT_CASE(2) CMS_CVT_CASE(3) CMS_CVT_CASE(4) CMS_CVT_CASE(5) CMS_CVT_CASE(6) CMS_CVT_CASE(7) CMS_CVT_CASE(8)
#undef CMS_CVT_CASE
    }
    return launch_status(what);
}

}  // namespace cms

using namespace cms;

extern "C" int cms_downsample_image_u8(const uint8_t* src, int n, int h, int w, int d, uint8_t* dst, void* stream) {
    return downsample_launch<3>("cms_downsample_image_u8", src, n, h, w, d, dst, stream);
}

extern "C" int cms_downsample_labels_u8(const uint8_t* src, int n, int h, int w, int d, uint8_t* dst, void* stream) {
    return downsample_launch<1>("cms_downsample_labels_u8", src, n, h, w, d, dst, stream);
}
