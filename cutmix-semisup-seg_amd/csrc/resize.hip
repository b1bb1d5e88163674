// Area resize and image statistics of the ISIC 2017 converter (gfx950): convert_isic.py:56-60, 67-73 of the reference on the device.
//   cms_resize_area_u8   (n, h, w, c) uint8 -> (n, ho, wo, c), c = 1 or 3, ho <= h, wo <= w: the exact area filter of
//                        resize_math.hpp, num / (h * w) rounded to nearest, ties to even
//   cms_sum_sumsq_u8     (n, pixels, c) uint8 -> (n, 2c) int64: sum p per channel, then sum p^2
// The arithmetic is resize_math.hpp's (integers only; no atomics; plain vector stores: every output byte is written once, by one
// thread, from the same inputs on every run).
//
// Resize: one workgroup of 256 threads per output row and segment of output columns, work items in row-major order over a
// grid-stride loop. Per chunk of 4096 source bytes of the row, every thread sums wy * p down the <= ceil(h / ho) + 1 source rows
// for its sixteen byte columns in registers -- four 32-bit words, 256 words apart, where the base and the pitch are on four bytes,
// single bytes 256 apart otherwise, so a wave's load is one contiguous stretch either way -- and hands the sums over through
// 16 KiB of LDS; one thread per output (ox, ch) then adds wx * column sum over its <= ceil(w / wo) + 1 columns in 64 bits, and
// after the last chunk divides, rounds and stores its byte. The source bytes under an output row are read from HBM once, plus the
// one source row that two neighbouring output rows may share and the one pixel column two neighbouring segments may share.
//
// Statistics: one workgroup per image, 64-bit partial sums per thread, added in a fixed tree through LDS.
#include "common.hpp"
#include "resize_math.hpp"

namespace cms {

template <bool WORDS>
__global__ __launch_bounds__(kRszThreads) void resize_area_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n,
                                                              RszGeom g) {
    __shared__ uint32_t sums[kRszChunk];
    const int t = threadIdx.x;
    const size_t pitch = (size_t)g.w * g.c, total = rsz_work_items(n, g);
    for (size_t item = blockIdx.x; item < total; item += gridDim.x) {
        const RszItem it = rsz_item(item, g);
        const uint8_t* img = src + it.src_row0 * pitch;
        const bool owner = t < it.nox * g.c;
        const int ox = it.ox0 + t / g.c, ch = t % g.c;
        uint64_t num = 0;
        for (int cb = it.a0; cb < it.b1; cb += kRszChunk) {
            uint32_t acc[kRszPerThread];
            rsz_column_sums<WORDS>(img, pitch, g, it, cb, t, acc);
            rsz_store_sums<WORDS>(acc, t, sums);
            __syncthreads();
            if (owner) num += rsz_add_chunk(sums, g, cb, ox, ch);
            __syncthreads();                                   // the next chunk, or the next item, overwrites the sums
        }
        if (owner) dst[(it.out_row * g.wo + ox) * g.c + ch] = (uint8_t)rsz_round_div(num, (uint64_t)g.h * g.w);
    }
}

__global__ __launch_bounds__(kRszThreads) void sum_sumsq_u8(const uint8_t* __restrict__ src, int pixels, int c,
                                                            int64_t* __restrict__ out) {
    __shared__ uint64_t part[6][kRszThreads];
    const int t = threadIdx.x;
    uint64_t acc[6] = {};
    rsz_sum_sumsq_thread(src + (size_t)blockIdx.x * pixels * c, pixels, c, t, kRszThreads, acc);
#pragma unroll
    for (int k = 0; k < 6; ++k) part[k][t] = acc[k];
    __syncthreads();
    for (int half = kRszThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int k = 0; k < 6; ++k) part[k][t] += part[k][t + half];
        }
        __syncthreads();
    }
    if (t < 2 * c) out[(size_t)blockIdx.x * 2 * c + t] = (int64_t)part[t][0];
}

}  // namespace cms

using namespace cms;

extern "C" int cms_resize_area_u8(const uint8_t* src, int n, int h, int w, int c, int ho, int wo, uint8_t* dst, void* stream) {
    const char* what = "cms_resize_area_u8";
    CMS_REQUIRE(src && dst, "%s: NULL pointer", what);
    CMS_REQUIRE(c == 1 || c == 3, "%s: c=%d, 1 and 3 are built", what, c);
    CMS_REQUIRE(n >= 1 && h >= 1 && w >= 1 && ho >= 1 && wo >= 1, "%s: bad geometry n=%d h=%d w=%d ho=%d wo=%d", what, n, h, w, ho, wo);
    CMS_REQUIRE(h <= kRszMaxSide && w <= kRszMaxSide, "%s: %dx%d, a side may be %d at the most", what, h, w, kRszMaxSide);
    CMS_REQUIRE(ho <= h && wo <= w, "%s: %dx%d -> %dx%d would enlarge; the area filter only shrinks", what, h, w, ho, wo);
    // n * h * w * c <= 2^31 - 1, tested factor by factor so that no product overflows (the output is the smaller tensor)
    CMS_REQUIRE(n <= 0x7fffffff / h && n * h <= 0x7fffffff / w && n * h * w <= 0x7fffffff / c,
                "%s: more than 2^31 - 1 bytes per tensor", what);
    RszGeom g;
    g.h = h, g.w = w, g.c = c, g.ho = ho, g.wo = wo;
    g.seg = rsz_plan_segment((long long)n * ho, w, c, wo);
    g.nseg = (wo + g.seg - 1) / g.seg;
    g.words = (uintptr_t)src % 4 == 0 && ((size_t)w * c) % 4 == 0;
    const size_t total = rsz_work_items(n, g);
    const dim3 grid((unsigned)(total < (1u << 20) ? total : (1u << 20))), block(kRszThreads);
    hipStream_t s = (hipStream_t)stream;
    if (g.words) hipLaunchKernelGGL(resize_area_u8<true>, grid, block, 0, s, src, dst, n, g);
    else hipLaunchKernelGGL(resize_area_u8<false>, grid, block, 0, s, src, dst, n, g);
    return launch_status(what);
}

extern "C" int cms_sum_sumsq_u8(const uint8_t* src, int n, int pixels, int c, int64_t* sums, void* stream) {
    const char* what = "cms_sum_sumsq_u8";
    CMS_REQUIRE(src && sums, "%s: NULL pointer", what);
    CMS_REQUIRE(c == 1 || c == 3, "%s: c=%d, 1 and 3 are built", what, c);
    CMS_REQUIRE(n >= 1 && pixels >= 1, "%s: bad geometry n=%d pixels=%d", what, n, pixels);
    CMS_REQUIRE(n <= 0x7fffffff / pixels && n * pixels <= 0x7fffffff / c, "%s: more than 2^31 - 1 bytes in the tensor", what);
    hipLaunchKernelGGL(sum_sumsq_u8, dim3(n), dim3(kRszThreads), 0, (hipStream_t)stream, src, pixels, c, sums);
    return launch_status(what);
}
