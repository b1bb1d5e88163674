// Batched 2-D complex fp64 FFT, power-of-two lengths 8 ... 4096 per axis (gfx950). The transform under the patch-distance
// analysis (csrc/patchdist.hip): patch_dist.py:107-154 computes its cross-correlations with scipy.signal.fftconvolve; here they
// are fp64 transforms whose results round back to exact integers.
//
//   rows     a workgroup holds whole rows in LDS (one row of 4096 complex128 = 64 KiB; shorter rows share a workgroup), loads them
//            in bit-reversed order and runs log2(n) radix-2 decimation-in-time stages, a barrier after each
//   columns  a workgroup holds a tile of `tc` ADJACENT columns (tc * fh <= 8192 complex128 = 128 KiB of the CU's 160 KiB), so a
//            global access touches tc * 16 contiguous bytes per row; in LDS each column is contiguous and the same stages run
//   twiddles exp(-2 pi i k / n), k < n / 2, from a table the host builds in float64; the inverse conjugates them and scales each
//            axis by 1 / n (a power of two: exact)
// One code path serves every length: radix 2 throughout, so 2^odd and 2^even lengths do not differ.
#include "common.hpp"

namespace cms {

constexpr int kFftThreads = 256;
constexpr int kFftMaxLen = 4096;
constexpr int kFftRowElems = 1024;     // rows shorter than this share a workgroup up to this many elements
constexpr int kFftColElems = 8192;     // column tile: tc * fh elements at most
constexpr int kFftMaxTileCols = 16;

// `count` transforms of length n = 2^log2n, each contiguous in `s`, inputs already in bit-reversed order
__device__ __forceinline__ void fft_stages(double2* s, int n, int log2n, int count, const double2* __restrict__ tw, bool inverse) {
    const int butterflies = count * (n >> 1);
    for (int st = 0; st < log2n; ++st) {
        const int half = 1 << st;
        const int tw_step = n >> (st + 1);
        for (int i = threadIdx.x; i < butterflies; i += blockDim.x) {
            const int t = i >> (log2n - 1);             // which transform
            const int b = i & ((n >> 1) - 1);           // which butterfly of it
            const int j = b & (half - 1);
            const int lo = t * n + ((b >> st) << (st + 1)) + j;
            const int hi = lo + half;
            double2 w = tw[j * tw_step];
            if (inverse) w.y = -w.y;
            const double2 a = s[lo], c = s[hi];
            const double wr = c.x * w.x - c.y * w.y, wi = c.x * w.y + c.y * w.x;
            s[lo] = make_double2(a.x + wr, a.y + wi);
            s[hi] = make_double2(a.x - wr, a.y - wi);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int bit_reverse(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

__global__ __launch_bounds__(kFftThreads) void fft_rows(double2* __restrict__ data, long long total_rows, int n, int log2n,
                                                        int rows_per_wg, const double2* __restrict__ tw, int inverse, double scale) {
    extern __shared__ __attribute__((aligned(16))) char fft_smem[];
    double2* s = reinterpret_cast<double2*>(fft_smem);
    const long long row0 = (long long)blockIdx.x * rows_per_wg;
    const int elems = rows_per_wg * n;
    for (int i = threadIdx.x; i < elems; i += blockDim.x) {
        const int r = i >> log2n, c = i & (n - 1);
        double2 v = make_double2(0.0, 0.0);
        if (row0 + r < total_rows) v = data[(size_t)(row0 + r) * n + c];
        s[r * n + bit_reverse(c, log2n)] = v;
    }
    __syncthreads();
    fft_stages(s, n, log2n, rows_per_wg, tw, inverse != 0);
    for (int i = threadIdx.x; i < elems; i += blockDim.x) {
        const int r = i >> log2n;
        if (row0 + r < total_rows) {
            const double2 v = s[i];
            data[(size_t)(row0 + r) * n + (i & (n - 1))] = make_double2(v.x * scale, v.y * scale);
        }
    }
}

// grid (fw / tc, batch)
__global__ __launch_bounds__(kFftThreads) void fft_cols(double2* __restrict__ data, int fh, int log2h, int fw, int tc, int log2tc,
                                                        const double2* __restrict__ tw, int inverse, double scale) {
    extern __shared__ __attribute__((aligned(16))) char fft_smem[];
    double2* s = reinterpret_cast<double2*>(fft_smem);
    double2* plane = data + (size_t)blockIdx.y * fh * fw + (size_t)blockIdx.x * tc;
    const int elems = fh * tc;
    for (int i = threadIdx.x; i < elems; i += blockDim.x) {
        const int r = i >> log2tc, c = i & (tc - 1);
        s[c * fh + bit_reverse(r, log2h)] = plane[(size_t)r * fw + c];
    }
    __syncthreads();
    fft_stages(s, fh, log2h, tc, tw, inverse != 0);
    for (int i = threadIdx.x; i < elems; i += blockDim.x) {
        const int r = i >> log2tc, c = i & (tc - 1);
        const double2 v = s[c * fh + r];
        plane[(size_t)r * fw + c] = make_double2(v.x * scale, v.y * scale);
    }
}

// log2 of a supported length, or -1
static int fft_log2(int n) {
    if (n < 8 || n > kFftMaxLen || (n & (n - 1))) return -1;
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

}  // namespace cms

using namespace cms;

extern "C" int cms_fft2(void* data, int batch, int fh, int fw, int inverse, const void* tw_h, const void* tw_w, void* stream) {
    CMS_REQUIRE(data && tw_h && tw_w, "fft2: NULL pointer");
    const int lh = fft_log2(fh), lw = fft_log2(fw);
    CMS_REQUIRE(lh > 0 && lw > 0, "fft2: lengths must be powers of two in 8 ... %d (got %d x %d)", kFftMaxLen, fh, fw);
    CMS_REQUIRE(batch > 0 && batch <= 65535, "fft2: batch must be in 1 ... 65535 (got %d)", batch);
    hipStream_t s = (hipStream_t)stream;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fft_rows), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kFftMaxLen * (int)sizeof(double2));
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fft_cols), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kFftColElems * (int)sizeof(double2));
        attr_set = true;
    }
    // rows
    const int rows_per_wg = fw >= kFftRowElems ? 1 : kFftRowElems / fw;
    const long long total_rows = (long long)batch * fh;
    const unsigned row_blocks = (unsigned)((total_rows + rows_per_wg - 1) / rows_per_wg);
    hipLaunchKernelGGL(fft_rows, dim3(row_blocks), dim3(kFftThreads), (size_t)rows_per_wg * fw * sizeof(double2), s, (double2*)data,
                       total_rows, fw, lw, rows_per_wg, (const double2*)tw_w, inverse, inverse ? 1.0 / fw : 1.0);
    // columns, in tiles of tc adjacent ones (tc a power of two that divides fw)
    int tc = kFftColElems / fh, log2tc = 0;
    if (tc > kFftMaxTileCols) tc = kFftMaxTileCols;
    if (tc > fw) tc = fw;
    while ((1 << log2tc) < tc) ++log2tc;
    hipLaunchKernelGGL(fft_cols, dim3((unsigned)(fw / tc), (unsigned)batch), dim3(kFftThreads), (size_t)tc * fh * sizeof(double2), s,
                       (double2*)data, fh, lh, fw, tc, log2tc, (const double2*)tw_h, inverse, inverse ? 1.0 / fh : 1.0);
    return launch_status("cms_fft2");
}
