// CowMask generator (gfx950): Gaussian-smoothed noise thresholded at a chosen share of ones, all in fp64 from the f32 noise onward
// so that the mask equals an fp64 host restatement pixel for pixel (the threshold is a discontinuity). The arithmetic and the
// indexing are cowmask_math.hpp's. Three launches per batch, no atomics, every sum in a fixed order:
//   1  cow_blur<float, false>   noise (N,H,W) f32 -> blur along x -> (N,W,H) f64                                [workspace plane 0]
//   2  cow_blur<double, true>   (N,W,H) f64 -> blur along y -> s (N,H,W) f64 and, per tile, { sum, sum of squared distances to
//                               the tile's own mean }                                                          [plane 1, slots]
//   3  cow_threshold_kernel     every workgroup adds the slots of its sample in the same order (mean, then Chan's combination of
//                               the squared distances), forms tau = mean + std * f and writes mask = (s <= tau)
#include "common.hpp"
#include "cowmask_math.hpp"

namespace cms {

// fixed-order sum over the workgroup: a[tid] holds one value per thread; the result is a[0], read by everyone after the call
__device__ __forceinline__ double cow_block_sum(double* a, double v) {
    const int tid = threadIdx.x;
    __syncthreads();                       // a[] may still be read from an earlier call
    a[tid] = v;
    __syncthreads();
    for (int s = kCowThreads / 2; s > 0; s >>= 1) {
        if (tid < s) a[tid] += a[tid + s];
        __syncthreads();
    }
    return a[0];
}

// in: (n, rows, cols), convolved along cols with the sample's taps; out: (n, cols, rows)
template <class T, bool STATS>
__global__ __launch_bounds__(kCowThreads) void cow_blur(const T* __restrict__ in, const double* __restrict__ taps, double* __restrict__ out,
                                                        double* __restrict__ partials, int rows, int cols, int radius) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cow_smem[];
    __shared__ double red[kCowThreads];
    double* taps_s = reinterpret_cast<double*>(cow_smem);
    const int kp = cow_taps_padded(radius), ntaps = 2 * radius + 1;
    T* tile = reinterpret_cast<T*>(taps_s + kp);
    const int tid = threadIdx.x, sample = blockIdx.z;
    const int r0 = blockIdx.y * kCowTileR, c0 = blockIdx.x * kCowTileC;
    const T* plane = in + (size_t)sample * rows * cols;

    int k_lo, k_hi;
    cow_tile_tap_range(c0, cols, radius, &k_lo, &k_hi);
    for (int k = tid; k < kp; k += kCowThreads) taps_s[k] = k < ntaps ? taps[(size_t)sample * ntaps + k] : 0.0;
    // local columns k_lo .. k_hi + kCowTileC - 1 are read below; consecutive lanes take consecutive columns of one row
    const int l_end = k_hi + kCowTileC;
    for (int rl = tid / 64; rl < kCowTileR; rl += kCowThreads / 64)
        for (int l = k_lo + (tid % 64); l < l_end; l += 64)
            tile[(size_t)l * kCowPitch + rl] = (T)cow_fetch(plane, rows, cols, r0 + rl, c0 - radius + l);
    __syncthreads();

    const int row = cow_thread_row(tid), cl = cow_thread_col(tid);
    double acc[kCowPerThread];
    cow_blur_thread(tile, taps_s, row, cl, k_lo, k_hi, acc);

    double* oplane = out + (size_t)sample * rows * cols;
    const bool row_ok = r0 + row < rows;
#pragma unroll
    for (int j = 0; j < kCowPerThread; ++j)
        if (row_ok && c0 + cl + j < cols) oplane[(size_t)(c0 + cl + j) * rows + (r0 + row)] = acc[j];

    if constexpr (STATS) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < kCowPerThread; ++j)
            if (row_ok && c0 + cl + j < cols) sum += acc[j];
        const double tile_sum = cow_block_sum(red, sum);
        const double tile_mean = tile_sum / (double)cow_tile_count(blockIdx.y, blockIdx.x, rows, cols);
        double m2 = 0.0;
#pragma unroll
        for (int j = 0; j < kCowPerThread; ++j)
            if (row_ok && c0 + cl + j < cols) {
                const double d = acc[j] - tile_mean;
                m2 = fma(d, d, m2);
            }
        const double tile_m2 = cow_block_sum(red, m2);
        if (tid == 0) {
            double* slot = partials + cow_partial_slot(sample, blockIdx.y, blockIdx.x, rows, cols);
            slot[0] = tile_sum;
            slot[1] = tile_m2;
        }
    }
}

// s: (n, h, w) f64; the slots were written over the (rows = w, cols = h) plane of the second pass
__global__ __launch_bounds__(kCowThreads) void cow_threshold_kernel(const double* __restrict__ s, const double* __restrict__ partials,
                                                                    const double* __restrict__ factor, float* __restrict__ mask,
                                                                    double* __restrict__ stats, int h, int w) {
    __shared__ double red[kCowThreads];
    const int tid = threadIdx.x, sample = blockIdx.y;
    const int rows = w, cols = h, tiles_c = cow_div_up(cols, kCowTileC), tiles = cow_tiles(rows, cols);
    const size_t pixels = (size_t)h * w;
    const double* slots = partials + cow_partial_slot(sample, 0, 0, rows, cols);
    double v = 0.0;
    for (int t = tid; t < tiles; t += kCowThreads) v += slots[2 * t];
    const double mean = cow_block_sum(red, v) / (double)pixels;
    v = 0.0;
    for (int t = tid; t < tiles; t += kCowThreads)
        v += cow_m2_term(slots[2 * t], slots[2 * t + 1], cow_tile_count(t / tiles_c, t % tiles_c, rows, cols), mean);
    const double m2 = cow_block_sum(red, v);
    double sd;
    const double tau = cow_threshold(mean, m2, pixels, factor[sample], &sd);
    if (stats && blockIdx.x == 0 && tid == 0) {
        stats[2 * sample] = mean;
        stats[2 * sample + 1] = sd;
    }
    const double* sp = s + (size_t)sample * pixels;
    float* mp = mask + (size_t)sample * pixels;
    for (size_t i = (size_t)blockIdx.x * kCowThreads + tid; i < pixels; i += (size_t)gridDim.x * kCowThreads)
        mp[i] = cow_mask_bit(sp[i], tau);
}

template <class T, bool STATS>
static void cow_blur_launch(const T* in, const double* taps, double* out, double* partials, int n, int rows, int cols, int radius,
                            hipStream_t s) {
    const size_t lds = cow_lds_bytes(radius, sizeof(T));
    // the largest radius needs 90 KB; the limit is raised once per kernel (to what every radius fits in), not per launch
    static const bool raised =
        hipFuncSetAttribute(reinterpret_cast<const void*>(cow_blur<T, STATS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)cow_lds_bytes(kCowMaxRadius, sizeof(T))) == hipSuccess;
    (void)raised;
    const dim3 grid(cow_div_up(cols, kCowTileC), cow_div_up(rows, kCowTileR), n), block(kCowThreads);
    hipLaunchKernelGGL((cow_blur<T, STATS>), grid, block, lds, s, in, taps, out, partials, rows, cols, radius);
}

}  // namespace cms

using namespace cms;

// every size the entry point accepts: n * h * w <= 2^31 - 1 (tested factor by factor), at most 65535 samples and tile rows
static bool cow_geometry_ok(int n, int h, int w) {
    return n >= 1 && h >= 1 && w >= 1 && n <= 65535 && n <= 0x7fffffff / h && n * h <= 0x7fffffff / w &&
           cow_div_up(h, kCowTileR) <= 65535 && cow_div_up(w, kCowTileR) <= 65535;
}

extern "C" size_t cms_cowmask_workspace_bytes(int n, int h, int w) { return cow_geometry_ok(n, h, w) ? cow_workspace_bytes(n, h, w) : 0; }

extern "C" int cms_cowmask(const float* noise, const double* taps, const double* thresh_factor, int n, int h, int w, int radius,
                           float* mask_out, double* stats_out, void* workspace, size_t workspace_bytes, void* stream) {
    CMS_REQUIRE(noise && taps && thresh_factor && mask_out && workspace, "cms_cowmask: NULL pointer");
    CMS_REQUIRE(n >= 1 && h >= 1 && w >= 1, "cms_cowmask: bad geometry n=%d h=%d w=%d", n, h, w);
    CMS_REQUIRE(radius >= 0 && radius <= kCowMaxRadius, "cms_cowmask: radius=%d, 0..%d are built", radius, kCowMaxRadius);
    CMS_REQUIRE(cow_geometry_ok(n, h, w), "cms_cowmask: n=%d h=%d w=%d is more than 2^31 - 1 pixels or 65535 samples", n, h, w);
    CMS_REQUIRE(workspace_bytes >= cow_workspace_bytes(n, h, w), "cms_cowmask: workspace of %zu bytes, %zu needed", workspace_bytes,
                cow_workspace_bytes(n, h, w));
    hipStream_t s = (hipStream_t)stream;
    const size_t plane = (size_t)n * h * w;
    double* along_x = reinterpret_cast<double*>(workspace);        // (n, w, h)
    double* smooth = along_x + plane;                              // (n, h, w)
    double* partials = smooth + plane;
    cow_blur_launch<float, false>(noise, taps, along_x, nullptr, n, h, w, radius, s);
    cow_blur_launch<double, true>(along_x, taps, smooth, partials, n, w, h, radius, s);
    const dim3 grid(grid_for((size_t)h * w, kCowThreads, 512), n), block(kCowThreads);
    hipLaunchKernelGGL(cow_threshold_kernel, grid, block, 0, s, smooth, partials, thresh_factor, mask_out, stats_out, h, w);
    return launch_status("cms_cowmask");
}
