// Indexing and arithmetic of the CowMask generator (cowmask.hip), driven on the host by tests/hostcheck_cowmask.
// Same conventions as pixel_math.hpp / aug_math.hpp / stage_math.hpp: `__host__ __device__`, no state. All arithmetic is fp64.
//
// A CowMask (French et al., "Milking CowMask for semi-supervised image classification") is Gaussian-smoothed noise thresholded so
// that a chosen share of the pixels is 1:
//     s    = taps (*)_y (taps (*)_x noise)      separable, ZERO padding outside the image, one row of 2R+1 taps per sample
//     tau  = mean(s) + std(s) * f               std with ddof = 0, f = the standard normal's inverse CDF of the share p (host)
//     mask = s <= tau
//
// One blur pass convolves along the CONTIGUOUS axis of a (rows, cols) plane and writes its result TRANSPOSED, (cols, rows); two
// such passes give the separable blur and put the plane back in its own layout:
//     noise (H, W) f32  --along x-->  (W, H) f64  --along y-->  s (H, W) f64
// A workgroup of 256 threads owns a tile of kCowTileR rows x kCowTileC outputs along the axis. The tile's input, kCowTileC + 2R
// columns with zeros where the image ends, sits in LDS column-major with an odd pitch: lds[col * kCowPitch + row]. The 32 lanes
// of a half wave hold the 32 rows of ONE column group, so their LDS reads are 32 consecutive elements (no bank conflict for 4- or
// 8-byte elements) and their transposed global stores are 32 consecutive doubles. A thread produces kCowPerThread consecutive
// outputs from a sliding register window: one LDS read per kCowPerThread multiply-adds.
#pragma once
#include "pixel_math.hpp"

namespace cms {

constexpr int kCowTileR = 32;          // rows of a tile = lanes of a half wave
constexpr int kCowTileC = 64;          // outputs of a tile along the convolved axis
constexpr int kCowPerThread = 8;       // consecutive outputs of one thread; kCowTileC / kCowPerThread half waves = 256 threads
constexpr int kCowThreads = kCowTileR * (kCowTileC / kCowPerThread);
constexpr int kCowPitch = kCowTileR + 1;
constexpr int kCowMaxRadius = 128;

CMS_HD int cow_div_up(int a, int b) { return (a + b - 1) / b; }

// the tap loop runs in steps of kCowPerThread: taps k >= 2R+1 of the padded table are 0, and the tile carries as many extra
// (zero) columns so that the window of the last step stays inside it
CMS_HD int cow_taps_padded(int radius) { return cow_div_up(2 * radius + 1, kCowPerThread) * kCowPerThread; }
CMS_HD int cow_tile_in_cols(int radius) { return kCowTileC + cow_taps_padded(radius) + kCowPerThread; }
// bytes of LDS of one blur workgroup: the padded taps, then the tile
CMS_HD size_t cow_lds_bytes(int radius, size_t elem_bytes) {
    return (size_t)cow_taps_padded(radius) * sizeof(double) + (size_t)cow_tile_in_cols(radius) * kCowPitch * elem_bytes;
}

// element (row, col) of a plane, 0 outside it: the zero padding
template <class T>
CMS_HD double cow_fetch(const T* plane, int rows, int cols, int row, int col) {
    return (row >= 0 && row < rows && col >= 0 && col < cols) ? (double)plane[(size_t)row * cols + col] : 0.0;
}

// Output c takes tap k from input column c - R + k. For the outputs c0 .. c0 + kCowTileC - 1 of a tile the taps that can meet a
// column inside 0 .. cols-1 are k_lo .. k_hi - 1; every other product has a zero factor. Rounded outwards to whole steps, clipped
// to the padded table. An empty range (k_lo >= k_hi) cannot happen for a tile that holds an output.
CMS_HD void cow_tile_tap_range(int c0, int cols, int radius, int* k_lo, int* k_hi) {
    int lo = radius - (c0 + kCowTileC - 1);           // column c_last - R + k >= 0
    int hi = radius + cols - 1 - c0 + 1;              // column c0 - R + k <= cols - 1   (exclusive)
    const int kp = cow_taps_padded(radius);
    if (lo < 0) lo = 0;
    if (hi > 2 * radius + 1) hi = 2 * radius + 1;
    lo = (lo / kCowPerThread) * kCowPerThread;
    hi = cow_div_up(hi, kCowPerThread) * kCowPerThread;
    if (hi > kp) hi = kp;
    *k_lo = lo;
    *k_hi = hi;
}

// thread -> (row of the tile, first of its outputs along the axis)
CMS_HD int cow_thread_row(int tid) { return tid % kCowTileR; }
CMS_HD int cow_thread_col(int tid) { return (tid / kCowTileR) * kCowPerThread; }

// The kCowPerThread outputs of one thread. `tile`: lds[col * kCowPitch + row], local column l = image column c0 - R + l;
// `taps`: the padded table. acc[j] = sum_k taps[k] * tile[cl + j + k], k ascending.
template <class T>
CMS_HD void cow_blur_thread(const T* tile, const double* taps, int row, int cl, int k_lo, int k_hi, double (&acc)[kCowPerThread]) {
    constexpr int P = kCowPerThread;
    double win[2 * P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        acc[j] = 0.0;
        win[j] = (double)tile[(size_t)(cl + k_lo + j) * kCowPitch + row];
    }
    for (int k = k_lo; k < k_hi; k += P) {
#pragma unroll
        for (int j = 0; j < P; ++j) win[P + j] = (double)tile[(size_t)(cl + k + P + j) * kCowPitch + row];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const double t = taps[k + i];
#pragma unroll
            for (int j = 0; j < P; ++j) acc[j] = fma(t, win[i + j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < P; ++j) win[j] = win[P + j];
    }
}

// ---- statistics: every tile of the second pass leaves { sum, sum of squared distances to its OWN mean } in its slot; the slots
//      of a sample are combined in a fixed order (Chan et al.), so nothing cancels and the same input gives the same bits
CMS_HD int cow_tiles(int rows, int cols) { return cow_div_up(rows, kCowTileR) * cow_div_up(cols, kCowTileC); }
CMS_HD size_t cow_partial_slot(int sample, int tile_r, int tile_c, int rows, int cols) {
    return ((size_t)sample * cow_tiles(rows, cols) + (size_t)tile_r * cow_div_up(cols, kCowTileC) + tile_c) * 2;
}
// outputs of tile (tile_r, tile_c) that lie inside the plane
CMS_HD int cow_tile_count(int tile_r, int tile_c, int rows, int cols) {
    int r = rows - tile_r * kCowTileR, c = cols - tile_c * kCowTileC;
    r = r > kCowTileR ? kCowTileR : r;
    c = c > kCowTileC ? kCowTileC : c;
    return r * c;
}
// tile t's share of sum (s - mean)^2 over the sample
CMS_HD double cow_m2_term(double tile_sum, double tile_m2, int count, double mean) {
    const double d = tile_sum / (double)count - mean;
    return tile_m2 + (double)count * d * d;
}
CMS_HD double cow_threshold(double mean, double m2, size_t pixels, double factor, double* std_out) {
    const double sd = sqrt(m2 / (double)pixels);
    *std_out = sd;
    return mean + sd * factor;
}
CMS_HD float cow_mask_bit(double s, double tau) { return s <= tau ? 1.0f : 0.0f; }

// bytes of the caller's workspace: two fp64 planes per sample and the tile slots
CMS_HD size_t cow_workspace_bytes(int n, int h, int w) {
    return ((size_t)2 * n * h * w + (size_t)2 * n * cow_tiles(w, h)) * sizeof(double);
}

}  // namespace cms
