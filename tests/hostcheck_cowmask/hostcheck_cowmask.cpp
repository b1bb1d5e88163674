// test infrastructure: a stand-alone host driver of the product's CowMask arithmetic (csrc/cowmask_math.hpp), the very functions the
// kernels of csrc/cowmask.hip call, walked workgroup by workgroup and thread by thread as the three launches walk them.
//
//   hostcheck_cowmask REQUEST RESULT
//
// REQUEST: four little-endian int32 -- n, h, w, radius -- then n * (2 * radius + 1) float64 taps, n float64 threshold factors and
// n * h * w float32 noise. RESULT: n * h * w float32 mask, then n * 2 float64 (mean, std). The LDS image of a workgroup, the two fp64
// planes and the tile slots live in exactly-sized heap blocks (a sanitizer build sees every byte outside them), and the LDS image
// is filled with NaN outside what the kernel loads, so a read of a column the load loop skipped shows in the result.
// Exit code 2 for a request the product refuses.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cutmix-semisup-seg_amd/csrc/cowmask_math.hpp"

using namespace cms;

// fixed-order sum of one value per thread: the tree of cow_block_sum
static double block_sum(std::vector<double>& a) {
    for (int s = kCowThreads / 2; s > 0; s >>= 1)
        for (int tid = 0; tid < s; ++tid) a[tid] += a[tid + s];
    return a[0];
}

// one launch of cow_blur<T, STATS>: in (n, rows, cols) -> out (n, cols, rows)
template <class T>
static void blur(const T* in, const double* taps, double* out, double* partials, int n, int rows, int cols, int radius) {
    const int kp = cow_taps_padded(radius), ntaps = 2 * radius + 1;
    const size_t tile_elems = (size_t)cow_tile_in_cols(radius) * kCowPitch;
    if (cow_lds_bytes(radius, sizeof(T)) != kp * sizeof(double) + tile_elems * sizeof(T)) exit(3);
    for (int sample = 0; sample < n; ++sample)
        for (int by = 0; by < cow_div_up(rows, kCowTileR); ++by)
            for (int bx = 0; bx < cow_div_up(cols, kCowTileC); ++bx) {
                double* taps_s = (double*)malloc(kp * sizeof(double));
                T* tile = (T*)malloc(tile_elems * sizeof(T));
                for (size_t i = 0; i < tile_elems; ++i) tile[i] = (T)NAN;
                const int r0 = by * kCowTileR, c0 = bx * kCowTileC;
                const T* plane = in + (size_t)sample * rows * cols;
                int k_lo, k_hi;
                cow_tile_tap_range(c0, cols, radius, &k_lo, &k_hi);
                if (k_lo < 0 || k_hi > kp || k_lo >= k_hi || k_lo % kCowPerThread || k_hi % kCowPerThread) exit(3);
                for (int k = 0; k < kp; ++k) taps_s[k] = k < ntaps ? taps[(size_t)sample * ntaps + k] : 0.0;
                const int l_end = k_hi + kCowTileC;
                for (int tid = 0; tid < kCowThreads; ++tid)
                    for (int rl = tid / 64; rl < kCowTileR; rl += kCowThreads / 64)
                        for (int l = k_lo + (tid % 64); l < l_end; l += 64)
                            tile[(size_t)l * kCowPitch + rl] = (T)cow_fetch(plane, rows, cols, r0 + rl, c0 - radius + l);
                std::vector<double> sums(kCowThreads, 0.0), m2s(kCowThreads, 0.0);
                std::vector<double> accs((size_t)kCowThreads * kCowPerThread);
                double* oplane = out + (size_t)sample * rows * cols;
                for (int tid = 0; tid < kCowThreads; ++tid) {
                    const int row = cow_thread_row(tid), cl = cow_thread_col(tid);
                    double acc[kCowPerThread];
                    cow_blur_thread(tile, taps_s, row, cl, k_lo, k_hi, acc);
                    for (int j = 0; j < kCowPerThread; ++j) {
                        accs[(size_t)tid * kCowPerThread + j] = acc[j];
                        if (r0 + row < rows && c0 + cl + j < cols) {
                            oplane[(size_t)(c0 + cl + j) * rows + (r0 + row)] = acc[j];
                            sums[tid] += acc[j];
                        }
                    }
                }
                if (partials) {
                    const double tile_sum = block_sum(sums);
                    const double tile_mean = tile_sum / (double)cow_tile_count(by, bx, rows, cols);
                    for (int tid = 0; tid < kCowThreads; ++tid) {
                        const int row = cow_thread_row(tid), cl = cow_thread_col(tid);
                        for (int j = 0; j < kCowPerThread; ++j)
                            if (r0 + row < rows && c0 + cl + j < cols) {
                                const double d = accs[(size_t)tid * kCowPerThread + j] - tile_mean;
                                m2s[tid] = fma(d, d, m2s[tid]);
                            }
                    }
                    double* slot = partials + cow_partial_slot(sample, by, bx, rows, cols);
                    slot[0] = tile_sum;
                    slot[1] = block_sum(m2s);
                }
                free(tile);
                free(taps_s);
            }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_cowmask REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[4];
    if (fread(head, sizeof(int32_t), 4, f) != 4) return 1;
    const int n = head[0], h = head[1], w = head[2], radius = head[3];
    if (n < 1 || h < 1 || w < 1 || radius < 0 || radius > kCowMaxRadius) return 2;
    const int ntaps = 2 * radius + 1;
    const size_t pixels = (size_t)h * w, plane = (size_t)n * pixels;
    double* taps = (double*)malloc((size_t)n * ntaps * sizeof(double));
    double* factor = (double*)malloc(n * sizeof(double));
    float* noise = (float*)malloc(plane * sizeof(float));
    if (fread(taps, sizeof(double), (size_t)n * ntaps, f) != (size_t)n * ntaps) return 1;
    if (fread(factor, sizeof(double), n, f) != (size_t)n) return 1;
    if (fread(noise, sizeof(float), plane, f) != plane) return 1;
    fclose(f);

    // the caller's workspace, carved up as cms_cowmask carves it
    const size_t ws_bytes = cow_workspace_bytes(n, h, w);
    if (ws_bytes != (2 * plane + (size_t)2 * n * cow_tiles(w, h)) * sizeof(double)) return 3;
    double* ws = (double*)malloc(ws_bytes);
    double *along_x = ws, *smooth = ws + plane, *partials = smooth + plane;
    blur<float>(noise, taps, along_x, nullptr, n, h, w, radius);
    blur<double>(along_x, taps, smooth, partials, n, w, h, radius);

    float* mask = (float*)malloc(plane * sizeof(float));
    double* stats = (double*)malloc((size_t)n * 2 * sizeof(double));
    const int rows = w, cols = h, tiles_c = cow_div_up(cols, kCowTileC), tiles = cow_tiles(rows, cols);
    for (int sample = 0; sample < n; ++sample) {
        const double* slots = partials + cow_partial_slot(sample, 0, 0, rows, cols);
        std::vector<double> v(kCowThreads, 0.0);
        for (int tid = 0; tid < kCowThreads; ++tid)
            for (int t = tid; t < tiles; t += kCowThreads) v[tid] += slots[2 * t];
        const double mean = block_sum(v) / (double)pixels;
        std::fill(v.begin(), v.end(), 0.0);
        for (int tid = 0; tid < kCowThreads; ++tid)
            for (int t = tid; t < tiles; t += kCowThreads)
                v[tid] += cow_m2_term(slots[2 * t], slots[2 * t + 1], cow_tile_count(t / tiles_c, t % tiles_c, rows, cols), mean);
        const double m2 = block_sum(v);
        double sd;
        const double tau = cow_threshold(mean, m2, pixels, factor[sample], &sd);
        stats[2 * sample] = mean;
        stats[2 * sample + 1] = sd;
        for (size_t i = 0; i < pixels; ++i) mask[sample * pixels + i] = cow_mask_bit(smooth[sample * pixels + i], tau);
    }

    FILE* g = fopen(argv[2], "wb");
    if (!g) return 1;
    if (fwrite(mask, sizeof(float), plane, g) != plane) return 1;
    if (fwrite(stats, sizeof(double), (size_t)n * 2, g) != (size_t)n * 2) return 1;
    fclose(g);
    free(taps); free(factor); free(noise); free(ws); free(mask); free(stats);
    return 0;
}
