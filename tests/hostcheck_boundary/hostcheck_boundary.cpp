// test infrastructure: a stand-alone host driver of the product's boundary-score arithmetic (csrc/boundary_math.hpp), the very
// functions the kernels of csrc/boundary.hip call, walked chunk by chunk, lane by lane and pixel by pixel as the launches walk them.
// A ballot of the kernel is a loop over the 64 lanes here.
//
//   hostcheck_boundary REQUEST RESULT
//
// REQUEST, little-endian: int32 n, h, w, num_classes, ignore_index, k, maps_wanted; then n * k int32 widths; then the (n, h, w) uint8 truth and
// the (n, h, w) uint8 prediction.
// RESULT: n * h * w uint8 D_T, n * h * w uint8 D_P, k * (c+1)^2 int64 bcm, k * c^2 int64 tcm. With maps_wanted the maps are
// min(D, 255) as a caller receives them; without, what pass 2 leaves in the workspace: min(D, the sample's widest band + 1).
// Every tensor, the workspace and the histogram of a "workgroup" live in exactly-sized heap blocks, and the workspace is filled with
// 0xA5 before use, so a sanitizer build sees every byte outside them and a byte a later pass reads without an earlier one having
// written it shows in the result. Exit code 2 for a request the product refuses (the refusal is the product's own check).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cutmix-semisup-seg_amd/csrc/boundary_math.hpp"
#include "../hostcheck_common.hpp"

using namespace cms;
typedef unsigned long long u64;

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_boundary REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[7];
    if (fread(head, sizeof(int32_t), 7, f) != 7) return 1;
    const bool maps_wanted = head[6] != 0;
    cms_boundary_desc d;
    memset(&d, 0, sizeof(d));
    d.n = head[0], d.h = head[1], d.w = head[2], d.num_classes = head[3], d.ignore_index = head[4], d.k = head[5];
    // the product's verdict on the sizes before anything is read or allocated by them
    alignas(16) static char probe[16];
    d.truth = d.pred = (const uint8_t*)probe, d.widths = (const int32_t*)probe, d.bcm = d.tcm = (int64_t*)probe, d.workspace = probe;
    d.workspace_bytes = (size_t)-1;
    if (boundary_check(&d)) return 2;
    const int H = d.h, W = d.w, C = d.num_classes, K = d.k, ignore = d.ignore_index;
    const size_t hw = (size_t)H * W, pix = (size_t)d.n * hw;
    int32_t* widths = (int32_t*)read_block(f, (size_t)d.n * K * sizeof(int32_t));
    uint8_t* truth = (uint8_t*)read_block(f, pix);
    uint8_t* pred = (uint8_t*)read_block(f, pix);
    fclose(f);
    const size_t ws_bytes = boundary_workspace_bytes(d.n, H, W), map = boundary_map_bytes(d.n, H, W);
    uint8_t* ws = (uint8_t*)aligned_alloc(16, ws_bytes);
    memset(ws, 0xA5, ws_bytes);
    const size_t B = (size_t)(C + 1) * (C + 1), CC = (size_t)C * C;
    int64_t* bcm = (int64_t*)calloc(K * B, sizeof(int64_t));
    int64_t* tcm = (int64_t*)calloc(K * CC, sizeof(int64_t));
    d.truth = truth, d.pred = pred, d.widths = widths, d.bcm = bcm, d.tcm = tcm, d.workspace = ws, d.workspace_bytes = ws_bytes;
    if (boundary_check(&d)) return 2;
    uint32_t* row_words = (uint32_t*)ws;
    uint8_t *dist_t = ws + boundary_rows_bytes(d.n, H, W), *dist_p = dist_t + map;

    // ---- pass 1: a wavefront per 64 pixels of a row
    const int cpr = (W + kBdLanes - 1) / kBdLanes;
    const long long rows = (long long)d.n * H;
    for (long long c = 0; c < rows * cpr; ++c) {
        const long long row = c / cpr, cx = (c - row * cpr) * kBdLanes;
        const uint8_t* trow = truth + row * W;
        const uint8_t* prow = pred + row * W;
        // flags of the 64 positions from `base`: first[0/1] = first pixel of a run of T / P, last[0/1] = last pixel
        auto ballots = [&](long long base, u64* first, u64* last) {
            first[0] = first[1] = last[0] = last[1] = 0;
            for (int lane = 0; lane < kBdLanes; ++lane) {
                const long long q = base + lane;
                const BdPair a = bd_row_values(trow, prow, q - 1, W, ignore), b = bd_row_values(trow, prow, q, W, ignore),
                             e = bd_row_values(trow, prow, q + 1, W, ignore);
                first[0] |= (u64)(b.t != a.t) << lane, first[1] |= (u64)(b.p != a.p) << lane;
                last[0] |= (u64)(b.t != e.t) << lane, last[1] |= (u64)(b.p != e.p) << lane;
            }
        };
        long long left[2][kBdLanes], right[2][kBdLanes];
        u64 first[2], last[2];
        ballots(cx, first, last);
        for (int m = 0; m < 2; ++m)
            for (int lane = 0; lane < kBdLanes; ++lane) {
                const int i = bd_last_at_or_below(first[m], lane), j = bd_first_at_or_above(last[m], lane);
                left[m][lane] = i != kBdNone ? lane - i : kBdNone;
                right[m][lane] = j != kBdNone ? j - lane : kBdNone;
            }
        for (int j = 1; j <= kBdReach; ++j) {
            bool need_l = false, need_r = false;
            for (int lane = 0; lane < kBdLanes; ++lane) {
                const bool in = cx + lane < W;
                need_l |= in && (left[0][lane] == kBdNone || left[1][lane] == kBdNone);
                need_r |= in && (right[0][lane] == kBdNone || right[1][lane] == kBdNone);
            }
            if (!need_l && !need_r) break;
            if (need_l) {
                const long long base = cx - (long long)j * kBdLanes;
                ballots(base, first, last);
                for (int m = 0; m < 2; ++m) {
                    const int i = bd_last_at_or_below(first[m], kBdLanes - 1);
                    for (int lane = 0; lane < kBdLanes; ++lane)
                        if (left[m][lane] == kBdNone && i != kBdNone) left[m][lane] = cx + lane - (base + i);
                }
            }
            if (need_r) {
                const long long base = cx + (long long)j * kBdLanes;
                ballots(base, first, last);
                for (int m = 0; m < 2; ++m) {
                    const int i = bd_first_at_or_above(last[m], 0);
                    for (int lane = 0; lane < kBdLanes; ++lane)
                        if (right[m][lane] == kBdNone && i != kBdNone) right[m][lane] = (base + i) - (cx + lane);
                }
            }
        }
        for (int lane = 0; lane < kBdLanes; ++lane)
            if (cx + lane < W) {
                const BdPair b = bd_row_values(trow, prow, cx + lane, W, ignore);
                row_words[row * W + cx + lane] =
                    bd_pack(b.t, bd_row_dist(left[0][lane], right[0][lane]), b.p, bd_row_dist(left[1][lane], right[1][lane]));
            }
    }

    // ---- pass 2: a thread per pixel
    for (size_t idx = 0; idx < pix; ++idx) {
        const size_t row = idx / W;
        const int y = (int)(row % H);
        const size_t col = idx - (size_t)y * W;
        const int cap = bd_walk_cap(widths + (row / H) * K, K, maps_wanted);
        BdDist dd;
        dd.t = dd.p = 0;
        if (truth[idx] != ignore) dd = bd_column_walk(row_words[idx], y, H, [&](int yy) { return row_words[col + (size_t)yy * W]; }, cap);
        dist_t[idx] = (uint8_t)dd.t;
        dist_p[idx] = (uint8_t)dd.p;
    }

    // ---- pass 3: one "workgroup" per launch, its histogram in a block of exactly the bytes the launch asks for
    const int per = boundary_widths_per_launch(C, K);
    for (int k0 = 0; k0 < K; k0 += per) {
        const int kk = K - k0 < per ? K - k0 : per;
        const size_t lds = kk * boundary_width_bytes(C);
        if (lds > kBdLdsBytes) return 3;
        unsigned int* hist = (unsigned int*)calloc(1, lds);
        const size_t nb = kk * B, nt = kk * CC;
        for (size_t idx = 0; idx < pix; ++idx) {
            const int t = truth[idx], p = pred[idx];
            if (!bd_counted(t, p, ignore, C)) continue;
            const int dt = dist_t[idx], dp = dist_p[idx];
            const int32_t* wd = widths + (idx / hw) * K + k0;
            for (int j = 0; j < kk; ++j) {
                const int dd = bd_clamp_width(wd[j]);
                hist[j * B + bd_bcm_bin(t, p, dt, dp, dd, C)] += 1;
                const int tb = bd_tcm_bin(t, p, dt, dd, C);
                if (tb >= 0) hist[nb + j * CC + tb] += 1;
            }
        }
        for (size_t i = 0; i < nb; ++i) bcm[k0 * B + i] += hist[i];
        for (size_t i = 0; i < nt; ++i) tcm[k0 * CC + i] += hist[nb + i];
        free(hist);
    }

    FILE* g = fopen(argv[2], "wb");
    if (!g) return 1;
    if (fwrite(dist_t, 1, pix, g) != pix || fwrite(dist_p, 1, pix, g) != pix || fwrite(bcm, 8, K * B, g) != K * B ||
        fwrite(tcm, 8, K * CC, g) != K * CC)
        return 1;
    fclose(g);
    free(widths), free(truth), free(pred), free(ws), free(bcm), free(tcm);
    return 0;
}
