// Boundary IoU and trimap IoU (gfx950): the capped Chebyshev distance-to-boundary maps of a truth and a prediction map, and the two
// integer confusion matrices built on them (Cheng et al., "Boundary IoU", CVPR 2021; the trimap plots of the DeepLab papers). Written
// with tensor operations this is a one-hot tensor (N, C, H, W) and a max-pool of window 2d + 1 per width; here it is
//   pass 1  rows: a wavefront owns 64 consecutive pixels of one row. The flags "first pixel of a run" / "last pixel of a run" of the
//           64 positions are two ballots, and a lane finds its run's ends with a count of leading / trailing zeros; lanes whose run
//           leaves the chunk look at up to four chunks on either side (4 * 64 >= 255, the cap), the loop being wave-uniform. The
//           pass leaves one 32-bit word (T, r_T, P, r_P) per pixel
//   pass 2  columns: a thread owns a pixel and walks up and down its column, one word load a step for both maps: min over dy of
//           max(|dy|, row distance) while the value stays its own, stopping as soon as |dy| reaches the best value so far -- or,
//           where the maps are no output of the call, the sample's widest band + 1: in the middle of a region hundreds of pixels
//           wide that is 10 steps instead of 255
//   pass 3  counts: every pixel is binned for all widths of its sample in one read of the four maps; per-workgroup histograms in LDS
//           (integer atomics, order-independent => bit exact), one 64-bit atomic per non-empty bin, as csrc/eval.hip does
// Every index stays inside its own row (pass 1) and its own sample's column (pass 2): no window reads a neighbouring image. The
// arithmetic is csrc/boundary_math.hpp's.
#include "common.hpp"
#include "boundary_math.hpp"

namespace cms {

typedef unsigned long long u64;

__global__ __launch_bounds__(kBdBlock) void boundary_row_kernel(const uint8_t* __restrict__ truth, const uint8_t* __restrict__ pred,
                                                                int ignore, long long rows, int W, int cpr,
                                                                uint32_t* __restrict__ row_words) {
    const int lane = threadIdx.x & (kBdLanes - 1);
    const long long nwaves = (long long)gridDim.x * (kBdBlock / kBdLanes), total = rows * cpr;
    for (long long c = (long long)blockIdx.x * (kBdBlock / kBdLanes) + threadIdx.x / kBdLanes; c < total; c += nwaves) {
        const long long row = c / cpr, cx = (c - row * cpr) * kBdLanes, x = cx + lane;
        const uint8_t* trow = truth + row * W;
        const uint8_t* prow = pred + row * W;
        const bool in = x < W;
        long long lt = kBdNone, rt = kBdNone, lp = kBdNone, rp = kBdNone;      // how far the run's first / last pixel is
        const BdPair b = bd_row_values(trow, prow, x, W, ignore);
        {
            const BdPair a = bd_row_values(trow, prow, x - 1, W, ignore), e = bd_row_values(trow, prow, x + 1, W, ignore);
            const u64 ft = __ballot(b.t != a.t), gt = __ballot(b.t != e.t), fp = __ballot(b.p != a.p), gp = __ballot(b.p != e.p);
            int i;
            if ((i = bd_last_at_or_below(ft, lane)) != kBdNone) lt = lane - i;
            if ((i = bd_first_at_or_above(gt, lane)) != kBdNone) rt = i - lane;
            if ((i = bd_last_at_or_below(fp, lane)) != kBdNone) lp = lane - i;
            if ((i = bd_first_at_or_above(gp, lane)) != kBdNone) rp = i - lane;
        }
        for (int j = 1; j <= kBdReach; ++j) {
            const u64 need_l = __ballot(in && (lt == kBdNone || lp == kBdNone));
            const u64 need_r = __ballot(in && (rt == kBdNone || rp == kBdNone));
            if (!need_l && !need_r) break;
            if (need_l) {
                const long long q = cx - (long long)j * kBdLanes + lane;
                const BdPair a = bd_row_values(trow, prow, q - 1, W, ignore), b = bd_row_values(trow, prow, q, W, ignore);
                const int it = bd_last_at_or_below(__ballot(b.t != a.t), kBdLanes - 1);
                const int ip = bd_last_at_or_below(__ballot(b.p != a.p), kBdLanes - 1);
                if (lt == kBdNone && it != kBdNone) lt = x - (q - lane + it);
                if (lp == kBdNone && ip != kBdNone) lp = x - (q - lane + ip);
            }
            if (need_r) {
                const long long q = cx + (long long)j * kBdLanes + lane;
                const BdPair b = bd_row_values(trow, prow, q, W, ignore), e = bd_row_values(trow, prow, q + 1, W, ignore);
                const int it = bd_first_at_or_above(__ballot(b.t != e.t), 0);
                const int ip = bd_first_at_or_above(__ballot(b.p != e.p), 0);
                if (rt == kBdNone && it != kBdNone) rt = (q - lane + it) - x;
                if (rp == kBdNone && ip != kBdNone) rp = (q - lane + ip) - x;
            }
        }
        if (in) row_words[row * W + x] = bd_pack(b.t, bd_row_dist(lt, rt), b.p, bd_row_dist(lp, rp));
    }
}

__global__ __launch_bounds__(kBdBlock) void boundary_column_kernel(const uint8_t* __restrict__ truth,
                                                                   const uint32_t* __restrict__ row_words,
                                                                   const int* __restrict__ widths, int K, int maps_wanted,
                                                                   int ignore, size_t count, int H, int W,
                                                                   uint8_t* __restrict__ dist_t, uint8_t* __restrict__ dist_p) {
    for (size_t idx = (size_t)blockIdx.x * kBdBlock + threadIdx.x; idx < count; idx += (size_t)gridDim.x * kBdBlock) {
        const size_t row = idx / W;
        const int y = (int)(row % H);
        const int cap = bd_walk_cap(widths ? widths + (row / H) * K : nullptr, K, maps_wanted != 0);
        const size_t col = idx - (size_t)y * W;                   // the pixel of row 0 of this sample in this column
        BdDist d;
        d.t = d.p = 0;
        if (truth[idx] != ignore) d = bd_column_walk(row_words[idx], y, H, [&](int yy) { return row_words[col + (size_t)yy * W]; }, cap);
        dist_t[idx] = (uint8_t)d.t;
        dist_p[idx] = (uint8_t)d.p;
    }
}

// widths [k0, k0 + kk) of every sample; LDS: kk histograms of (C+1)^2 bins, then kk of C^2
__global__ __launch_bounds__(kBdBlock) void boundary_count_kernel(const uint8_t* __restrict__ truth, const uint8_t* __restrict__ pred,
                                                                  const uint8_t* __restrict__ dist_t, const uint8_t* __restrict__ dist_p,
                                                                  const int* __restrict__ widths, int ignore, size_t count, size_t hw,
                                                                  int C, int K, int k0, int kk, u64* __restrict__ bcm,
                                                                  u64* __restrict__ tcm) {
    extern __shared__ unsigned int bd_hist[];
    const int B = (C + 1) * (C + 1), CC = C * C, nb = kk * B, nt = kk * CC;
    for (int i = threadIdx.x; i < nb + nt; i += kBdBlock) bd_hist[i] = 0;
    __syncthreads();
    for (size_t idx = (size_t)blockIdx.x * kBdBlock + threadIdx.x; idx < count; idx += (size_t)gridDim.x * kBdBlock) {
        const int t = truth[idx], p = pred[idx];
        if (!bd_counted(t, p, ignore, C)) continue;
        const int dt = dist_t[idx], dp = dist_p[idx];
        const int* wd = widths + (idx / hw) * K + k0;
        for (int j = 0; j < kk; ++j) {
            const int d = bd_clamp_width(wd[j]);
            if (bcm) atomicAdd(&bd_hist[j * B + bd_bcm_bin(t, p, dt, dp, d, C)], 1u);
            const int tb = bd_tcm_bin(t, p, dt, d, C);
            if (tcm && tb >= 0) atomicAdd(&bd_hist[nb + j * CC + tb], 1u);
        }
    }
    __syncthreads();
    if (bcm) {
        for (int i = threadIdx.x; i < nb; i += kBdBlock) {
            const unsigned int v = bd_hist[i];
            if (v) atomicAdd(&bcm[(size_t)k0 * B + i], (u64)v);
        }
    }
    if (tcm) {
        for (int i = threadIdx.x; i < nt; i += kBdBlock) {
            const unsigned int v = bd_hist[nb + i];
            if (v) atomicAdd(&tcm[(size_t)k0 * CC + i], (u64)v);
        }
    }
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_boundary_workspace_bytes(int n, int h, int w) { return boundary_workspace_bytes(n, h, w); }

extern "C" int cms_boundary_confusion(const cms_boundary_desc* d, void* stream) {
    const char* why = boundary_check(d);
    CMS_REQUIRE(!why, "boundary_confusion: %s", why);
    hipStream_t s = (hipStream_t)stream;
    const size_t count = (size_t)d->n * d->h * d->w, map = boundary_map_bytes(d->n, d->h, d->w);
    uint8_t* ws = (uint8_t*)d->workspace;
    uint32_t* row_words = (uint32_t*)ws;
    uint8_t* maps = ws + boundary_rows_bytes(d->n, d->h, d->w);
    uint8_t* dist_t = d->dist_truth ? d->dist_truth : maps;
    uint8_t* dist_p = d->dist_pred ? d->dist_pred : maps + map;
    const int cpr = (d->w + kBdLanes - 1) / kBdLanes;
    const long long rows = (long long)d->n * d->h;
    const size_t chunks = (size_t)rows * cpr;
    hipLaunchKernelGGL(boundary_row_kernel, dim3(grid_for(chunks, kBdBlock / kBdLanes)), dim3(kBdBlock), 0, s, d->truth, d->pred,
                       d->ignore_index, rows, d->w, cpr, row_words);
    int rc = launch_status("cms_boundary_confusion (rows)");
    if (rc != CMS_OK) return rc;
    hipLaunchKernelGGL(boundary_column_kernel, dim3(grid_for(count, kBdBlock)), dim3(kBdBlock), 0, s, d->truth, row_words,
                       d->widths, d->k, (d->dist_truth || d->dist_pred) ? 1 : 0, d->ignore_index, count, d->h, d->w, dist_t, dist_p);
    rc = launch_status("cms_boundary_confusion (columns)");
    if (rc != CMS_OK || (!d->bcm && !d->tcm)) return rc;
    const int C = d->num_classes, per = boundary_widths_per_launch(C, d->k);
    for (int k0 = 0; k0 < d->k; k0 += per) {
        const int kk = d->k - k0 < per ? d->k - k0 : per;
        hipLaunchKernelGGL(boundary_count_kernel, dim3(grid_for(count, kBdBlock, kBdCountBlocks)), dim3(kBdBlock),
                           kk * boundary_width_bytes(C), s, d->truth, d->pred, dist_t, dist_p, d->widths, d->ignore_index, count,
                           (size_t)d->h * d->w, C, d->k, k0, kk, (u64*)d->bcm, (u64*)d->tcm);
        rc = launch_status("cms_boundary_confusion (counts)");
        if (rc != CMS_OK) return rc;
    }
    return CMS_OK;
}
