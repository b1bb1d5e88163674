// Surface distances (gfx950): the exact squared Euclidean distance from every surface pixel of a class in the prediction to the
// nearest surface pixel of the same class in the truth map and back, and per (sample, class) what the Hausdorff distance, its 95th
// percentile and the average symmetric surface distance follow from (MedPy's hd / hd95 / assd, connectivity 1, unit spacing). On the
// host this is a binary erosion and a Euclidean distance transform per class and image; here it is
//   pass 1  mark: a thread owns a pixel, looks at its four edge neighbours in both maps and writes the class whose surface the pixel
//           is on, one byte per map; surface pixels are counted per (sample, class) in LDS, one integer atomic per non-empty bin
//   pass 2  rows: a wavefront owns one row of one (map, sample, class) plane. The flags "surface pixel of the class" of 64 positions
//           are a ballot, a lane finds the nearest one with a count of leading / trailing zeros, and the nearest one of the chunks
//           before (after) travels along a sweep from the left (right) as a wave-uniform position. Planes of an unscored pair --
//           a class absent from either map of the sample -- are skipped at once, and are never read
//   pass 3  columns: a thread owns a pixel; where it is a surface pixel of a scored pair it walks its column in the other map's
//           plane of its class, rows y -+ dy for dy = 1, 2, ..., until dy^2 reaches the best dy^2 + r^2 so far
//   pass 4  partial maxima and fp64 sums of sqrt(d2) per (sample, class, slab) by a tree in LDS, then one thread per pair adds the
//           slabs in order: no atomics, so the same input gives the same bits
//   pass 5  the values of ranks lo and hi of the pooled squared distances by a masked radix select after csrc/patchdist.hip's: 8-bit
//           digits from the top, per pass an LDS histogram per workgroup (integer atomics) and a pick; a pass whose digit is 0 for
//           every value of the pair (most of the upper two) ends at once
// Every index stays inside its own sample. The arithmetic is csrc/surface_math.hpp's.
#include "common.hpp"
#include "surface_math.hpp"

namespace cms {

typedef unsigned long long u64;

// grid: n * bps workgroups, workgroup b takes every bps-th chunk of 256 pixels of sample b / bps
__global__ __launch_bounds__(kSfBlock) void surface_mark_kernel(const uint8_t* __restrict__ truth, const uint8_t* __restrict__ pred,
                                                                int ignore, int H, int W, int C, int bps,
                                                                uint8_t* __restrict__ surf_t, uint8_t* __restrict__ surf_p,
                                                                int32_t* __restrict__ counts) {
    __shared__ unsigned int bins[2 * kSfMaxClasses];
    if (threadIdx.x < 2 * kSfMaxClasses) bins[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x / bps, j = blockIdx.x - i * bps;
    const size_t hw = (size_t)H * W, base = (size_t)i * hw;
    for (size_t k = (size_t)j * kSfBlock + threadIdx.x; k < hw; k += (size_t)bps * kSfBlock) {
        const int y = (int)(k / W), x = (int)(k - (size_t)y * W);
        const SfPair s = sf_surface(truth + base, pred + base, x, y, H, W, ignore, C);
        surf_t[base + k] = (uint8_t)s.t;
        surf_p[base + k] = (uint8_t)s.p;
        if (s.p != kSfNoClass) atomicAdd(&bins[2 * s.p], 1u);
        if (s.t != kSfNoClass) atomicAdd(&bins[2 * s.t + 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
        const unsigned int v = bins[threadIdx.x];
        if (v) atomicAdd(&counts[(size_t)i * 2 * C + threadIdx.x], (int32_t)v);
    }
}

// item = ((map * n + sample) * C + class) * H + row, one wavefront each
__global__ __launch_bounds__(kSfBlock) void surface_row_kernel(const uint8_t* __restrict__ surf_t, const uint8_t* __restrict__ surf_p,
                                                               const int32_t* __restrict__ counts, int n, int H, int W, int C,
                                                               uint16_t* __restrict__ rows_t, uint16_t* __restrict__ rows_p) {
    const int lane = threadIdx.x & (kSfLanes - 1);
    const long long nwaves = (long long)gridDim.x * (kSfBlock / kSfLanes), total = 2ll * n * C * H;
    const int chunks = (W + kSfLanes - 1) / kSfLanes;
    for (long long item = (long long)blockIdx.x * (kSfBlock / kSfLanes) + threadIdx.x / kSfLanes; item < total; item += nwaves) {
        const int y = (int)(item % H);
        const long long pc = item / H;                                        // (map * n + sample) * C + class
        const int c = (int)(pc % C);
        const long long mi = pc / C;
        const int i = (int)(mi % n), map = (int)(mi / n);
        if (!sf_scored(counts + ((size_t)i * C + c) * 2)) continue;
        const uint8_t* srow = (map ? surf_p : surf_t) + ((size_t)i * H + y) * W;
        uint16_t* out = (map ? rows_p : rows_t) + (((size_t)i * C + c) * H + y) * W;
        int last = -1;
        for (int k = 0; k < chunks; ++k) {
            const int cx = k * kSfLanes, x = cx + lane;
            const u64 m = __ballot(x < W && srow[x] == c);
            if (x < W) out[x] = (uint16_t)sf_row_left(m, lane, x, last);
            last = sf_carry_last(m, cx, last);
        }
        if (last < 0) continue;                                               // no surface pixel in this row: kSfNoRow everywhere
        int next = -1;
        for (int k = chunks - 1; k >= 0; --k) {
            const int cx = k * kSfLanes, x = cx + lane;
            const u64 m = __ballot(x < W && srow[x] == c);
            if (x < W) {
                const int l = out[x], r = sf_row_right(m, lane, x, next);
                if (r < l) out[x] = (uint16_t)r;
            }
            next = sf_carry_next(m, cx, next);
        }
    }
}

__global__ __launch_bounds__(kSfBlock) void surface_column_kernel(const uint8_t* __restrict__ surf_t, const uint8_t* __restrict__ surf_p,
                                                                  const int32_t* __restrict__ counts,
                                                                  const uint16_t* __restrict__ rows_t,
                                                                  const uint16_t* __restrict__ rows_p, size_t count, int H, int W, int C,
                                                                  int32_t* __restrict__ d2_pred, int32_t* __restrict__ d2_truth) {
    const size_t hw = (size_t)H * W;
    for (size_t idx = (size_t)blockIdx.x * kSfBlock + threadIdx.x; idx < count; idx += (size_t)gridDim.x * kSfBlock) {
        const size_t i = idx / hw, k = idx - i * hw;
        const int y = (int)(k / W);
        const size_t col = k - (size_t)y * W;
        const int sp = surf_p[idx], st = surf_t[idx];
        int32_t dp = -1, dt = -1;
        if (sp != kSfNoClass && sf_scored(counts + (i * C + sp) * 2)) {
            const uint16_t* plane = rows_t + (i * C + sp) * hw + col;       // column x of the truth's plane of the class
            dp = sf_column_walk(plane[(size_t)y * W], y, H, [&](int yy) { return (int)plane[(size_t)yy * W]; });
        }
        if (st != kSfNoClass && sf_scored(counts + (i * C + st) * 2)) {
            const uint16_t* plane = rows_p + (i * C + st) * hw + col;
            dt = sf_column_walk(plane[(size_t)y * W], y, H, [&](int yy) { return (int)plane[(size_t)yy * W]; });
        }
        d2_pred[idx] = dp;
        d2_truth[idx] = dt;
    }
}

// workgroup = (sample * C + class) * slabs + slab
__global__ __launch_bounds__(kSfBlock) void surface_partial_kernel(const uint8_t* __restrict__ surf_t, const uint8_t* __restrict__ surf_p,
                                                                   const int32_t* __restrict__ counts,
                                                                   const int32_t* __restrict__ d2_pred,
                                                                   const int32_t* __restrict__ d2_truth, int H, int W, int C,
                                                                   SfPartial* __restrict__ partial) {
    __shared__ double sum[2][kSfBlock];
    __shared__ int32_t mx[2][kSfBlock];
    const int slabs = sf_slabs(H, W), slab = blockIdx.x % slabs;
    const size_t pair = blockIdx.x / slabs, i = pair / C;
    const int c = (int)(pair - i * C), t = threadIdx.x;
    if (!sf_scored(counts + pair * 2)) return;
    const size_t hw = (size_t)H * W, len = (size_t)sf_slab_len(H, W), base = i * hw;
    const size_t lo = slab * len, hi = lo + len < hw ? lo + len : hw;
    double s0 = 0.0, s1 = 0.0;
    int32_t m0 = -1, m1 = -1;
    for (size_t k = lo + t; k < hi; k += kSfBlock) {
        if (surf_p[base + k] == c) {
            const int32_t v = d2_pred[base + k];
            s0 += sqrt((double)v), m0 = v > m0 ? v : m0;
        }
        if (surf_t[base + k] == c) {
            const int32_t v = d2_truth[base + k];
            s1 += sqrt((double)v), m1 = v > m1 ? v : m1;
        }
    }
    sum[0][t] = s0, sum[1][t] = s1, mx[0][t] = m0, mx[1][t] = m1;
    __syncthreads();
    for (int stride = kSfBlock / 2; stride > 0; stride >>= 1) {
        if (t < stride) sf_tree_step(sum[0], mx[0], t, stride), sf_tree_step(sum[1], mx[1], t, stride);
        __syncthreads();
    }
    if (t == 0) {
        SfPartial p;
        p.sum[0] = sum[0][0], p.sum[1] = sum[1][0], p.max_d2[0] = mx[0][0], p.max_d2[1] = mx[1][0], p.pad[0] = p.pad[1] = 0;
        partial[blockIdx.x] = p;
    }
}

// a thread per (sample, class): the counts, the slabs in order, the ranks the select looks for
__global__ __launch_bounds__(kSfBlock) void surface_finish_kernel(const int32_t* __restrict__ counts,
                                                                  const SfPartial* __restrict__ partial, size_t pairs, int slabs,
                                                                  SfState* __restrict__ state, int64_t* __restrict__ stats,
                                                                  double* __restrict__ sums) {
    const size_t pair = (size_t)blockIdx.x * kSfBlock + threadIdx.x;
    if (pair >= pairs) return;
    const int32_t* cnt = counts + pair * 2;
    SfState st;
    st.max_d2 = -1, st.prefix[0] = st.prefix[1] = st.remaining[0] = st.remaining[1] = 0, st.pad[0] = st.pad[1] = st.pad[2] = 0;
    double s0 = 0.0, s1 = 0.0;
    int32_t m0 = -1, m1 = -1;
    if (sf_scored(cnt)) {
        for (int s = 0; s < slabs; ++s) {
            const SfPartial p = partial[pair * slabs + s];
            s0 += p.sum[0], s1 += p.sum[1];
            m0 = p.max_d2[0] > m0 ? p.max_d2[0] : m0, m1 = p.max_d2[1] > m1 ? p.max_d2[1] : m1;
        }
        const u64 m = (u64)cnt[0] + (u64)cnt[1];
        st.max_d2 = m0 > m1 ? m0 : m1;
        st.remaining[0] = (uint32_t)sf_rank_lo(m), st.remaining[1] = (uint32_t)sf_rank_hi(m);
    }
    state[pair] = st;
    if (stats) {
        int64_t* o = stats + pair * 6;
        o[0] = cnt[0], o[1] = cnt[1], o[2] = m0, o[3] = m1, o[4] = o[5] = -1;
    }
    if (sums) sums[pair * 2] = s0, sums[pair * 2 + 1] = s1;
}

// workgroup = (sample * C + class) * slabs + slab; hist (pairs, 2, 256) += the digit at `shift` of the values that share a prefix
__global__ __launch_bounds__(kSfBlock) void surface_histogram_kernel(const uint8_t* __restrict__ surf_t,
                                                                     const uint8_t* __restrict__ surf_p,
                                                                     const int32_t* __restrict__ d2_pred,
                                                                     const int32_t* __restrict__ d2_truth, int H, int W, int C,
                                                                     int shift, const SfState* __restrict__ state,
                                                                     uint32_t* __restrict__ hist) {
    __shared__ unsigned int bins[2][256];
    const int slabs = sf_slabs(H, W), slab = blockIdx.x % slabs;
    const size_t pair = blockIdx.x / slabs, i = pair / C;
    const int c = (int)(pair - i * C), t = threadIdx.x;
    const SfState st = state[pair];
    if (sf_pass_skipped(st.max_d2, shift)) return;
    bins[0][t] = bins[1][t] = 0;
    __syncthreads();
    const size_t hw = (size_t)H * W, len = (size_t)sf_slab_len(H, W), base = i * hw;
    const size_t lo = slab * len, hi = lo + len < hw ? lo + len : hw;
    for (size_t k = lo + t; k < hi; k += kSfBlock) {
        for (int dir = 0; dir < 2; ++dir) {
            if ((dir ? surf_t : surf_p)[base + k] != c) continue;
            const uint32_t v = (uint32_t)(dir ? d2_truth : d2_pred)[base + k];
            if (sf_in_prefix(v, st.prefix[0], shift)) atomicAdd(&bins[0][v >> shift & 255u], 1u);
            if (sf_in_prefix(v, st.prefix[1], shift)) atomicAdd(&bins[1][v >> shift & 255u], 1u);
        }
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
        const unsigned int v = bins[r][t];
        if (v) atomicAdd(&hist[(pair * 2 + r) * 256 + t], v);
    }
}

// a thread per (sample, class) and rank: the digit that holds the rank; the histogram is cleared for the next pass
__global__ __launch_bounds__(kSfBlock) void surface_pick_kernel(SfState* __restrict__ state, uint32_t* __restrict__ hist, size_t pairs,
                                                                int shift, int64_t* __restrict__ stats) {
    const size_t id = (size_t)blockIdx.x * kSfBlock + threadIdx.x, pair = id >> 1;
    const int r = (int)(id & 1);
    if (pair >= pairs) return;
    const int32_t max_d2 = state[pair].max_d2;
    if (max_d2 < 0) return;
    if (!sf_pass_skipped(max_d2, shift)) {
        uint32_t* h = hist + (pair * 2 + r) * 256;
        uint32_t rem = state[pair].remaining[r];
        const int d = sf_pick_digit(h, &rem);
        state[pair].prefix[r] |= (uint32_t)d << shift;
        state[pair].remaining[r] = rem;
        for (int k = 0; k < 256; ++k) h[k] = 0;
    }
    if (shift == 0 && stats) stats[pair * 6 + 4 + r] = state[pair].prefix[r];
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_surface_workspace_bytes(int n, int h, int w, int num_classes) {
    return surface_workspace_bytes(n, h, w, num_classes);
}

extern "C" int cms_surface_distances(const cms_surface_desc* d, void* stream) {
    const char* why = surface_check(d);
    CMS_REQUIRE(!why, "surface_distances: %s", why);
    hipStream_t s = (hipStream_t)stream;
    const int n = d->n, H = d->h, W = d->w, C = d->num_classes;
    const SfLayout l = surface_layout(n, H, W, C);
    const size_t hw = (size_t)H * W, count = (size_t)n * hw, pairs = (size_t)n * C;
    uint8_t* ws = (uint8_t*)d->workspace;
    int32_t* counts = (int32_t*)(ws + l.counts);
    uint32_t* hist = (uint32_t*)(ws + l.hist);
    SfState* state = (SfState*)(ws + l.state);
    SfPartial* partial = (SfPartial*)(ws + l.partial);
    uint8_t *surf_t = ws + l.surf, *surf_p = surf_t + l.map;
    int32_t* d2_pred = d->d2_pred ? d->d2_pred : (int32_t*)(ws + l.d2);
    int32_t* d2_truth = d->d2_truth ? d->d2_truth : (int32_t*)(ws + l.d2 + l.d2map);
    uint16_t *rows_t = (uint16_t*)(ws + l.rows), *rows_p = (uint16_t*)(ws + l.rows + l.plane);
    if (hipMemsetAsync(ws, 0, l.zeroed, s) != hipSuccess) return launch_status("cms_surface_distances (memset)");

    size_t bps = (hw + kSfBlock - 1) / kSfBlock;
    if (bps > (size_t)kSfMarkBlocks) bps = kSfMarkBlocks;
    hipLaunchKernelGGL(surface_mark_kernel, dim3((unsigned)(n * bps)), dim3(kSfBlock), 0, s, d->truth, d->pred, d->ignore_index, H, W, C,
                       (int)bps, surf_t, surf_p, counts);
    int rc = launch_status("cms_surface_distances (mark)");
    if (rc != CMS_OK) return rc;
    hipLaunchKernelGGL(surface_row_kernel, dim3(grid_for(2 * pairs * H, kSfBlock / kSfLanes, 1 << 16)), dim3(kSfBlock), 0, s, surf_t,
                       surf_p, counts, n, H, W, C, rows_t, rows_p);
    rc = launch_status("cms_surface_distances (rows)");
    if (rc != CMS_OK) return rc;
    hipLaunchKernelGGL(surface_column_kernel, dim3(grid_for(count, kSfBlock, 1 << 16)), dim3(kSfBlock), 0, s, surf_t, surf_p, counts,
                       rows_t, rows_p, count, H, W, C, d2_pred, d2_truth);
    rc = launch_status("cms_surface_distances (columns)");
    if (rc != CMS_OK || (!d->stats && !d->sums)) return rc;

    const int slabs = sf_slabs(H, W);
    const unsigned per_pair = (unsigned)((pairs + kSfBlock - 1) / kSfBlock), per_rank = (unsigned)((2 * pairs + kSfBlock - 1) / kSfBlock);
    hipLaunchKernelGGL(surface_partial_kernel, dim3((unsigned)(pairs * slabs)), dim3(kSfBlock), 0, s, surf_t, surf_p, counts, d2_pred,
                       d2_truth, H, W, C, partial);
    rc = launch_status("cms_surface_distances (partial sums)");
    if (rc != CMS_OK) return rc;
    hipLaunchKernelGGL(surface_finish_kernel, dim3(per_pair), dim3(kSfBlock), 0, s, counts, partial, pairs, slabs, state, d->stats,
                       d->sums);
    rc = launch_status("cms_surface_distances (sums)");
    if (rc != CMS_OK || !d->stats) return rc;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(surface_histogram_kernel, dim3((unsigned)(pairs * slabs)), dim3(kSfBlock), 0, s, surf_t, surf_p, d2_pred,
                           d2_truth, H, W, C, shift, state, hist);
        rc = launch_status("cms_surface_distances (select histogram)");
        if (rc != CMS_OK) return rc;
        hipLaunchKernelGGL(surface_pick_kernel, dim3(per_rank), dim3(kSfBlock), 0, s, state, hist, pairs, shift, d->stats);
        rc = launch_status("cms_surface_distances (select pick)");
        if (rc != CMS_OK) return rc;
    }
    return CMS_OK;
}
