// CRF refinement kernels (gfx950): the unary launch and the mean-field launch of cms_crf_refine (include/cutmixseg.h states the
// definition, csrc/crf_math.hpp holds the arithmetic). The reference has nothing of the kind. Written with tensor operations,
// an iteration materialises an (N, C (2R+1)^2, H, W) unfold or (2R+1)^2 shifted copies of the class probabilities; here it is one
// launch per iteration. A workgroup owns a 32 x 8 tile of ONE residue class of a sample's dilation sublattice -- the pixels
// (ry + S i, rx + S j) of its rectangle -- so its dilated window is dense: the (32 + 2R) x (8 + 2R) halo of Q (up to 32 classes
// at a time, planar, so a wavefront's two rows of 32 read conflict-free) and of the packed colours sits in LDS, a thread owns a
// pixel, recomputes its (2R+1)^2 - 1 pair weights (one expf each) and keeps the messages of the chunk in registers. The last
// iteration fuses the argmax, the C x C histogram (LDS integer atomics, one 64-bit atomic per non-empty bin, as csrc/eval.hip)
// and the two counts. The rectangles of up to 32 samples travel as kernel arguments; a larger batch takes more launches.
#include "common.hpp"
#include "crf_math.hpp"

namespace cms {

constexpr int kCrfBlock = kCrfTileW * kCrfTileH;
typedef unsigned long long u64;

struct CrfGeom {
    CrfRects rects;
    int n, C, H, W, R, S;
};

__device__ __forceinline__ int crf_label(const void* labels, int label_dtype, size_t pix) {
    if (label_dtype == CMS_LABEL_U8) return (int)((const uint8_t*)labels)[pix];
    const int64_t v = ((const int64_t*)labels)[pix];
    return (v < 0 || v > 0x7fffffff) ? -1 : (int)v;
}

// One thread per canvas pixel: the vote's scores in an LDS column, then P, log P and the unary argmax; a pixel outside its sample's
// rectangle is finished here (prediction, histogram, q_out = P).
__global__ __launch_bounds__(256) void crf_unary_kernel(const TtaViews v, int k, const CrfGeom g, int align, const void* labels,
                                                        int label_dtype, int ignore_index, float* __restrict__ logp,
                                                        float* __restrict__ q0, uint8_t* __restrict__ uarg,
                                                        u64* __restrict__ cm, uint8_t* __restrict__ pred_out,
                                                        float* __restrict__ q_out) {
    extern __shared__ __attribute__((aligned(16))) float crf_smem[];
    const int C = g.C;
    float* score = crf_smem;                                                        // [C][256]
    unsigned int* hist = reinterpret_cast<unsigned int*>(crf_smem + C * 256);      // [C][C]
    const bool count = labels != nullptr && cm != nullptr;
    if (count) {
        for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0;
    }
    __syncthreads();
    const size_t plane = (size_t)g.H * g.W;
    const size_t P = (size_t)g.n * plane;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < P; idx += (size_t)gridDim.x * 256) {
        const int x = (int)(idx % g.W);
        const size_t t = idx / g.W;
        const int y = (int)(t % g.H);
        const int n = (int)(t / g.H);
        const int best = tta_vote_pixel(v, k, n, C, y, x, align != 0, [&](int c) -> float& { return score[c * 256 + threadIdx.x]; });
        const int u = y - g.rects.top[n], vv = x - g.rects.left[n];
        const bool inside = u >= 0 && u < g.rects.h[n] && vv >= 0 && vv < g.rects.w[n];
        const size_t base = (size_t)n * C * plane + (size_t)y * g.W + x;
        for (int c = 0; c < C; ++c) {
            float p, lp;
            crf_unary_value(score[c * 256 + threadIdx.x], k, &p, &lp);
            logp[base + c * plane] = lp;
            q0[base + c * plane] = p;
            if (q_out && !inside) q_out[base + c * plane] = p;
        }
        uarg[idx] = (uint8_t)best;
        if (!inside) {
            if (pred_out) pred_out[idx] = (uint8_t)best;
            if (count) {
                const int tr = crf_label(labels, label_dtype, idx);
                if (tr != ignore_index && tr >= 0 && tr < C) atomicAdd(&hist[tr * C + best], 1u);
            }
        }
    }
    __syncthreads();
    if (count) {
        for (int i = threadIdx.x; i < C * C; i += 256) {
            const unsigned int val = hist[i];
            if (val) atomicAdd(&cm[i], (u64)val);
        }
    }
}

// One mean-field iteration. grid = (tiles of the largest sublattice, S * S residue classes, samples); CC classes per chunk.
// LAST: also the argmax, the prediction, the histogram and the counts. With more than one chunk (C > 32) the messages pass through
// q_dst, which is then never NULL; with one chunk q_dst is written only when it is given.
template <int CC, bool LAST>
__global__ __launch_bounds__(kCrfBlock) void crf_meanfield_kernel(const CrfGeom g, const CrfTables tab, float w_b, float inv2b,
                                                                  int tiles_x, const uint8_t* __restrict__ rgb,
                                                                  const float* __restrict__ logp, const float* __restrict__ q_src,
                                                                  float* __restrict__ q_dst, const uint8_t* __restrict__ uarg,
                                                                  const void* labels, int label_dtype, int ignore_index,
                                                                  u64* __restrict__ cm, uint8_t* __restrict__ pred_out,
                                                                  u64* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float crf_smem[];
    const int C = g.C, R = g.R, S = g.S;
    const int n = blockIdx.z;
    const int ry = blockIdx.y / S, rx = blockIdx.y % S;
    const int top = g.rects.top[n], left = g.rects.left[n], h = g.rects.h[n], w = g.rects.w[n];
    if (ry >= h || rx >= w) return;
    const int hi = (h - ry + S - 1) / S, wi = (w - rx + S - 1) / S;          // the sublattice of this residue class
    const int i0 = (blockIdx.x / tiles_x) * kCrfTileH, j0 = (blockIdx.x % tiles_x) * kCrfTileW;
    if (i0 >= hi || j0 >= wi) return;
    const int HW = kCrfTileW + 2 * R, HH = kCrfTileH + 2 * R, HP = HW * HH;
    uint32_t* rgb_s = reinterpret_cast<uint32_t*>(crf_smem);                  // [HP] packed colour, 0 = not a neighbour
    int* off_s = reinterpret_cast<int*>(crf_smem) + HP;                       // [HP] offset in the canvas plane, -1 = none
    float* q_s = crf_smem + 2 * HP;                                           // [CC][HP]
    unsigned int* hist = reinterpret_cast<unsigned int*>(q_s + CC * HP);      // LAST: [C][C], then the two counts
    const size_t plane = (size_t)g.H * g.W;
    const bool count = LAST && labels != nullptr && cm != nullptr;
    if (LAST) {
        for (int i = threadIdx.x; i < C * C + 2; i += kCrfBlock) hist[i] = 0;
    }
    const uint8_t* img = rgb + (size_t)n * 3 * plane;
    for (int pos = threadIdx.x; pos < HP; pos += kCrfBlock) {
        const int i = i0 - R + pos / HW, j = j0 - R + pos % HW;
        uint32_t px = 0;
        int off = -1;
        if (i >= 0 && i < hi && j >= 0 && j < wi) {
            off = (top + ry + S * i) * g.W + left + rx + S * j;
            px = crf_pack_rgb(img[off], img[plane + off], img[2 * plane + off]);
        }
        rgb_s[pos] = px;
        off_s[pos] = off;
    }
    const int ly = threadIdx.x / kCrfTileW, lx = threadIdx.x % kCrfTileW;
    const bool active = i0 + ly < hi && j0 + lx < wi;
    const int u = ry + S * (i0 + ly), vv = rx + S * (j0 + lx);
    const size_t pix = (size_t)(top + u) * g.W + left + vv;                   // in the plane; meaningful when active
    const size_t base = (size_t)n * C * plane + pix;
    const int centre = (ly + R) * HW + lx + R;
    const int n_nb = active ? crf_neighbours(u, vv, h, w, R, S) : 0;
    const bool one_chunk = C <= CC;
    float acc[CC];
    for (int c0 = 0; c0 < C; c0 += CC) {
        __syncthreads();                      // the colours and offsets are written / the previous chunk has been read
        // a thread fills the halo positions it worked out above, the CC loads of a position independent of each other and in flight
        // together (a loop over (class, position) pairs, one load per trip: 0.87 ms per launch at 10 x 21 x 321 x 321, this 0.69)
        const float* src = q_src + ((size_t)n * C + c0) * plane;
        for (int pos = threadIdx.x; pos < HP; pos += kCrfBlock) {
            const int off = off_s[pos];
            float val[CC];
#pragma unroll
            for (int c = 0; c < CC; ++c) val[c] = (off >= 0 && c0 + c < C) ? src[(size_t)c * plane + off] : 0.0f;
#pragma unroll
            for (int c = 0; c < CC; ++c) q_s[c * HP + pos] = val[c];
        }
        __syncthreads();
        if (active) {
            crf_message<CC>(
                tab, R, w_b, inv2b, [&](int dy, int dx) { return rgb_s[centre + dy * HW + dx]; },
                [&](int dy, int dx, int c) { return q_s[c * HP + centre + dy * HW + dx]; }, acc);
            if (!one_chunk) {
#pragma unroll
                for (int c = 0; c < CC; ++c)
                    if (c0 + c < C) q_dst[base + (size_t)(c0 + c) * plane] = acc[c];
            }
        }
    }
    if (active) {
        int best;
        if (one_chunk) {
#pragma unroll
            for (int c = 0; c < CC; ++c)
                if (c < C) acc[c] = crf_energy(logp[base + (size_t)c * plane], acc[c], n_nb);
            best = crf_softmax_argmax<CC>(C, [&](int c) -> float& { return acc[c]; });
            if (q_dst) {
#pragma unroll
                for (int c = 0; c < CC; ++c)
                    if (c < C) q_dst[base + (size_t)c * plane] = acc[c];
            }
        } else {
            // the thread reads back what it wrote itself: program order, no fence
            for (int c = 0; c < C; ++c) {
                const size_t at = base + (size_t)c * plane;
                q_dst[at] = crf_energy(logp[at], q_dst[at], n_nb);
            }
            best = crf_softmax_argmax<0>(C, [&](int c) -> float& { return q_dst[base + (size_t)c * plane]; });
        }
        if (LAST) {
            const size_t idx = (size_t)n * plane + pix;
            if (pred_out) pred_out[idx] = (uint8_t)best;
            atomicAdd(&hist[C * C], 1u);
            if (best != (int)uarg[idx]) atomicAdd(&hist[C * C + 1], 1u);
            if (count) {
                const int tr = crf_label(labels, label_dtype, idx);
                if (tr != ignore_index && tr >= 0 && tr < C) atomicAdd(&hist[tr * C + best], 1u);
            }
        }
    }
    if (LAST) {
        __syncthreads();
        if (count) {
            for (int i = threadIdx.x; i < C * C; i += kCrfBlock) {
                const unsigned int val = hist[i];
                if (val) atomicAdd(&cm[i], (u64)val);
            }
        }
        if (threadIdx.x < 2) {
            const unsigned int val = hist[C * C + threadIdx.x];
            if (val) atomicAdd(&stats[threadIdx.x], (u64)val);
        }
    }
}

struct CrfIter {
    const float* q_src;
    float* q_dst;
};

template <int CC, bool LAST>
static int crf_launch_iter(const cms_crf_desc* d, const CrfGeom& g, const CrfTables& tab, int tiles_x, int tiles, size_t sample0,
                           const float* logp, const CrfIter& it, const uint8_t* uarg, hipStream_t s) {
    const int HP = (kCrfTileW + 2 * g.R) * (kCrfTileH + 2 * g.R);
    const size_t lds = ((size_t)(2 + CC) * HP + (LAST ? (size_t)g.C * g.C + 2 : 0)) * sizeof(float);
    auto kern = crf_meanfield_kernel<CC, LAST>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const size_t plane = (size_t)g.H * g.W, pix0 = sample0 * plane, el0 = pix0 * g.C;
    const void* labels = nullptr;
    if (d->labels) labels = (const uint8_t*)d->labels + pix0 * (d->label_dtype == CMS_LABEL_I64 ? 8 : 1);
    hipLaunchKernelGGL(kern, dim3(tiles, g.S * g.S, g.n), dim3(kCrfBlock), lds, s, g, tab, d->bi_w, crf_inv2b(d->bi_rgb), tiles_x,
                       d->rgb + pix0 * 3, logp + el0, it.q_src + el0, it.q_dst ? it.q_dst + el0 : nullptr, uarg + pix0, labels,
                       d->label_dtype, d->ignore_index, (u64*)d->cm, d->pred_out ? d->pred_out + pix0 : nullptr, (u64*)d->stats);
    return launch_status("cms_crf_refine (mean field)");
}

template <int CC>
static int crf_launch_cc(bool last, const cms_crf_desc* d, const CrfGeom& g, const CrfTables& tab, int tiles_x, int tiles,
                         size_t sample0, const float* logp, const CrfIter& it, const uint8_t* uarg, hipStream_t s) {
    return last ? crf_launch_iter<CC, true>(d, g, tab, tiles_x, tiles, sample0, logp, it, uarg, s)
                : crf_launch_iter<CC, false>(d, g, tab, tiles_x, tiles, sample0, logp, it, uarg, s);
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_crf_workspace_bytes(int n, int c, int H, int W) { return crf_workspace_bytes(n, c, H, W); }

extern "C" int cms_crf_refine(const cms_crf_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    const char* why = crf_check(d, workspace, workspace_bytes);
    CMS_REQUIRE(!why, "crf_refine: %s", why);
    hipStream_t s = (hipStream_t)stream;
    const int C = d->c;
    const size_t plane = (size_t)d->H * d->W, pix = (size_t)d->n * plane, fbytes = crf_align(pix * C * sizeof(float));
    uint8_t* ws = (uint8_t*)workspace;
    float* logp = (float*)ws;
    float* qa = (float*)(ws + fbytes);
    float* qb = (float*)(ws + 2 * fbytes);
    uint8_t* uarg = ws + 3 * fbytes;
    if (hipMemsetAsync(d->stats, 0, 2 * sizeof(int64_t), s) != hipSuccess) return launch_status("cms_crf_refine (memset)");
    CrfTables tab;
    crf_make_tables(d->radius, d->dilation, d->bi_xy, d->pos_w, d->pos_xy, &tab);
    const int cc = crf_chunk_for(C);
    const bool chunks = C > cc;
    for (int n0 = 0; n0 < d->n; n0 += kCrfGroup) {
        CrfGeom g;
        g.n = d->n - n0 < kCrfGroup ? d->n - n0 : kCrfGroup;
        g.C = C, g.H = d->H, g.W = d->W, g.R = d->radius, g.S = d->dilation;
        int hmax = 1, wmax = 1;
        for (int i = 0; i < kCrfGroup; ++i) {
            const bool on = i < g.n;
            const int32_t* r = d->rect + 4 * (size_t)(n0 + (on ? i : 0));
            g.rects.top[i] = on ? r[0] : 0, g.rects.left[i] = on ? r[1] : 0, g.rects.h[i] = on ? r[2] : 0, g.rects.w[i] = on ? r[3] : 0;
            if (on && r[2] > hmax) hmax = r[2];
            if (on && r[3] > wmax) wmax = r[3];
        }
        const size_t pix0 = (size_t)n0 * plane, el0 = pix0 * C;
        // ---- the unary launch over the group's canvas pixels
        cms_tta_desc td;
        for (int i = 0; i < CMS_TTA_MAX_VIEWS; ++i) {
            const bool on = i < d->k;
            td.logits[i] = on ? d->logits[i] + (size_t)n0 * C * d->h[i] * d->w[i] : nullptr;
            td.h[i] = on ? d->h[i] : 1, td.w[i] = on ? d->w[i] : 1, td.flip[i] = on ? d->flip[i] : 0;
        }
        td.n = g.n, td.c = C, td.H = d->H, td.W = d->W, td.k = d->k, td.align_corners = d->align_corners;
        TtaViews v;
        tta_make_views(&td, &v);
        const void* labels = nullptr;
        if (d->labels) labels = (const uint8_t*)d->labels + pix0 * (d->label_dtype == CMS_LABEL_I64 ? 8 : 1);
        const size_t lds = ((size_t)C * 256 + (size_t)C * C) * sizeof(float);
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void*)crf_unary_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(crf_unary_kernel, dim3(grid_for((size_t)g.n * plane, 256, 4096)), dim3(256), lds, s, v, d->k, g,
                           d->align_corners, labels, d->label_dtype, d->ignore_index, logp + el0, qa + el0, uarg + pix0, (u64*)d->cm,
                           d->pred_out ? d->pred_out + pix0 : nullptr, d->q_out ? d->q_out + el0 : nullptr);
        int rc = launch_status("cms_crf_refine (unary)");
        if (rc != CMS_OK) return rc;
        // ---- the iterations: the tiles of the largest sublattice (residue 0, 0) of the largest rectangle
        const int S = d->dilation;
        const int tiles_x = ((wmax + S - 1) / S + kCrfTileW - 1) / kCrfTileW, tiles_y = ((hmax + S - 1) / S + kCrfTileH - 1) / kCrfTileH;
        const int tiles = tiles_x * tiles_y;
        for (int t = 0; t < d->iters; ++t) {
            const bool last = t == d->iters - 1;
            CrfIter it;
            it.q_src = (t % 2 == 0) ? qa : qb;
            it.q_dst = (t % 2 == 0) ? qb : qa;
            if (last) it.q_dst = d->q_out ? d->q_out : (chunks ? it.q_dst : nullptr);
            switch (cc) {
                case 4: rc = crf_launch_cc<4>(last, d, g, tab, tiles_x, tiles, n0, logp, it, uarg, s); break;
                case 8: rc = crf_launch_cc<8>(last, d, g, tab, tiles_x, tiles, n0, logp, it, uarg, s); break;
                case 16: rc = crf_launch_cc<16>(last, d, g, tab, tiles_x, tiles, n0, logp, it, uarg, s); break;
                case 24: rc = crf_launch_cc<24>(last, d, g, tab, tiles_x, tiles, n0, logp, it, uarg, s); break;
                default: rc = crf_launch_cc<32>(last, d, g, tab, tiles_x, tiles, n0, logp, it, uarg, s); break;
            }
            if (rc != CMS_OK) return rc;
        }
    }
    return CMS_OK;
}
