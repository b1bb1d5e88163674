// Calibration and pseudo-label quality (gfx950): the vote kernel of csrc/tta.hip with the confidence kept. csrc/tta.hip holds the
// vote's scores in LDS only long enough to take the argmax; here the same walk -- a thread owns an output pixel, grid-stride, the
// score column of k >= 2 views in LDS [C][256] -- also bins the confidence of every scored pixel and adds what the report needs into
// the workgroup's tables in LDS: per (predicted class, bin) the pixels and the correct pixels as 32-bit counts and the fixed-point
// confidence sum as a 64-bit one, the C x C matrix, and per thread in registers the fixed-point Brier and NLL sums. The tables leave
// with one 64-bit global atomic per non-empty cell (csrc/eval.hip's flush). Written with tensor operations the same report
// materialises K tensors of (N, C, H, W) probabilities. One launch takes the place of the vote launch. The arithmetic is
// csrc/calib_math.hpp's; all sums are of integers, so the same input gives the same bits.
#include "common.hpp"
#include "calib_math.hpp"

namespace cms {

// MODE 0: one view of the output's size (no interpolation), 1: one view, resampled, 2: the vote over k >= 2 views
template <int MODE>
__global__ __launch_bounds__(kCalibBlock) void calib_kernel(const TtaViews v, const CalibParams prm, int k, const void* labels,
                                                            int label_dtype, int ignore_index, int N, int C, int H, int W, int align,
                                                            unsigned long long* __restrict__ hist,
                                                            unsigned long long* __restrict__ scores,
                                                            unsigned long long* __restrict__ cm, uint8_t* __restrict__ pred_out) {
    extern __shared__ __attribute__((aligned(16))) float calib_smem[];
    const int nb = prm.nb, cells = C * nb;
    float* score = calib_smem;                                                            // MODE 2: [C][kCalibBlock]
    unsigned long long* conf_fx = reinterpret_cast<unsigned long long*>(calib_smem + (MODE == 2 ? C * kCalibBlock : 0));   // [C][nb]
    unsigned long long* tot = conf_fx + cells;                                            // [kCalibScores]
    unsigned int* cnt = reinterpret_cast<unsigned int*>(tot + kCalibScores);              // [C][nb]
    unsigned int* hit = cnt + cells;                                                      // [C][nb]
    unsigned int* mat = hit + cells;                                                      // [C][C]
    for (int i = threadIdx.x; i < cells; i += kCalibBlock) conf_fx[i] = 0ull, cnt[i] = 0u, hit[i] = 0u;
    for (int i = threadIdx.x; i < C * C; i += kCalibBlock) mat[i] = 0u;
    if (threadIdx.x < kCalibScores) tot[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long n_scored = 0ull, brier = 0ull, nll[CMS_CALIB_MAX_TEMPS];
#pragma unroll
    for (int t = 0; t < CMS_CALIB_MAX_TEMPS; ++t) nll[t] = 0ull;
    const size_t P = (size_t)N * H * W;
    for (size_t idx = (size_t)blockIdx.x * kCalibBlock + threadIdx.x; idx < P; idx += (size_t)gridDim.x * kCalibBlock) {
        const int x = (int)(idx % W);
        const size_t t_ = idx / W;
        const int y = (int)(t_ % H);
        const int n = (int)(t_ / H);
        const int label = calib_valid_label(tta_label(labels, label_dtype, idx), ignore_index, C);
        CalibPixel px;
        float px_nll[CMS_CALIB_MAX_TEMPS];
        if (MODE == 2) {
            calib_vote_pixel(v, k, n, C, y, x, align != 0, label, prm, [&](int c) -> float& { return score[c * kCalibBlock + threadIdx.x]; },
                             px, px_nll);
        } else {
            calib_single_pixel<MODE == 0>(v, n, C, y, x, align != 0, label, prm, px, px_nll);
        }
        if (pred_out) pred_out[idx] = (uint8_t)px.pred;
        if (label < 0) continue;
        const int cell = px.pred * nb + calib_bin(prm, px.conf);                          // pred < C, bin < nb: inside the tables
        atomicAdd(&cnt[cell], 1u);
        if (px.pred == label) atomicAdd(&hit[cell], 1u);
        atomicAdd(&conf_fx[cell], calib_fx(px.conf, kCalibConfScale, 1.0f));
        if (cm) atomicAdd(&mat[label * C + px.pred], 1u);
        n_scored += 1ull;
        brier += calib_fx(px.brier, kCalibBrierScale, 2.0f);
#pragma unroll
        for (int t = 0; t < CMS_CALIB_MAX_TEMPS; ++t)
            if (t < prm.nt) nll[t] += calib_fx(px_nll[t], kCalibNllScale, kCalibNllCap);
    }
    if (n_scored) {
        atomicAdd(&tot[0], n_scored);
        atomicAdd(&tot[1], brier);
#pragma unroll
        for (int t = 0; t < CMS_CALIB_MAX_TEMPS; ++t)
            if (t < prm.nt) atomicAdd(&tot[2 + t], nll[t]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kCalibBlock) {
        const unsigned int a = cnt[i];
        if (a) {
            atomicAdd(&hist[3 * i], (unsigned long long)a);
            const unsigned int b = hit[i];
            if (b) atomicAdd(&hist[3 * i + 1], (unsigned long long)b);
            const unsigned long long f = conf_fx[i];
            if (f) atomicAdd(&hist[3 * i + 2], f);
        }
    }
    if (cm) {
        for (int i = threadIdx.x; i < C * C; i += kCalibBlock) {
            const unsigned int val = mat[i];
            if (val) atomicAdd(&cm[i], (unsigned long long)val);
        }
    }
    if (threadIdx.x < 2 + prm.nt) {
        const unsigned long long val = tot[threadIdx.x];
        if (val) atomicAdd(&scores[threadIdx.x], val);
    }
}

}  // namespace cms

using namespace cms;

template <int MODE>
static int calib_launch(const cms_calib_desc* d, const TtaViews& v, const CalibParams& prm, hipStream_t s) {
    const size_t P = (size_t)d->n * d->H * d->W;
    const size_t lds = calib_lds_bytes(d->c, d->nb, d->k);
    auto kern = calib_kernel<MODE>;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid_for(P, kCalibBlock, 1024)), dim3(kCalibBlock), lds, s, v, prm, d->k, d->labels, d->label_dtype,
                       d->ignore_index, d->n, d->c, d->H, d->W, d->align_corners, (unsigned long long*)d->hist,
                       (unsigned long long*)d->scores, (unsigned long long*)d->cm, d->pred_out);
    return launch_status("cms_calib_accumulate");
}

extern "C" int cms_calib_accumulate(const cms_calib_desc* d, void* stream) {
    const char* why = calib_check(d);
    CMS_REQUIRE(!why, "calib_accumulate: %s", why);
    cms_tta_desc td;
    calib_tta_desc(d, &td);
    TtaViews v;
    tta_make_views(&td, &v);
    CalibParams prm;
    calib_make_params(d, &prm);
    hipStream_t s = (hipStream_t)stream;
    if (d->k >= 2) return calib_launch<2>(d, v, prm, s);
    if (d->h[0] == d->H && d->w[0] == d->W) return calib_launch<0>(d, v, prm, s);
    return calib_launch<1>(d, v, prm, s);
}
