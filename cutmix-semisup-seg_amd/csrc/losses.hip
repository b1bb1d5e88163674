// Fused loss kernels of the CutMix mean-teacher step (gfx950).
//
//   consistency:  bilinear upsample of low-res logits + paste of the two teacher predictions with the box mask
//                 (rasterised in-kernel) + softmax x2 + confidence threshold + one of five per-pixel losses +
//                 masked mean, forward and backward.           train_seg_semisup_mask_mt.py:363-367, 407-459
//   supervised:   bilinear upsample + log-softmax + NLL(ignore_index), forward and backward.    :126, 299-301
//
// Design (MI355X-first): the (N,C,H,W) full-resolution logits / probabilities / per-pixel loss maps of the
// reference (12+ elementwise kernels and their autograd twins, (5C+4)*P*4 bytes of HBM traffic) are never
// materialised. One thread owns one output pixel, lanes of a wave are consecutive x so the hi-res validity masks
// are read fully coalesced, the low-res logits (a few MB, L2-resident) are gathered with the 4 bilinear taps, the
// class axis lives in registers (compile-time C for 2/5/19/21) so the channel reductions need no cross-lane
// traffic; the only cross-lane work is the wave-shuffle + LDS block reduction of the three loss sums.
// Backward: the per-pixel gradient vector is scattered to the low-res logits through an LDS-tiled separable
// adjoint of the bilinear upsample (x-reduce, then y-reduce, fixed order inside a tile), so global atomics are
// issued per low-res cell per tile instead of per pixel per tap.
//
// The tile walks, the tiled adjoint and the launch paths are csrc/loss_tiles.hpp, shared with the ICT loss (ict.hip) and the
// augmentation consistency (aug_loss.hip); this file also holds the one definition of the switch state they read. The
// consistency kernels and their launches are the templates of csrc/cons_kernels.hpp, instantiated here with the scalar threshold
// (TauThresh) and in cthresh.hip with per-class thresholds: one body for both.
#include "cons_kernels.hpp"

namespace cms {

// ------------------------------------------------------------------------------------------------ consistency
// (the forward, backward and fused kernels: cons_kernels.hpp)
__global__ void cons_finalize_kernel(const double* __restrict__ sl, const double* __restrict__ sg, float tau,
                                     int per_pixel, float ramp, float weight, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double Pl = sl[3];
    double closs, gs, rate;
    if (tau > 0.0f) {
        rate = sg[2] / sg[3];
        if (per_pixel) {
            closs = sl[1] / Pl;
            gs = 1.0 / Pl;
        } else {
            // default mode: the confidence mask is replaced by its scalar mean (:415-418)
            closs = rate * (sl[0] / Pl);
            gs = rate / Pl;
        }
    } else {
        rate = NAN;
        closs = sl[0] / Pl;
        gs = 1.0 / Pl;
    }
    closs *= (double)ramp;                      // :454-455
    out[0] = (float)closs;                      // logged value, :461
    out[1] = (float)rate;                       // :413
    out[2] = (float)(gs * (double)ramp * (double)weight);
    out[3] = (float)(closs * (double)weight);   // :458
}

// x[i] *= scalars[idx] * factor for i < n (the deferred factor of the fused loss launches: a device scalar)
__global__ __launch_bounds__(256) void scale_by_scalar_kernel(float* __restrict__ x, size_t n, const float* __restrict__ scalars,
                                                              int idx, float factor) {
    const float f = scalars[idx] * factor;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] *= f;
}

// ------------------------------------------------------------------------------------------------ cross entropy
struct CeArgs {
    cms_ce_desc d;
    Geo g;
};

__device__ __forceinline__ int load_label(const CeArgs& a, size_t pix) {
    if (a.d.label_dtype == CMS_LABEL_U8) return (int)((const uint8_t*)a.d.labels)[pix];
    const int64_t v = ((const int64_t*)a.d.labels)[pix];
    return (v < 0 || v > 0x7fffffff) ? -1 : (int)v;
}

__device__ __forceinline__ bool ce_ignored(const CeArgs& a, int label) {
    return label == a.d.ignore_index || label < 0 || label >= a.g.c;
}

__device__ __forceinline__ void ce_stage(const CeArgs& a, int n, const Patch& p, float* P) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w;
    stage_patch(P, a.d.logits + (size_t)n * g.c * plane, g.c, plane, g.w, p);
}

// one valid pixel of a forward kernel from its gather: the two loss sums
template <int CT, bool IDENT>
__device__ __forceinline__ void ce_fwd_pixel(const CeArgs& a, const Gather<IDENT>& gl, int label, float (&acc)[2]) {
    float v;
    if (CT > 0) {
        RegVec<CT> r;
        fill<CT, IDENT>(r, gl);
        float mx, z;
        softmax_stats<CT>(r, a.g.c, mx, z);
        v = -((gl(label) - mx) - logf(z));   // label is a run-time index: re-gather instead of indexing registers
    } else {
        v = ce_pixel_fwd<0>(gl, a.g.c, label);
    }
    acc[0] += v;
    acc[1] += 1.0f;
}

template <int CT, bool IDENT>
__global__ __launch_bounds__(256) void ce_fwd_kernel(CeArgs a, float* __restrict__ partials) {
    const Geo& g = a.g;
    float acc[2] = {0.0f, 0.0f};
    pixel_walk(g, [&](size_t pix, int n, int y, int x) {
        const int label = load_label(a, pix);
        if (ce_ignored(a, label)) return;
        ce_fwd_pixel<CT, IDENT>(a, gather_at<IDENT>(a.d.logits + (size_t)n * g.c * ((size_t)g.h * g.w), g, y, x), label, acc);
    });
    __shared__ float red[2 * 16];
    store_partials<2>(acc, red, partials);
}

template <int CT>
__global__ __launch_bounds__(256) void ce_fwd_tiled_kernel(CeArgs a, float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Geo& g = a.g;
    float acc[2] = {0.0f, 0.0f};
    fwd_tile_walk<true>(
        g, smem, [&](int n, const Patch& p, float* P) { ce_stage(a, n, p, P); },
        [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p) {
            const int label = load_label(a, ((size_t)n * g.H + y) * g.W + x);
            if (ce_ignored(a, label)) return;
            ce_fwd_pixel<CT, false>(a, gather_staged(smem, p, ty, tx), label, acc);
        });
    __shared__ float red[2 * 16];
    store_partials<2>(acc, red, partials);
}

__global__ void ce_finalize_kernel(const double* __restrict__ stats, float weight, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = (float)(stats[0] / stats[1]);         // 0 / 0 = NaN when every label is ignored, as nn.CrossEntropyLoss gives
    // the gradient factor: with no valid pixel no row received a gradient, and the factor is 0 rather than weight / 0 = inf --
    // cms_scale_by_scalar behind the one-launch path would turn its all-zero rows into 0 * inf = NaN, where the forward /
    // backward launch pair (which skips ignored pixels) and torch leave them zero
    out[1] = stats[1] > 0.0 ? (float)((double)weight / stats[1]) : 0.0f;
}

template <int CT>
__global__ __launch_bounds__(256) void ce_bwd_ident_kernel(CeArgs a, const float* __restrict__ scalars,
                                                           float* __restrict__ grad) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w;
    const float gscale = scalars[1];
    pixel_walk(g, [&](size_t pix, int n, int y, int x) {
        const int label = load_label(a, pix);
        if (ce_ignored(a, label)) return;
        const Gather<true> gl = gather_at<true>(a.d.logits + (size_t)n * g.c * plane, g, y, x);
        float* gp = grad + (size_t)n * g.c * plane + gl.off;
        if (CT > 0) {
            RegVec<CT> r;
            fill<CT, true>(r, gl);
            ce_pixel_bwd<CT>(r, g.c, label, [&](int k, float v) { gp[k * plane] += gscale * v; });
        } else {
            ce_pixel_bwd<0>(gl, g.c, label, [&](int k, float v) { gp[k * plane] += gscale * v; });
        }
    });
}

template <int CT>
__global__ __launch_bounds__(256) void ce_bwd_tiled_kernel(CeArgs a, const float* __restrict__ scalars,
                                                           float* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Geo& g = a.g;
    const float gscale = scalars[1];
    auto stage = [&](int n, const Patch& p, float* P) { ce_stage(a, n, p, P); };
    auto pixel_grad = [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p, const float* P, auto emit) -> bool {
        const size_t pix = ((size_t)n * g.H + y) * g.W + x;
        const int label = load_label(a, pix);
        if (ce_ignored(a, label)) return false;
        const Gather<false> gl = gather_staged(P, p, ty, tx);       // (taps already rebased to the rectangle)
        if (CT > 0) {
            RegVec<CT> r;
            fill<CT, false>(r, gl);
            ce_pixel_bwd<CT>(r, g.c, label, [&](int k, float v) { emit(k, gscale * v); });
        } else {
            ce_pixel_bwd<0>(gl, g.c, label, [&](int k, float v) { emit(k, gscale * v); });
        }
        return true;
    };
    tiled_scatter(g, stage, pixel_grad, grad, smem);
}

// forward + backward of the cross entropy in one launch (round 6): the gradient is (softmax - onehot) * weight / n_valid, linear
// in the one scalar the forward pass contributes (the count of valid labels, global under data parallelism) -- computed here
// with that factor left out, scaled by cms_scale_by_scalar behind cms_ce_finalize.
template <int CT>
__global__ __launch_bounds__(256) void ce_fused_tiled_kernel(CeArgs a, float* __restrict__ grad, float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Geo& g = a.g;
    float acc[2] = {0.0f, 0.0f};
    auto stage = [&](int n, const Patch& p, float* P) { ce_stage(a, n, p, P); };
    auto pixel_grad = [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p, const float* P, auto emit) -> bool {
        const size_t pix = ((size_t)n * g.H + y) * g.W + x;
        const int label = load_label(a, pix);
        if (ce_ignored(a, label)) return false;
        const Gather<false> gl = gather_staged(P, p, ty, tx);       // (taps already rebased to the rectangle)
        float v;
        if (CT > 0) {
            RegVec<CT> r;
            fill<CT, false>(r, gl);
            // (the label is a run-time index: its logit is re-gathered instead of indexing registers, as in ce_fwd_tiled_kernel)
            v = ce_pixel_fwd_bwd<(CT > 0 ? CT : 1)>(r, gl(label), label, [&](int k, float gv) { emit(k, gv); });
        } else {
            v = ce_pixel_fwd<0>(gl, g.c, label);
            ce_pixel_bwd<0>(gl, g.c, label, [&](int k, float gv) { emit(k, gv); });
        }
        acc[0] += v;
        acc[1] += 1.0f;
        return true;
    };
    tiled_scatter(g, stage, pixel_grad, grad, smem);
    __shared__ float red[2 * 16];
    store_partials<2>(acc, red, partials);
}

// ------------------------------------------------------------------------------------------------ switch state
// Run-to-run reproducible backward of the two losses (cms_loss_set_deterministic / CMS_LOSS_DETERMINISTIC=1): the tiles go
// out as colour classes (below). Off (the throughput default, like the fp32 atomics of the weight gradients): ALL tiles in one
// launch -- tiles that share a low-resolution cell then add into it in a run-dependent order (fp32 atomics, ~1e-7), and the
// launch has four times the workgroups of a colour class: the four launches of a class each kept < 1 round of the machine
// busy and sat on the critical path between the forward and the backward pass (4 x 45-65 us per loss at 321 x 321).
static int g_loss_deterministic = -1;
bool loss_deterministic() {
    if (g_loss_deterministic < 0) {
        const char* e = getenv("CMS_LOSS_DETERMINISTIC");
        g_loss_deterministic = e ? (atoi(e) != 0) : 0;
    }
    return g_loss_deterministic != 0;
}

// the LDS-staged forward kernels: one workgroup per 64 x 8 tile of one sample (0 = use the direct-gather kernels: identity
// geometry, or rectangles beyond FWD_PATCH_LDS_MAX)
int fwd_tiles(const Geo& g, int n_patches, size_t* lds_out, int* stride_out) {
    if (is_ident(g)) return 0;
    static int on = -1;
    if (on < 0) {
        const char* e = getenv("CMS_LOSS_FWD_TILED");     // A/B switch, read once
        on = e ? (atoi(e) != 0) : 1;
    }
    if (!on) return 0;
    const size_t pf = patch_floats(g.c, g.sy, g.sx, FWD_TILE_H);
    const size_t lds = pf * n_patches * sizeof(float);
    if (lds > FWD_PATCH_LDS_MAX) return 0;
    if (lds_out) *lds_out = lds;
    if (stride_out) *stride_out = (int)pf;
    return ((g.W + TILE_W - 1) / TILE_W) * ((g.H + FWD_TILE_H - 1) / FWD_TILE_H) * g.n;
}

// the fused forward + backward launches: one workgroup per 64 x TILE_H tile of one sample, all tiles in ONE launch (0 = not
// available: identity geometry, rectangles beyond the LDS, or the deterministic mode, whose colour-class launches stay unfused)
int fused_tiles(const Geo& g, int n_patches) {
    if (is_ident(g)) return 0;
    if (loss_deterministic()) return 0;
    static int on = -1;
    if (on < 0) {
        const char* e = getenv("CMS_LOSS_FUSED");         // A/B switch, read once
        on = e ? (atoi(e) != 0) : 1;
    }
    if (!on) return 0;
    if (tile_lds_bytes(g.c, g.sy, g.sx, n_patches) > TILE_LDS_MAX) return 0;
    return ((g.W + TILE_W - 1) / TILE_W) * ((g.H + TILE_H - 1) / TILE_H) * g.n;
}

// ------------------------------------------------------------------------------------------------ host side
int check_cons(const cms_consistency_desc* d) {
    CMS_REQUIRE(d != nullptr, "consistency: null descriptor");
    CMS_REQUIRE(d->l_stu && d->l_tea0, "consistency: l_stu / l_tea0 must not be NULL");
    CMS_REQUIRE(d->mode == CMS_MODE_MIX || d->mode == CMS_MODE_CUT, "consistency: unknown mode %d", d->mode);
    CMS_REQUIRE(d->mode != CMS_MODE_MIX || d->l_tea1, "consistency: mix mode needs l_tea1");
    CMS_REQUIRE((d->ranges != nullptr) != (d->mask != nullptr), "consistency: give exactly one of ranges / mask");
    CMS_REQUIRE(d->ranges == nullptr || d->n_boxes >= 0, "consistency: n_boxes < 0");
    int rc = check_geometry(d, "consistency");
    return rc ? rc : check_loss_fn(d);
}

ConsArgs make_cons_args(const cms_consistency_desc* d) {
    ConsArgs a;
    a.d = *d;
    a.g = geo_of(d);
    a.tau = d->conf_thresh;
    a.inv_root_c = (float)(1.0 / sqrt((double)d->c));
    return a;
}

static int check_ce(const cms_ce_desc* d) {
    CMS_REQUIRE(d != nullptr, "ce: null descriptor");
    CMS_REQUIRE(d->logits && d->labels, "ce: logits / labels NULL");
    CMS_REQUIRE(d->label_dtype == CMS_LABEL_U8 || d->label_dtype == CMS_LABEL_I64, "ce: bad label dtype");
    return check_geometry(d, "ce", "label");
}

static CeArgs make_ce_args(const cms_ce_desc* d) {
    CeArgs a;
    a.d = *d;
    a.g = geo_of(d);
    return a;
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_consistency_workspace_bytes(const cms_consistency_desc* d) {
    if (!d) return 0;
    const Geo g = geo_of(d);
    return (size_t)std::max(fwd_blocks(g, 3), fused_tiles(g, 3)) * 3 * sizeof(float);
}

extern "C" int cms_consistency_fused_supported(const cms_consistency_desc* d) {
    if (check_cons(d)) return 0;
    return fused_tiles(geo_of(d), 3) > 0 ? 1 : 0;
}

extern "C" int cms_consistency_fwd_bwd(const cms_consistency_desc* d, float grad_unit, void* workspace, double* stats_out,
                                       float* grad_l_stu, void* stream) {
    int rc = check_cons(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out && grad_l_stu, "consistency_fwd_bwd: workspace / stats_out / grad NULL");
    const ConsArgs a = make_cons_args(d);
    const int tiles = fused_tiles(a.g, 3);
    CMS_REQUIRE(tiles > 0, "consistency_fwd_bwd: not available for this geometry / mode (ask cms_consistency_fused_supported)");
    cons_launch_fused<TauThresh>(a, tiles, grad_unit, (float*)workspace, stats_out, grad_l_stu, (hipStream_t)stream);
    return launch_status("cms_consistency_fwd_bwd");
}

extern "C" int cms_scale_by_scalar(float* x, long long n, const float* scalars, int index, float factor, void* stream) {
    CMS_REQUIRE(x && scalars && n >= 0 && index >= 0, "scale_by_scalar: bad argument");
    if (n == 0) return CMS_OK;
    const int grid = (int)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(scale_by_scalar_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (size_t)n, scalars, index, factor);
    return launch_status("cms_scale_by_scalar");
}

extern "C" int cms_consistency_fwd(const cms_consistency_desc* d, void* workspace, double* stats_out, void* stream) {
    int rc = check_cons(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out, "consistency_fwd: workspace / stats_out NULL");
    cons_launch_fwd<TauThresh>(make_cons_args(d), (float*)workspace, stats_out, (hipStream_t)stream);
    return launch_status("cms_consistency_fwd");
}

extern "C" int cms_consistency_finalize(const double* stats_local, const double* stats_global, float conf_thresh,
                                        int conf_per_pixel, float ramp_val, float cons_weight, float* scalars_out,
                                        void* stream) {
    CMS_REQUIRE(stats_local && stats_global && scalars_out, "consistency_finalize: NULL argument");
    hipLaunchKernelGGL(cons_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats_local, stats_global,
                       conf_thresh, conf_per_pixel, ramp_val, cons_weight, scalars_out);
    return launch_status("cms_consistency_finalize");
}

extern "C" int cms_loss_set_deterministic(int on) {
    cms::g_loss_deterministic = on ? 1 : 0;
    return CMS_OK;
}

extern "C" int cms_consistency_bwd(const cms_consistency_desc* d, const float* scalars, float* grad_l_stu,
                                   void* stream) {
    int rc = check_cons(d);
    if (rc) return rc;
    CMS_REQUIRE(scalars && grad_l_stu, "consistency_bwd: scalars / grad NULL");
    rc = cons_launch_bwd<TauThresh>("consistency_bwd", make_cons_args(d), scalars, grad_l_stu, (hipStream_t)stream);
    return rc ? rc : launch_status("cms_consistency_bwd");
}

extern "C" size_t cms_ce_workspace_bytes(const cms_ce_desc* d) {
    if (!d) return 0;
    const Geo g = geo_of(d);
    return (size_t)std::max(fwd_blocks(g, 1), fused_tiles(g, 1)) * 2 * sizeof(float);
}

extern "C" int cms_ce_fused_supported(const cms_ce_desc* d) {
    if (check_ce(d)) return 0;
    return fused_tiles(geo_of(d), 1) > 0 ? 1 : 0;
}

extern "C" int cms_ce_fwd_bwd(const cms_ce_desc* d, void* workspace, double* stats_out, float* grad_logits, void* stream) {
    int rc = check_ce(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out && grad_logits, "ce_fwd_bwd: workspace / stats_out / grad NULL");
    const CeArgs a = make_ce_args(d);
    const int tiles = fused_tiles(a.g, 1);
    CMS_REQUIRE(tiles > 0, "ce_fwd_bwd: not available for this geometry / mode (ask cms_ce_fused_supported)");
    CMS_DISPATCH_C(d->c, launch_fused<2>(ce_fused_tiled_kernel<CT>, tiles, tile_lds_bytes(d->c, a.g.sy, a.g.sx, 1), (hipStream_t)stream,
                                         (float*)workspace, stats_out, 0.0, -1, a, grad_logits));
    return launch_status("cms_ce_fwd_bwd");
}

extern "C" int cms_ce_fwd(const cms_ce_desc* d, void* workspace, double* stats_out, void* stream) {
    int rc = check_ce(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out, "ce_fwd: workspace / stats_out NULL");
    const CeArgs a = make_ce_args(d);
    const FwdPlan p = fwd_plan(a.g, 1);
    CMS_DISPATCH_C(d->c, launch_fwd<2>(ce_fwd_tiled_kernel<CT>, ce_fwd_kernel<CT, true>, ce_fwd_kernel<CT, false>, a, p,
                                       (float*)workspace, stats_out, 0.0, -1, (hipStream_t)stream));
    return launch_status("cms_ce_fwd");
}

extern "C" int cms_ce_finalize(const double* stats, float loss_weight, float* scalars_out, void* stream) {
    CMS_REQUIRE(stats && scalars_out, "ce_finalize: NULL argument");
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, loss_weight, scalars_out);
    return launch_status("cms_ce_finalize");
}

extern "C" int cms_ce_bwd(const cms_ce_desc* d, const float* scalars, float* grad_logits, void* stream) {
    int rc = check_ce(d);
    if (rc) return rc;
    CMS_REQUIRE(scalars && grad_logits, "ce_bwd: scalars / grad NULL");
    const CeArgs a = make_ce_args(d);
    CMS_DISPATCH_C(d->c, rc = launch_bwd("ce_bwd", ce_bwd_ident_kernel<CT>, ce_bwd_tiled_kernel<CT>, a, 1, 0, scalars, grad_logits,
                                         (hipStream_t)stream));
    return rc ? rc : launch_status("cms_ce_bwd");
}
