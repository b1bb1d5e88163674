// The kernels of the masked consistency loss and their launches, written ONCE for the two ways of thresholding the teacher's
// confidence: one scalar (losses.hip, `TauThresh` below) or one threshold per class with the statistics a self-adaptive
// threshold is made from (cthresh.hip, `ClassThresh`). A kernel is `cons_*_kernel<P, ...>` with the threshold policy P:
//
//   P::Args                     the kernel argument block: ConsArgs, or a struct derived from it
//   P::on(a)                    whether there is a threshold at all (the scalar one is off with tau <= 0)
//   P::Fwd<CT, PPT2>(a)         per-kernel state of a forward or fused kernel (PPT2: at most two pixels per thread, the tiled
//   P::Bwd<CT>(a)               kernels), of a backward kernel. Constructed by every thread in front of the walk (the prologue:
//                               the per-class policy loads thr[] into LDS behind a barrier). Members:
//     pick(a, lt)               the threshold of a pixel from its teacher row `lt`: a value with passes(conf), the pass bit
//     pick_max(a, lt, mx)       the same with the row's maximum already known (backward state)
//     valid(a, px, n, y, x)     whether the pixel counts in the statistics                              }
//     count(a, lt, t, pass, valid)   the statistics of one pixel                                        } forward state
//     pixel_done(a) / finish(a)      after each pixel of the flat walk / behind the loss sums           }
//
// A policy that needs LDS declares it itself (ClassThresh: a `__shared__` of its state's accessor). The scalar policy has no
// storage at all, and these templates declare none for it: cons_fused_tiled_kernel<TauThresh, 21, VAR> sits at its 128-register
// bound and its allocation depends on the LDS layout of the module (profiles/loss_kernels_resources_refactor.md). The two policies
// are instantiated in their own translation units for the same reason.
//
// The order of operations on every value is part of the contract (profiles/cons_threshold_policy_refactor.md): the forward
// kernels pick the threshold after the loss, the fused compile-time kernel before it and counts behind it, and no kernel has an
// early-out on a zero factor (the masked-consistency backward always does its full work -- confidence rate 0 at
// random init, invalid pixels: a zero factor simply contributes zeros).
#pragma once
#include "cons_args.hpp"

namespace cms {

// ------------------------------------------------------------------------------------------------ the scalar policy
struct TauThresh {
    using Args = ConsArgs;
    static __device__ __forceinline__ bool on(const ConsArgs& a) { return a.tau > 0.0f; }
    // (tau is read from the argument block where it is compared, not copied per pixel: a copy changes the register allocation of
    // the fused kernels)
    struct Pick {
        const ConsArgs& a;
        __device__ __forceinline__ bool passes(float conf) const { return conf >= a.tau; }
    };
    struct State {
        __device__ __forceinline__ explicit State(const ConsArgs&) {}
        __device__ __forceinline__ bool valid(const ConsArgs&, const ConsPixel&, int, int, int) const { return true; }
        template <class LT>
        __device__ __forceinline__ Pick pick(const ConsArgs& a, const LT&) const { return Pick{a}; }
        template <class LT>
        __device__ __forceinline__ Pick pick_max(const ConsArgs& a, const LT&, float) const { return Pick{a}; }
        template <class LT>
        __device__ __forceinline__ void count(const ConsArgs&, const LT&, const Pick&, bool, bool) {}
        __device__ __forceinline__ void pixel_done(const ConsArgs&) {}
        __device__ __forceinline__ void finish(const ConsArgs&) {}
    };
    template <int CT, bool PPT2>
    using Fwd = State;
    template <int CT>
    using Bwd = State;
};

// ------------------------------------------------------------------------------------------------ forward
// one pixel of a forward kernel from its two gathers: the three loss sums (and the policy's statistics)
template <class P, int CT, bool IDENT, class St>
__device__ __forceinline__ void cons_fwd_pixel(const typename P::Args& a, St& st, const ConsPixel& px, bool valid, const Gather<IDENT>& gs,
                                               const Gather<IDENT>& gt, float (&acc)[3]) {
    const Geo& g = a.g;
    PixelFwd r;
    bool pass;
    if (CT > 0) {
        RegVec<CT> rs, rt;
        fill<CT, IDENT>(rs, gs);
        fill<CT, IDENT>(rt, gt);
        r = consistency_pixel_fwd<CT>(rs, rt, g.c, a.d.loss_fn, a.inv_root_c);
        const auto t = st.pick(a, rt);
        pass = P::on(a) && t.passes(r.conf);
        st.count(a, rt, t, pass, valid);
    } else {
        r = consistency_pixel_fwd<0>(gs, gt, g.c, a.d.loss_fn, a.inv_root_c);
        const auto t = st.pick(a, gt);
        pass = P::on(a) && t.passes(r.conf);
        st.count(a, gt, t, pass, valid);
    }
    const float lm = r.loss * px.um;
    const float cf = pass ? 1.0f : 0.0f;
    acc[0] += lm;
    acc[1] += lm * cf;
    acc[2] += cf;
}

template <class P, int CT>
__global__ __launch_bounds__(256) void cons_fwd_tiled_kernel(typename P::Args a, float* __restrict__ partials, int patch_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typename P::template Fwd<CT, true> st(a);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    fwd_tile_walk<false>(
        a.g, smem, [&](int n, const Patch& p, float* P_) { cons_stage(a, n, p, P_, patch_stride); },
        [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p) {
            const ConsPixel px = cons_pixel_inputs(a, n, y, x);
            const Gather<false> gs = gather_staged(smem, p, ty, tx);
            const Gather<false> gt = gather_staged(smem + (px.which ? 2 : 1) * patch_stride, p, ty, tx);
            cons_fwd_pixel<P, CT, false>(a, st, px, st.valid(a, px, n, y, x), gs, gt, acc);
        });
    __shared__ float red[3 * 16];
    store_partials<3>(acc, red, partials);
    st.finish(a);
}

template <class P, int CT, bool IDENT>
__global__ __launch_bounds__(256) void cons_fwd_kernel(typename P::Args a, float* __restrict__ partials) {
    const Geo& g = a.g;
    typename P::template Fwd<CT, false> st(a);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    pixel_walk(g, [&](size_t, int n, int y, int x) {
        const ConsPixel px = cons_pixel_inputs(a, n, y, x);
        const Gather<IDENT> gs = gather_at<IDENT>(a.d.l_stu + (size_t)n * g.c * ((size_t)g.h * g.w), g, y, x);
        Gather<IDENT> gt = gs;
        gt.base = px.tea;
        cons_fwd_pixel<P, CT, IDENT>(a, st, px, st.valid(a, px, n, y, x), gs, gt, acc);
        st.pixel_done(a);
    });
    __shared__ float red[3 * 16];
    store_partials<3>(acc, red, partials);
    st.finish(a);
}

// ------------------------------------------------------------------------------------------------ backward
// The gradient vector of a pixel is scaled by base_f or, where the per-pixel confidence gate (`pp`) fails, by zero. The run-time
// class count takes the teacher's maximum for the threshold from the softmax statistics it needs anyway. (The two kernels keep
// their own copy of these lines: behind a shared function the compiler schedules the scalar instances differently.)
//
// ---- identity geometry (h == H, w == W): gradients land directly on their own pixel
template <class P, int CT>
__global__ __launch_bounds__(256) void cons_bwd_ident_kernel(typename P::Args a, const float* __restrict__ scalars, float* __restrict__ grad) {
    const Geo& g = a.g;
    const typename P::template Bwd<CT> st(a);
    const size_t plane = (size_t)g.h * g.w;
    const float gscale = scalars[2];
    pixel_walk(g, [&](size_t, int n, int y, int x) {
        const ConsPixel px = cons_pixel_inputs(a, n, y, x);
        const Gather<true> gs = gather_at<true>(a.d.l_stu + (size_t)n * g.c * plane, g, y, x);
        Gather<true> gt = gs;
        gt.base = px.tea;
        float* gp = grad + (size_t)n * g.c * plane + gs.off;
        const float base_f = gscale * px.um;
        const bool pp = P::on(a) && a.d.conf_per_pixel;
        if (CT > 0) {
            RegVec<CT> rs, rt;
            fill<CT, true>(rs, gs);
            fill<CT, true>(rt, gt);
            float gv[CT > 0 ? CT : 1];
            const float conf = consistency_pixel_bwd<CT>(rs, rt, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { gv[k] = v; });
            const float f = (pp && !st.pick(a, rt).passes(conf)) ? 0.0f : base_f;
#pragma unroll
            for (int k = 0; k < CT; ++k) gp[k * plane] += f * gv[k];
        } else {
            float mt, zt;
            softmax_stats<0>(gt, g.c, mt, zt);
            const float conf = 1.0f / zt;
            const float f = (pp && !st.pick_max(a, gt, mt).passes(conf)) ? 0.0f : base_f;
            consistency_pixel_bwd<0>(gs, gt, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { gp[k * plane] += f * v; });
        }
    });
}

// ---- with upsampling: the LDS-tiled adjoint of the bilinear interpolation, tiled_scatter (loss_tiles.hpp)
template <class P, int CT>
__global__ __launch_bounds__(256) void cons_bwd_tiled_kernel(typename P::Args a, const float* __restrict__ scalars, float* __restrict__ grad,
                                                             int patch_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const typename P::template Bwd<CT> st(a);
    const Geo& g = a.g;
    const float gscale = scalars[2];
    const bool pp = P::on(a) && a.d.conf_per_pixel;
    // LDS copies of the tile's logit rectangles: student | teacher 0 | teacher 1, `pstride` floats apart
    const int pstride = patch_stride;
    auto stage = [&](int n, const Patch& p, float* P_) { cons_stage(a, n, p, P_, pstride); };
    auto pixel_grad = [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p, const float* P_, auto emit) -> bool {
        const ConsPixel px = cons_pixel_inputs(a, n, y, x);
        const float base_f = gscale * px.um;
        const Gather<false> gs = gather_staged(P_, p, ty, tx);       // (taps already rebased to the rectangle)
        const Gather<false> gt = gather_staged(P_ + (px.which ? 2 * pstride : pstride), p, ty, tx);
        if (CT > 0) {
            RegVec<CT> rs, rt;
            fill<CT, false>(rs, gs);
            fill<CT, false>(rt, gt);
            float gv[CT > 0 ? CT : 1];
            const float conf = consistency_pixel_bwd<CT>(rs, rt, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { gv[k] = v; });
            const float f = (pp && !st.pick(a, rt).passes(conf)) ? 0.0f : base_f;
#pragma unroll
            for (int k = 0; k < CT; ++k) emit(k, f * gv[k]);
        } else {
            float mt, zt;
            softmax_stats<0>(gt, g.c, mt, zt);
            const float conf = 1.0f / zt;
            const float f = (pp && !st.pick_max(a, gt, mt).passes(conf)) ? 0.0f : base_f;
            consistency_pixel_bwd<0>(gs, gt, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { emit(k, f * v); });
        }
        return true;
    };
    tiled_scatter(g, stage, pixel_grad, grad, smem);
}

// ---- forward + backward in ONE launch (round 6) -----------------------------------------------------------------------
// The backward kernel recomputes everything the forward kernel computed (the tile's logit rectangles, both softmaxes of every
// pixel) and needs from it only ONE scalar: the factor of the gradient. That factor is  ramp * weight / P * um  [* per-pixel
// confidence]  -- known up front -- times, in the default confidence mode, the scalar RATE (train_seg_semisup_mask_mt.py:415-418:
// the confidence mask is replaced by its mean), in which the gradient is LINEAR. So one pass computes the loss partial sums AND
// the gradient with the rate left out (`grad_unit` = ramp * weight / P), the finalising launch derives the scalars, and
// cms_scale_by_scalar multiplies the gradient rows by the rate afterwards (a 350 k-float pass). The chain between the forward and
// the backward pass of the step loses a launch of 0.10-0.12 ms and a second staging of all rectangles; under data parallelism
// the gradient no longer waits for the all-reduce of the confidence count either. Per-pixel values are those of the two
// kernels (same functions on the same registers).
template <class P, int CT, int LF>
__global__ __launch_bounds__(256, (LF >= 0 && CT > 0) ? 4 : 1) void cons_fused_tiled_kernel(typename P::Args a, float grad_unit,
                                                                                            float* __restrict__ grad, int patch_stride,
                                                                                            float* __restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typename P::template Fwd<CT, true> st(a);
    const Geo& g = a.g;
    const bool pp = P::on(a) && a.d.conf_per_pixel;
    const int pstride = patch_stride;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    auto stage = [&](int n, const Patch& p, float* P_) { cons_stage(a, n, p, P_, pstride); };
    auto pixel_grad = [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p, const float* P_, auto emit) -> bool {
        const ConsPixel px = cons_pixel_inputs(a, n, y, x);
        const bool valid = st.valid(a, px, n, y, x);
        const float base_f = grad_unit * px.um;
        const Gather<false> gs = gather_staged(P_, p, ty, tx);       // (taps already rebased to the rectangle)
        const Gather<false> gt = gather_staged(P_ + (px.which ? 2 * pstride : pstride), p, ty, tx);
        PixelFwd r;
        bool pass;
        if (CT > 0) {
            RegVec<CT> rs, rt;
            fill<CT, false>(rs, gs);
            fill<CT, false>(rt, gt);
            const auto t = st.pick(a, rt);
            r = consistency_pixel_fwd_bwd<(CT > 0 ? CT : 1), LF>(
                rs, rt, a.d.loss_fn, a.inv_root_c, [&](float conf) -> float { return (pp && !t.passes(conf)) ? 0.0f : base_f; },
                [&](int k, float v) { emit(k, v); });
            pass = P::on(a) && t.passes(r.conf);
            st.count(a, rt, t, pass, valid);
        } else {
            r = consistency_pixel_fwd<0>(gs, gt, g.c, a.d.loss_fn, a.inv_root_c);
            const auto t = st.pick(a, gt);
            const float f = (pp && !t.passes(r.conf)) ? 0.0f : base_f;
            consistency_pixel_bwd<0>(gs, gt, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { emit(k, f * v); });
            pass = P::on(a) && t.passes(r.conf);
            st.count(a, gt, t, pass, valid);
        }
        const float lm = r.loss * px.um;
        const float cf = pass ? 1.0f : 0.0f;
        acc[0] += lm;
        acc[1] += lm * cf;
        acc[2] += cf;
        return true;
    };
    tiled_scatter(g, stage, pixel_grad, grad, smem);
    __shared__ float red[3 * 16];
    store_partials<3>(acc, red, partials);
    st.finish(a);
}

// ------------------------------------------------------------------------------------------------ host side
// The three launches of a policy's kernel set on its checked argument block; the callers are the extern "C" entry points.
template <class P>
inline void cons_launch_fwd(const typename P::Args& a, float* workspace, double* stats_out, hipStream_t s) {
    const FwdPlan p = fwd_plan(a.g, 3);
    CMS_DISPATCH_C(a.g.c, launch_fwd<3>(cons_fwd_tiled_kernel<P, CT>, cons_fwd_kernel<P, CT, true>, cons_fwd_kernel<P, CT, false>, a, p,
                                        workspace, stats_out, (double)((size_t)a.g.n * a.g.H * a.g.W), 3, s, p.pstride));
}

// (`what` names the entry point in the refusal of a geometry whose tiles do not fit the LDS)
template <class P>
inline int cons_launch_bwd(const char* what, const typename P::Args& a, const float* scalars, float* grad, hipStream_t s) {
    const int pstride = (int)patch_floats(a.g.c, a.g.sy, a.g.sx, TILE_H);
    int rc = CMS_OK;
    CMS_DISPATCH_C(a.g.c, rc = launch_bwd(what, cons_bwd_ident_kernel<P, CT>, cons_bwd_tiled_kernel<P, CT>, a, 3, 0, scalars, grad, s, pstride));
    return rc;
}

// the fused kernel of this class count and loss function: the default loss (`var`) as a compile-time constant has its own
// register allocation (see consistency_pixel_fwd_bwd)
template <class P, int CT>
inline auto cons_fused_kernel(int loss_fn) {
    return loss_fn == CMS_LOSS_VAR ? cons_fused_tiled_kernel<P, CT, LOSS_VAR> : cons_fused_tiled_kernel<P, CT, -1>;
}

template <class P>
inline void cons_launch_fused(const typename P::Args& a, int tiles, float grad_unit, float* workspace, double* stats_out, float* grad,
                              hipStream_t s) {
    const int pstride = (int)patch_floats(a.g.c, a.g.sy, a.g.sx, TILE_H);
    CMS_DISPATCH_C(a.g.c, launch_fused<3>(cons_fused_kernel<P, CT>(a.d.loss_fn), tiles, tile_lds_bytes(a.g.c, a.g.sy, a.g.sx, 3), s, workspace,
                                          stats_out, (double)((size_t)a.g.n * a.g.H * a.g.W), 3, a, grad_unit, grad, pstride));
}

}  // namespace cms
