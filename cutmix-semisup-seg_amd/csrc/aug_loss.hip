// Augmentation consistency loss (gfx950)
// The classic mean teacher between two augmented views (train_seg_semisup_aug_mt.py:302-390): the teacher's prediction of view 0
// is warped into the student's view 1 with the four taps of F.grid_sample, per pixel, and never becomes a tensor. Same kernel
// shapes as the other loss families (one thread per output pixel, 64 x 8 forward and 64 x 4 backward tiles, the student's rectangle staged
// to LDS, class axis in registers, the tiled adjoint of the student's upsample for the backward); the per-pixel arithmetic is
// csrc/aug_math.hpp. What is new is the TEACHER's rectangle: a tile samples a parallelogram of the teacher's map. Every workgroup
// maps its tile's corners (aug_tile_box), converts the padded, clipped bounding box to low-resolution cells and stages it if it
// fits `tea_cap` floats (uniform over the workgroup); otherwise, and for any tap whose cells are not all inside the staged
// rectangle, the taps are gathered from global memory (L2-resident). Both routes run bilin_gather on the same values: the results
// are bit-identical, and there is never an LDS index outside the staged region.
// Compulsory traffic per launch: two low-resolution logit tensors, um1 once (coalesced) and um0 at four taps per pixel.
// The tile walks, the tiled adjoint and the launch paths are csrc/loss_tiles.hpp, shared with losses.hip and ict.hip.
#include "loss_tiles.hpp"
#include "aug_math.hpp"

namespace cms {

constexpr size_t AUG_TEA_LDS_MAX = 32 * 1024;       // LDS for the teacher's rectangle, at most (keeps 4 workgroups per CU)

struct AugArgs {
    cms_aug_desc d;
    Geo g;
    float tau, inv_root_c;
    int tea_cap;        // floats of LDS behind the student's rectangle for the teacher's; 0: never staged
};

// the teacher's (upsampled) logits at the taps of one student pixel: `tea(k)` -> a Gather for teacher pixel (Y0 + k/2, X0 + k%2)
template <bool IDENT>
struct AugTea {
    const float* gbase;     // global: class-0 plane of the sample
    const float* lbase;     // LDS copy of the rectangle `lp` of every class plane, or NULL
    size_t gplane;
    Patch lp;
    int gh, gw;
    float sy, sx;
    bool align;
    int X0, Y0;
    __device__ __forceinline__ Gather<IDENT> operator()(int k) const {
        const int Y = Y0 + (k >> 1), X = X0 + (k & 1);
        Gather<IDENT> r;
        r.base = gbase;
        r.plane = gplane;
        r.w_in = gw;
        if (IDENT) {
            r.off = (size_t)Y * gw + X;
            return r;
        }
        Tap ty = bilin_tap(Y, sy, gh, align), tx = bilin_tap(X, sx, gw, align);
        const bool in = lbase != nullptr && ty.i0 >= lp.y_lo && ty.i1 < lp.y_lo + lp.n_rows && tx.i0 >= lp.x_lo &&
                        tx.i1 < lp.x_lo + lp.n_cols;
        if (in) {
            rebase(ty, tx, lp);
            r.base = lbase;
            r.plane = (size_t)lp.n_rows * lp.n_cols;
            r.w_in = lp.n_cols;
        }
        r.ty = ty;
        r.tx = tx;
        return r;
    }
};

template <bool IDENT>
__device__ __forceinline__ AugTea<IDENT> aug_tea(const AugArgs& a, int n, const float* lds, const Patch& lp) {
    const Geo& g = a.g;
    AugTea<IDENT> t;
    t.gplane = (size_t)g.h * g.w;
    t.gbase = a.d.l_tea + (size_t)n * g.c * t.gplane;
    t.lbase = lds;
    t.lp = lp;
    t.gh = g.h; t.gw = g.w;
    t.sy = g.sy; t.sx = g.sx;
    t.align = g.align != 0;
    t.X0 = t.Y0 = 0;
    return t;
}

// low-resolution cells under the teacher pixels a tile samples (n_rows == 0: the tile looks wholly outside the teacher's view)
__device__ __forceinline__ Patch aug_tile_patch(const Geo& g, const float* xf, int x0, int y0, int tw, int th) {
    const AugBox b = aug_tile_box(xf, x0, y0, tw, th, g.H, g.W);
    Patch p;
    p.x_lo = p.y_lo = p.n_cols = p.n_rows = 0;
    if (b.x_hi < b.x_lo || b.y_hi < b.y_lo) return p;
    const Tap xa = bilin_tap(b.x_lo, g.sx, g.w, g.align != 0), xb = bilin_tap(b.x_hi, g.sx, g.w, g.align != 0);
    const Tap ya = bilin_tap(b.y_lo, g.sy, g.h, g.align != 0), yb = bilin_tap(b.y_hi, g.sy, g.h, g.align != 0);
    p.x_lo = xa.i0; p.n_cols = xb.i1 - xa.i0 + 1;
    p.y_lo = ya.i0; p.n_rows = yb.i1 - ya.i0 + 1;
    return p;
}

__device__ __forceinline__ bool aug_fits(const Patch& p, int C, int cap) {
    return p.n_rows > 0 && p.n_cols > 0 && (long long)C * p.n_rows * p.n_cols <= (long long)cap;
}

// grid_sample(um0) * um1 (:306)
__device__ __forceinline__ float aug_mask(const AugArgs& a, const AugTaps& taps, int n, int y, int x) {
    const Geo& g = a.g;
    const size_t img = (size_t)n * g.H * g.W;
    const float m0 = aug_warp_mask(taps, a.d.um0 ? a.d.um0 + img : nullptr, g.W);
    const float m1 = a.d.um1 ? a.d.um1[img + (size_t)y * g.W + x] : 1.0f;
    return m0 * m1;
}

template <int CT, bool IDENT>
__device__ __forceinline__ void aug_fwd_pixel(const AugArgs& a, const Gather<IDENT>& gs, AugTea<IDENT> tea, int n, int y, int x,
                                              float (&acc)[3]) {
    const Geo& g = a.g;
    const AugTaps taps = aug_taps(a.d.xf + (size_t)n * 6, x, y, g.H, g.W);
    tea.X0 = taps.X0;
    tea.Y0 = taps.Y0;
    const bool thresh = a.tau > 0.0f;
    const PixelFwd r = aug_pixel_fwd<CT>(gs, taps, tea, g.c, a.d.loss_fn, a.inv_root_c, thresh);
    const float lm = r.loss * aug_mask(a, taps, n, y, x);
    const float cf = (thresh && r.conf >= a.tau) ? 1.0f : 0.0f;
    acc[0] += lm;
    acc[1] += lm * cf;
    acc[2] += cf;
}

template <int CT, bool IDENT, class E>
__device__ __forceinline__ void aug_bwd_pixel(const AugArgs& a, float gscale, const Gather<IDENT>& gs, AugTea<IDENT> tea, int n,
                                              int y, int x, E emit) {
    const Geo& g = a.g;
    const AugTaps taps = aug_taps(a.d.xf + (size_t)n * 6, x, y, g.H, g.W);
    tea.X0 = taps.X0;
    tea.Y0 = taps.Y0;
    const bool thresh = a.tau > 0.0f;
    const bool pp = thresh && a.d.conf_per_pixel;
    const float base_f = gscale * aug_mask(a, taps, n, y, x);
    // (no early-out on a zero factor, see cons_bwd_ident_kernel)
    auto factor = [&](float conf) { return (pp && !(conf >= a.tau)) ? 0.0f : base_f; };
    aug_pixel_bwd<CT>(gs, taps, tea, g.c, a.d.loss_fn, a.inv_root_c, thresh, factor, emit);
}

// the student's rectangle `p` of a tile to `P` and, unless `Pt` is NULL, the teacher's rectangle `tp` to `Pt`
__device__ __forceinline__ void aug_stage(const AugArgs& a, int n, const Patch& p, float* P, float* Pt, const Patch& tp) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w, sample = (size_t)n * g.c * plane;
    stage_patch(P, a.d.l_stu + sample, g.c, plane, g.w, p);
    if (Pt) stage_patch(Pt, a.d.l_tea + sample, g.c, plane, g.w, tp);
}

template <int CT>
__global__ __launch_bounds__(256) void aug_fwd_tiled_kernel(AugArgs a, float* __restrict__ partials, int patch_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Geo& g = a.g;
    // the teacher's rectangle of this workgroup's tile (fwd_tile_walk derives the same tile from the same arithmetic)
    const ScatterTile tile = fwd_tile(g);
    const Patch tp = aug_tile_patch(g, a.d.xf + (size_t)tile.n * 6, tile.x0, tile.y0, tile.tw, tile.th);
    const bool staged = aug_fits(tp, g.c, a.tea_cap);               // (uniform over the workgroup)
    const AugTea<false> tea = aug_tea<false>(a, tile.n, staged ? smem + patch_stride : nullptr, tp);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    fwd_tile_walk<false>(
        g, smem, [&](int n, const Patch& p, float* P) { aug_stage(a, n, p, P, staged ? P + patch_stride : nullptr, tp); },
        [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p) {
            aug_fwd_pixel<CT, false>(a, gather_staged(smem, p, ty, tx), tea, n, y, x, acc);
        });
    __shared__ float red[3 * 16];
    store_partials<3>(acc, red, partials);
}

// direct gathers from global memory: identity geometry (the U-Nets), or student rectangles beyond FWD_PATCH_LDS_MAX
template <int CT, bool IDENT>
__global__ __launch_bounds__(256) void aug_fwd_kernel(AugArgs a, float* __restrict__ partials) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    pixel_walk(g, [&](size_t, int n, int y, int x) {
        aug_fwd_pixel<CT, IDENT>(a, gather_at<IDENT>(a.d.l_stu + (size_t)n * g.c * plane, g, y, x),
                                 aug_tea<IDENT>(a, n, nullptr, Patch{0, 0, 0, 0}), n, y, x, acc);
    });
    __shared__ float red[3 * 16];
    store_partials<3>(acc, red, partials);
}

template <int CT>
__global__ __launch_bounds__(256) void aug_bwd_ident_kernel(AugArgs a, const float* __restrict__ scalars, float* __restrict__ grad) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w;
    const float gscale = scalars[2];
    pixel_walk(g, [&](size_t, int n, int y, int x) {
        const size_t sample = (size_t)n * g.c * plane;
        const Gather<true> gs = gather_at<true>(a.d.l_stu + sample, g, y, x);
        float* gp = grad + sample + gs.off;
        aug_bwd_pixel<CT, true>(a, gscale, gs, aug_tea<true>(a, n, nullptr, Patch{0, 0, 0, 0}), n, y, x,
                                [&](int k, float v) { gp[k * plane] += v; });
    });
}

template <int CT>
__global__ __launch_bounds__(256) void aug_bwd_tiled_kernel(AugArgs a, const float* __restrict__ scalars, float* __restrict__ grad,
                                                            int patch_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Geo& g = a.g;
    const float gscale = scalars[2];
    // the teacher's rectangle of this workgroup's tile (tiled_scatter derives the same tile from the same arithmetic)
    const ScatterTile tile = scatter_tile(g);
    const Patch tp = aug_tile_patch(g, a.d.xf + (size_t)tile.n * 6, tile.x0, tile.y0, tile.tw, tile.th);
    const bool staged = aug_fits(tp, g.c, a.tea_cap);               // (uniform over the workgroup)
    // LDS behind G and R: the student's rectangle | the teacher's, `pstride` floats apart
    const int pstride = patch_stride;
    auto stage = [&](int n, const Patch& p, float* P) { aug_stage(a, n, p, P, staged ? P + pstride : nullptr, tp); };
    auto pixel_grad = [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p, const float* P, auto emit) -> bool {
        // (taps already rebased to the rectangle)
        aug_bwd_pixel<CT, false>(a, gscale, gather_staged(P, p, ty, tx), aug_tea<false>(a, n, staged ? P + pstride : nullptr, tp), n, y,
                                 x, emit);
        return true;
    };
    tiled_scatter(g, stage, pixel_grad, grad, smem);
}

// ---- host side
static int check_aug(const cms_aug_desc* d) {
    CMS_REQUIRE(d != nullptr, "aug: null descriptor");
    CMS_REQUIRE(d->l_stu && d->l_tea, "aug: l_stu / l_tea must not be NULL");
    CMS_REQUIRE(d->xf, "aug: xf must not be NULL");
    int rc = check_sizes_positive(d, "aug");
    if (rc) return rc;
    CMS_REQUIRE(d->H >= 2 && d->W >= 2, "aug: the align_corners=True grid needs H >= 2 and W >= 2 (got %d x %d)", d->H, d->W);
    rc = check_logits_fit(d, "aug");
    return rc ? rc : check_loss_fn(d);
}

// capacity rule: the teacher's rectangle may use the LDS left beside what the kernel stages anyway, AUG_TEA_LDS_MAX at most
static int aug_tea_cap(size_t limit, size_t used, bool force_global) {
    if (force_global || used >= limit) return 0;
    return (int)(std::min(limit - used, AUG_TEA_LDS_MAX) / sizeof(float));
}

static AugArgs make_aug_args(const cms_aug_desc* d) {
    AugArgs a;
    a.d = *d;
    a.g = geo_of(d);
    a.tau = d->conf_thresh;
    a.inv_root_c = (float)(1.0 / sqrt((double)d->c));
    a.tea_cap = 0;
    return a;
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_aug_workspace_bytes(const cms_aug_desc* d) {
    if (!d || d->n <= 0 || d->c <= 0 || d->h <= 0 || d->w <= 0 || d->H <= 0 || d->W <= 0) return 0;
    return (size_t)fwd_blocks(geo_of(d), 1) * 3 * sizeof(float);
}

extern "C" int cms_aug_fwd(const cms_aug_desc* d, void* workspace, double* stats_out, void* stream) {
    int rc = check_aug(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out, "aug_fwd: workspace / stats_out NULL");
    AugArgs a = make_aug_args(d);
    FwdPlan p = fwd_plan(a.g, 1);
    if (p.tiles > 0) {
        a.tea_cap = aug_tea_cap(FWD_PATCH_LDS_MAX, p.lds, d->force_global != 0);
        p.lds += (size_t)a.tea_cap * sizeof(float);
    }
    CMS_DISPATCH_C(d->c, launch_fwd<3>(aug_fwd_tiled_kernel<CT>, aug_fwd_kernel<CT, true>, aug_fwd_kernel<CT, false>, a, p,
                                       (float*)workspace, stats_out, (double)((size_t)d->n * d->H * d->W), 3,
                                       (hipStream_t)stream, p.pstride));
    return launch_status("cms_aug_fwd");
}

extern "C" int cms_aug_bwd(const cms_aug_desc* d, const float* scalars, float* grad_l_stu, void* stream) {
    int rc = check_aug(d);
    if (rc) return rc;
    CMS_REQUIRE(scalars && grad_l_stu, "aug_bwd: scalars / grad NULL");
    AugArgs a = make_aug_args(d);
    // the teacher's rectangle: the LDS left beside G, R and the student's rectangle of a backward tile
    if (!is_ident(a.g)) a.tea_cap = aug_tea_cap(TILE_LDS_MAX, tile_lds_bytes(d->c, a.g.sy, a.g.sx, 1), d->force_global != 0);
    const int pstride = (int)patch_floats(d->c, a.g.sy, a.g.sx, TILE_H);
    CMS_DISPATCH_C(d->c, rc = launch_bwd("aug_bwd", aug_bwd_ident_kernel<CT>, aug_bwd_tiled_kernel<CT>, a, 1,
                                         (size_t)a.tea_cap * sizeof(float), scalars, grad_l_stu, (hipStream_t)stream, pstride));
    return rc ? rc : launch_status("cms_aug_bwd");
}
