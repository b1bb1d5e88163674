// ICT (interpolation consistency training, gfx950).
//
// Input blend: out = x0 * (1 - lam[n]) + x1 * lam[n] per sample, train_seg_semisup_ict.py:310-311 -- the student's image and the
// loss's validity mask. HBM-bound: two tensors read, one written, 16 bytes per lane per access.
//
// Interpolation loss (second half of this file): thin shells over the tile walks and launch paths of csrc/loss_tiles.hpp, which
// it shares with the CutMix consistency (losses.hip). The per-pixel arithmetic of both is csrc/ict_math.hpp.
#include <algorithm>
#include "loss_tiles.hpp"
#include "ict_math.hpp"

namespace cms {

template <typename T>
struct BlendElem;
template <>
struct BlendElem<float> {
    static __device__ __forceinline__ float load(float v) { return v; }
    static __device__ __forceinline__ float store(float v) { return v; }
};
template <>
struct BlendElem<uint16_t> {      // bf16: fp32 arithmetic, ONE rounding of the sum
    static __device__ __forceinline__ float load(uint16_t v) { return bf16_to_f32(v); }
    static __device__ __forceinline__ uint16_t store(float v) { return f32_to_bf16(v); }
};

// The tensors are walked FLAT in vectors of VEC elements (VEC * sizeof(T) = 16 bytes), so the accesses stay aligned when
// `chw` is no multiple of VEC; a vector that straddles a sample boundary switches its factor on the way. The last
// total % VEC elements are the scalar tail. IDX32: the element count fits 32 bits (one 32-bit division per vector).
template <typename T, int VEC, bool IDX32>
__global__ __launch_bounds__(256) void ict_blend_kernel(const T* __restrict__ x0, const T* __restrict__ x1, T* __restrict__ out,
                                                        const float* __restrict__ lam, size_t total, size_t chw) {
    struct alignas(VEC * sizeof(T)) Vec {
        T v[VEC];
    };
    const size_t nvec = total / VEC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e0 = i * VEC;
        size_t s, rem;
        if (IDX32) {
            const uint32_t q = (uint32_t)e0 / (uint32_t)chw;
            s = q;
            rem = (uint32_t)e0 - q * (uint32_t)chw;
        } else {
            s = e0 / chw;
            rem = e0 - s * chw;
        }
        const Vec a = reinterpret_cast<const Vec*>(x0)[i], b = reinterpret_cast<const Vec*>(x1)[i];
        Vec o;
        float l = lam[s];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            o.v[j] = BlendElem<T>::store(ict_mix(BlendElem<T>::load(a.v[j]), BlendElem<T>::load(b.v[j]), 1.0f - l, l));
            if (++rem == chw && j + 1 < VEC && e0 + j + 1 < total) {
                rem = 0;
                l = lam[++s];
            }
        }
        reinterpret_cast<Vec*>(out)[i] = o;
    }
    const size_t tail = nvec * VEC + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tail < total) {
        const float l = lam[tail / chw];
        out[tail] = BlendElem<T>::store(ict_mix(BlendElem<T>::load(x0[tail]), BlendElem<T>::load(x1[tail]), 1.0f - l, l));
    }
}

template <typename T, int VEC>
static void blend_launch(const void* x0, const void* x1, void* out, const float* lam, size_t total, size_t chw, hipStream_t s) {
    const int grid = grid_for(total / VEC + 1, 256, 256 * 16);
    if (total < ((size_t)1 << 32))
        hipLaunchKernelGGL((ict_blend_kernel<T, VEC, true>), dim3(grid), dim3(256), 0, s, (const T*)x0, (const T*)x1, (T*)out, lam,
                           total, chw);
    else
        hipLaunchKernelGGL((ict_blend_kernel<T, VEC, false>), dim3(grid), dim3(256), 0, s, (const T*)x0, (const T*)x1, (T*)out, lam,
                           total, chw);
}

}  // namespace cms

using namespace cms;

extern "C" int cms_ict_blend(const void* x0, const void* x1, void* out, int dtype, const float* lam, int n, long long chw,
                             void* stream) {
    CMS_REQUIRE(x0 && x1 && out && lam, "ict_blend: NULL argument");
    CMS_REQUIRE(dtype == CMS_F32 || dtype == CMS_BF16, "ict_blend: unknown dtype %d", dtype);
    CMS_REQUIRE(n > 0 && chw > 0, "ict_blend: bad geometry");
    const size_t total = (size_t)n * (size_t)chw;
    const bool aligned = (((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)out) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CMS_F32) {
        if (aligned) blend_launch<float, 4>(x0, x1, out, lam, total, (size_t)chw, s);
        else blend_launch<float, 1>(x0, x1, out, lam, total, (size_t)chw, s);
    } else {
        if (aligned) blend_launch<uint16_t, 8>(x0, x1, out, lam, total, (size_t)chw, s);
        else blend_launch<uint16_t, 1>(x0, x1, out, lam, total, (size_t)chw, s);
    }
    return launch_status("cms_ict_blend");
}

// ================================================================================================ the interpolation loss
// Interpolation consistency training (train_seg_semisup_ict.py:306-391): the student sees a per-sample blend of two images,
// the target is the same blend of the teacher's two predictions. Same kernel shapes as the CutMix consistency of losses.hip (one
// thread per output pixel, the low-resolution rectangles of the THREE logit tensors staged to LDS per tile, class axis in
// registers, the tiled adjoint of the upsample for the backward); the per-pixel arithmetic is csrc/ict_math.hpp. Compulsory
// traffic per launch: the two validity masks (2 * P * 4 B) and the three low-resolution logit tensors; nothing of size C * P.
namespace cms {

struct IctArgs {
    cms_ict_desc d;
    Geo g;
    float tau, inv_root_c;
    float* cmap;        // (H,W) sum_i [conf(i,y,x) >= tau] -- --conf_per_pixel with a threshold only, else NULL
    int count_pass;     // forward kernels: 1 = write `cmap` (teachers only), 0 = the loss sums
};

__device__ __forceinline__ float ict_um(const IctArgs& a, size_t pix, float lam) {
    // um0 * (1 - lam) + um1 * lam (:311); a missing mask is the all-ones mask the reference's loader would deliver
    const float u0 = a.d.um0 ? a.d.um0[pix] : 1.0f, u1 = a.d.um1 ? a.d.um1[pix] : 1.0f;
    return ict_mix(u0, u1, 1.0f - lam, lam);
}

// one pixel of a forward kernel from its three gathers: a vote into the confidence map (count pass) or the three loss sums
template <int CT, bool IDENT>
__device__ __forceinline__ void ict_fwd_pixel(const IctArgs& a, const Gather<IDENT>& gs, const Gather<IDENT>& g0,
                                              const Gather<IDENT>& g1, int n, int y, int x, float lam, float (&acc)[3]) {
    const Geo& g = a.g;
    const size_t yx = (size_t)y * g.W + x;
    if (a.count_pass) {
        float conf;
        if (CT > 0) {
            RegVec<CT> r0, r1;
            fill<CT, IDENT>(r0, g0);
            fill<CT, IDENT>(r1, g1);
            conf = ict_conf<CT>(r0, r1, lam, g.c);
        } else {
            conf = ict_conf<0>(g0, g1, lam, g.c);
        }
        // whole numbers <= N: the float sum is exact whatever order the samples' workgroups arrive in
        if (conf >= a.tau) atomicAdd(a.cmap + yx, 1.0f);
        return;
    }
    PixelFwd r;
    if (CT > 0) {
        RegVec<CT> rs, r0, r1;
        fill<CT, IDENT>(rs, gs);
        fill<CT, IDENT>(r0, g0);
        fill<CT, IDENT>(r1, g1);
        r = ict_pixel_fwd<CT>(rs, r0, r1, lam, g.c, a.d.loss_fn, a.inv_root_c);
    } else {
        r = ict_pixel_fwd<0>(gs, g0, g1, lam, g.c, a.d.loss_fn, a.inv_root_c);
    }
    const float lm = r.loss * ict_um(a, (size_t)n * g.H * g.W + yx, lam);
    const float cf = (a.tau > 0.0f && r.conf >= a.tau) ? 1.0f : 0.0f;
    // --conf_per_pixel: the batch mean of the indicator at this pixel position (the reference's broadcast, cutmixseg.h)
    const float wgt = a.cmap ? a.cmap[yx] / (float)g.n : cf;
    acc[0] += lm;
    acc[1] += lm * wgt;
    acc[2] += cf;
}

// student | teacher 0 | teacher 1 rectangles of a tile, `pstride` floats apart (the count pass reads the teachers only)
__device__ __forceinline__ void ict_stage(const IctArgs& a, int n, const Patch& p, float* P, int pstride, bool student) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w, sample = (size_t)n * g.c * plane;
    if (student) stage_patch(P, a.d.l_stu + sample, g.c, plane, g.w, p);
    stage_patch(P + pstride, a.d.l_tea0 + sample, g.c, plane, g.w, p);
    stage_patch(P + 2 * pstride, a.d.l_tea1 + sample, g.c, plane, g.w, p);
}

template <int CT>
__global__ __launch_bounds__(256) void ict_fwd_tiled_kernel(IctArgs a, float* __restrict__ partials, int patch_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const float lam = a.d.lam[fwd_tile(a.g).n];
    float acc[3] = {0.0f, 0.0f, 0.0f};
    fwd_tile_walk<false>(
        a.g, smem, [&](int n, const Patch& p, float* P) { ict_stage(a, n, p, P, patch_stride, !a.count_pass); },
        [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p) {
            ict_fwd_pixel<CT, false>(a, gather_staged(smem, p, ty, tx), gather_staged(smem + patch_stride, p, ty, tx),
                                     gather_staged(smem + 2 * patch_stride, p, ty, tx), n, y, x, lam, acc);
        });
    if (a.count_pass) return;           // (uniform over the launch)
    __shared__ float red[3 * 16];
    store_partials<3>(acc, red, partials);
}

// the three gathers of pixel (y, x) of sample n from global memory
template <bool IDENT>
struct IctGathers {
    Gather<IDENT> s, t0, t1;
};
template <bool IDENT>
__device__ __forceinline__ IctGathers<IDENT> ict_gathers(const IctArgs& a, int n, int y, int x) {
    const Geo& g = a.g;
    const size_t sample = (size_t)n * g.c * ((size_t)g.h * g.w);
    IctGathers<IDENT> r;
    r.s = gather_at<IDENT>(a.d.l_stu + sample, g, y, x);
    r.t0 = r.t1 = r.s;
    r.t0.base = a.d.l_tea0 + sample;
    r.t1.base = a.d.l_tea1 + sample;
    return r;
}

// direct gathers from global memory: identity geometry (the U-Nets), or rectangles beyond FWD_PATCH_LDS_MAX
template <int CT, bool IDENT>
__global__ __launch_bounds__(256) void ict_fwd_kernel(IctArgs a, float* __restrict__ partials) {
    float acc[3] = {0.0f, 0.0f, 0.0f};
    pixel_walk(a.g, [&](size_t, int n, int y, int x) {
        const IctGathers<IDENT> t = ict_gathers<IDENT>(a, n, y, x);
        ict_fwd_pixel<CT, IDENT>(a, t.s, t.t0, t.t1, n, y, x, a.d.lam[n], acc);
    });
    if (a.count_pass) return;           // (uniform over the launch)
    __shared__ float red[3 * 16];
    store_partials<3>(acc, red, partials);
}

// factor of a pixel's gradient vector: the finalised scale x the blended validity mask [x the batch-mean indicator]. The
// confidence enters through scalars[2] (default mode: the rate) or the map (--conf_per_pixel); neither depends on the student.
__device__ __forceinline__ float ict_bwd_factor(const IctArgs& a, float gscale, int n, int y, int x, float lam) {
    const Geo& g = a.g;
    const size_t yx = (size_t)y * g.W + x;
    float f = gscale * ict_um(a, (size_t)n * g.H * g.W + yx, lam);
    if (a.cmap) f *= a.cmap[yx] / (float)g.n;
    return f;
}

template <int CT>
__global__ __launch_bounds__(256) void ict_bwd_ident_kernel(IctArgs a, const float* __restrict__ scalars, float* __restrict__ grad) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w;
    const float gscale = scalars[2];
    pixel_walk(g, [&](size_t, int n, int y, int x) {
        const float lam = a.d.lam[n];
        const IctGathers<true> t = ict_gathers<true>(a, n, y, x);
        float* gp = grad + (size_t)n * g.c * plane + t.s.off;
        const float f = ict_bwd_factor(a, gscale, n, y, x, lam);
        // (no early-out on f == 0, see cons_bwd_ident_kernel)
        if (CT > 0) {
            RegVec<CT> rs, r0, r1;
            fill<CT, true>(rs, t.s);
            fill<CT, true>(r0, t.t0);
            fill<CT, true>(r1, t.t1);
            ict_pixel_bwd<CT>(rs, r0, r1, lam, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { gp[k * plane] += f * v; });
        } else {
            ict_pixel_bwd<0>(t.s, t.t0, t.t1, lam, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { gp[k * plane] += f * v; });
        }
    });
}

template <int CT>
__global__ __launch_bounds__(256) void ict_bwd_tiled_kernel(IctArgs a, const float* __restrict__ scalars, float* __restrict__ grad,
                                                            int patch_stride) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Geo& g = a.g;
    const float gscale = scalars[2];
    // LDS copies of the tile's logit rectangles: student | teacher 0 | teacher 1, `pstride` floats apart
    const int pstride = patch_stride;
    auto stage = [&](int n, const Patch& p, float* P) { ict_stage(a, n, p, P, pstride, true); };
    auto pixel_grad = [&](int n, int y, int x, const Tap& ty, const Tap& tx, const Patch& p, const float* P, auto emit) -> bool {
        const float lam = a.d.lam[n];
        const float f = ict_bwd_factor(a, gscale, n, y, x, lam);
        // (taps already rebased to the rectangle)
        const Gather<false> gs = gather_staged(P, p, ty, tx), g0 = gather_staged(P + pstride, p, ty, tx),
                            g1 = gather_staged(P + 2 * pstride, p, ty, tx);
        if (CT > 0) {
            RegVec<CT> rs, r0, r1;
            fill<CT, false>(rs, gs);
            fill<CT, false>(r0, g0);
            fill<CT, false>(r1, g1);
            ict_pixel_bwd<CT>(rs, r0, r1, lam, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { emit(k, f * v); });
        } else {
            ict_pixel_bwd<0>(gs, g0, g1, lam, g.c, a.d.loss_fn, a.inv_root_c, [&](int k, float v) { emit(k, f * v); });
        }
        return true;
    };
    tiled_scatter(g, stage, pixel_grad, grad, smem);
}

// ---- host side
static int check_ict(const cms_ict_desc* d) {
    CMS_REQUIRE(d != nullptr, "ict: null descriptor");
    CMS_REQUIRE(d->l_stu && d->l_tea0 && d->l_tea1, "ict: l_stu / l_tea0 / l_tea1 must not be NULL");
    CMS_REQUIRE(d->lam, "ict: lam must not be NULL");
    int rc = check_geometry(d, "ict");
    return rc ? rc : check_loss_fn(d);
}

static bool ict_has_map(const cms_ict_desc* d) { return d->conf_thresh > 0.0f && d->conf_per_pixel != 0; }

// workspace = [per-workgroup partial sums, padded to 256 B][the (H,W) confidence map, --conf_per_pixel only]
static size_t ict_partials_bytes(const Geo& g) {
    return (((size_t)fwd_blocks(g, 3) * 3 * sizeof(float)) + 255) / 256 * 256;
}

static IctArgs make_ict_args(const cms_ict_desc* d, const void* workspace) {
    IctArgs a;
    a.d = *d;
    a.g = geo_of(d);
    a.tau = d->conf_thresh;
    a.inv_root_c = (float)(1.0 / sqrt((double)d->c));
    a.cmap = ict_has_map(d) ? (float*)((char*)workspace + ict_partials_bytes(a.g)) : nullptr;
    a.count_pass = 0;
    return a;
}

}  // namespace cms

extern "C" size_t cms_ict_workspace_bytes(const cms_ict_desc* d) {
    if (!d || d->n <= 0 || d->c <= 0 || d->h <= 0 || d->w <= 0 || d->H <= 0 || d->W <= 0) return 0;
    return ict_partials_bytes(geo_of(d)) + (ict_has_map(d) ? (size_t)d->H * d->W * sizeof(float) : 0);
}

extern "C" int cms_ict_fwd(const cms_ict_desc* d, void* workspace, double* stats_out, void* stream) {
    int rc = check_ict(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out, "ict_fwd: workspace / stats_out NULL");
    IctArgs a = make_ict_args(d, workspace);
    hipStream_t s = (hipStream_t)stream;
    const FwdPlan p = fwd_plan(a.g, 3);
    if (a.cmap) {
        hipError_t e = hipMemsetAsync(a.cmap, 0, (size_t)d->H * d->W * sizeof(float), s);
        CMS_REQUIRE(e == hipSuccess, "ict_fwd: clearing the confidence map: %s", hipGetErrorString(e));
    }
    // --conf_per_pixel: every sample's vote into the map first, then the loss sums weighted with it
    for (int pass = a.cmap ? 1 : 0; pass >= 0; --pass) {
        a.count_pass = pass;
        // (the count pass leaves no sums: the reduction runs behind the loss pass only)
        CMS_DISPATCH_C(d->c, launch_fwd<3>(ict_fwd_tiled_kernel<CT>, ict_fwd_kernel<CT, true>, ict_fwd_kernel<CT, false>, a, p,
                                           (float*)workspace, pass ? nullptr : stats_out, (double)((size_t)d->n * d->H * d->W), 3, s,
                                           p.pstride));
    }
    return launch_status("cms_ict_fwd");
}

extern "C" int cms_ict_bwd(const cms_ict_desc* d, const void* workspace, const float* scalars, float* grad_l_stu, void* stream) {
    int rc = check_ict(d);
    if (rc) return rc;
    CMS_REQUIRE(scalars && grad_l_stu, "ict_bwd: scalars / grad NULL");
    CMS_REQUIRE(workspace || !ict_has_map(d), "ict_bwd: conf_per_pixel needs the workspace cms_ict_fwd filled");
    IctArgs a = make_ict_args(d, workspace);
    const int pstride = (int)patch_floats(d->c, a.g.sy, a.g.sx, TILE_H);
    CMS_DISPATCH_C(d->c, rc = launch_bwd("ict_bwd", ict_bwd_ident_kernel<CT>, ict_bwd_tiled_kernel<CT>, a, 3, 0, scalars, grad_l_stu,
                                         (hipStream_t)stream, pstride));
    return rc ? rc : launch_status("cms_ict_bwd");
}
