// Class-threshold consistency (gfx950): the masked consistency loss of losses.hip with the scalar confidence threshold replaced
// by a per-class one, thr[argmax of the teacher row], and -- in the forward and the fused launch -- the statistics a self-adaptive
// threshold is made from, summed over the launch's valid pixels as exact integers (definition: include/cutmixseg.h).
//
// The kernels and their launches are those of losses.hip -- ONE body, the templates of cons_kernels.hpp, instantiated here with the
// policy `ClassThresh` below; with thr == tau in every entry the loss sums are bit for bit those of cms_consistency_*. What the
// policy adds per pixel is an argmax over the teacher row (registers), one LDS read of thr[k*] and the statistics:
//   * S_c / S_conf / n_valid: per-thread 32-bit partials (compile-time class counts) -> one integer wave reduction at the end of
//     the kernel -> one 64-bit LDS add per wave -> one 64-bit global atomic add per slot per workgroup, into one of
//     CMS_CTHRESH_REPLICAS copies of the table. Integer sums do not depend on the order of additions, so neither does the table.
//   * N_pred[k*] / N_pass[k*]: LDS integer atomics per pixel, as csrc/calib.hip counts its bins.
//   * the run-time class count has no register array: its S_c go to the LDS table per pixel (LDS atomics, never global ones).
// No float atomics and no per-pixel global atomics anywhere.
#include "cons_kernels.hpp"
#include "cthresh_math.hpp"

namespace cms {

constexpr int CT_RT_MAX = 128;      // most classes of the run-time path: thr[] and the table live in static LDS. With 128 the backward
                                    // kernels' static LDS (tiled_scatter's 3520 B + thr) stays within the 4096 B that TILE_LDS_MAX leaves
                                    // below the 160 KB of a workgroup: cms_cthresh_bwd runs wherever cms_consistency_bwd does

struct CtArgs : ConsArgs {
    const float* thr;
    unsigned long long* table;
};

template <int CT>
struct CtShared {
    static constexpr int N = CT > 0 ? CT : CT_RT_MAX;
    unsigned long long tab[2 + 3 * N];
    float thr[N];
};

// Flush bound of the per-thread partials. Every addend is ct_fix24(v) <= 2^24, so a 32-bit partial holds 255 pixels:
// 255 * 2^24 = 2^32 - 2^24 < 2^32. The tiled kernels give a thread at most TILE_H / 4 or FWD_TILE_H / 4 = 2 pixels and never flush;
// the flat pixel walk flushes a thread's partials into the LDS table (64-bit LDS atomics) after CT_FLUSH pixels.
constexpr uint32_t CT_FLUSH = 255;

template <int CT>
struct CtAcc {
    uint32_t s[CT > 0 ? CT : 1];
    uint32_t sconf, nvalid;
};

template <int CT>
__device__ __forceinline__ void ct_acc_zero(CtAcc<CT>& acc) {
#pragma unroll
    for (int c = 0; c < (CT > 0 ? CT : 1); ++c) acc.s[c] = 0u;
    acc.sconf = 0u;
    acc.nvalid = 0u;
}

// the backward kernels read thr only
template <int CT>
struct CtThr {
    float thr[CT > 0 ? CT : CT_RT_MAX];
};

// thr[] -> LDS (one vector load per class per workgroup), the LDS table zeroed; behind the barrier both may be used
template <int CT>
__device__ __forceinline__ void ct_begin(const CtArgs& a, CtShared<CT>& sh) {
    const int C = a.g.c;
    for (int i = threadIdx.x; i < C; i += blockDim.x) sh.thr[i] = a.thr[i];
    for (int i = threadIdx.x; i < ct_table_len(C); i += blockDim.x) sh.tab[i] = 0ull;
    __syncthreads();
}

template <int CT>
__device__ __forceinline__ void ct_begin_thr(const CtArgs& a, CtThr<CT>& sh) {
    for (int i = threadIdx.x; i < a.g.c; i += blockDim.x) sh.thr[i] = a.thr[i];
    __syncthreads();
}

// valid pixel, for the statistics only: mix -- the validity map of the image the mask selects; cut -- um0 whatever the mask bit
__device__ __forceinline__ bool ct_valid(const CtArgs& a, const ConsPixel& px, int n, int y, int x) {
    if (a.d.mode == MODE_MIX) return px.um >= 0.5f;
    if (!a.d.um0) return true;
    return a.d.um0[((size_t)n * a.d.H + y) * a.d.W + x] >= 0.5f;
}

// the statistics of one pixel whose teacher row is `lt` (registers, or a gather for the run-time class count)
template <int CT, class LT>
__device__ __forceinline__ void ct_count(const CtArgs& a, CtShared<CT>& sh, CtAcc<CT>& acc, const LT& lt, int k, bool pass, bool valid) {
    if (!valid) return;
    const int C = a.g.c;
    float conf;
    if (CT > 0) {
        ct_pixel_stats<CT>(lt, C, conf, [&](int c, uint32_t v) { acc.s[CT > 0 ? c : 0] += v; });
    } else {
        ct_pixel_stats<0>(lt, C, conf, [&](int c, uint32_t v) { atomicAdd(&sh.tab[ct_slot_s(C, c)], (unsigned long long)v); });
    }
    acc.sconf += ct_fix24(conf);
    acc.nvalid += 1u;
    atomicAdd(&sh.tab[ct_slot_pred(C, k)], 1ull);
    if (pass) atomicAdd(&sh.tab[ct_slot_pass(C, k)], 1ull);
}

// a thread's partials -> the LDS table (divergent callers: plain per-thread LDS atomics)
template <int CT>
__device__ __forceinline__ void ct_flush(const CtArgs& a, CtShared<CT>& sh, CtAcc<CT>& acc) {
    const int C = a.g.c;
    if (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) atomicAdd(&sh.tab[ct_slot_s(C, c)], (unsigned long long)acc.s[CT > 0 ? c : 0]);
    }
    atomicAdd(&sh.tab[0], (unsigned long long)acc.nvalid);
    atomicAdd(&sh.tab[1], (unsigned long long)acc.sconf);
    ct_acc_zero(acc);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// End of a kernel, every thread of the workgroup: partials -> wave sums -> LDS table -> ONE global add per non-zero slot.
// The 32-bit wave sum holds because a partial is at most 2 pixels here (tiled kernels) or has just been flushed (flat walk, PPT2
// false: flush first, nothing left to reduce): 64 lanes * 2 * 2^24 = 2^31.
template <int CT, bool PPT2>
__device__ __forceinline__ void ct_finish(const CtArgs& a, CtShared<CT>& sh, CtAcc<CT>& acc) {
    const int C = a.g.c;
    if (PPT2) {
        const int lane = threadIdx.x & 63;
        if (CT > 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const uint32_t v = wave_sum_u32(acc.s[CT > 0 ? c : 0]);
                if (lane == 0 && v) atomicAdd(&sh.tab[ct_slot_s(C, c)], (unsigned long long)v);
            }
        }
        const uint32_t nv = wave_sum_u32(acc.nvalid), sc = wave_sum_u32(acc.sconf);
        if (lane == 0) {
            if (nv) atomicAdd(&sh.tab[0], (unsigned long long)nv);
            if (sc) atomicAdd(&sh.tab[1], (unsigned long long)sc);
        }
    } else {
        ct_flush<CT>(a, sh, acc);
    }
    __syncthreads();
    // (one of CMS_CTHRESH_REPLICAS copies of the table, by workgroup index: with ONE copy the thousands of workgroups of a launch
    // queue at the same 2 + 3C addresses -- 4860 x 65 adds at 10 x 321 x 321, measured at 19 ns each: 0.1 ms, the whole launch again)
    unsigned long long* dst = a.table + (size_t)(blockIdx.x % CMS_CTHRESH_REPLICAS) * ct_table_len(C);
    for (int i = threadIdx.x; i < ct_table_len(C); i += blockDim.x) {
        const unsigned long long v = sh.tab[i];
        if (v) atomicAdd(&dst[i], v);
    }
}

// ------------------------------------------------------------------------------------------------ the threshold policy
// What cons_kernels.hpp asks of a policy. The threshold of a pixel is thr[k*], read from LDS.
struct CtPick {
    int k;
    float thr;
    __device__ __forceinline__ bool passes(float conf) const { return ct_pass(conf, thr); }
};

struct ClassThresh {
    using Args = CtArgs;
    static __device__ __forceinline__ bool on(const CtArgs&) { return true; }      // class thresholds are always on

    // forward and fused kernels: thr[] and the table in the static LDS of this state, the partials in registers
    template <int CT, bool PPT2>
    struct Fwd {
        static_assert(!PPT2 || (FWD_TILE_H / 4 <= 2 && TILE_H / 4 <= 2), "ct_finish: 32-bit wave sums hold two pixels per thread");
        CtAcc<CT> acc;
        static __device__ __forceinline__ CtShared<CT>& sh() {
            __shared__ CtShared<CT> s;
            return s;
        }
        __device__ __forceinline__ explicit Fwd(const CtArgs& a) {
            ct_begin<CT>(a, sh());
            ct_acc_zero(acc);
        }
        __device__ __forceinline__ bool valid(const CtArgs& a, const ConsPixel& px, int n, int y, int x) const { return ct_valid(a, px, n, y, x); }
        template <class LT>
        __device__ __forceinline__ CtPick pick(const CtArgs& a, const LT& lt) const {
            const int k = ct_kstar<CT>(lt, a.g.c);
            return CtPick{k, sh().thr[k]};
        }
        template <class LT>
        __device__ __forceinline__ void count(const CtArgs& a, const LT& lt, const CtPick& t, bool pass, bool valid) {
            ct_count<CT>(a, sh(), acc, lt, t.k, pass, valid);
        }
        // (the flat walk, whose threads see any number of pixels)
        __device__ __forceinline__ void pixel_done(const CtArgs& a) {
            if (acc.nvalid >= CT_FLUSH) ct_flush<CT>(a, sh(), acc);
        }
        __device__ __forceinline__ void finish(const CtArgs& a) { ct_finish<CT, PPT2>(a, sh(), acc); }
    };

    // backward kernels: thr[] alone; k* of the run-time class count by ct_argmax from the maximum the kernel has computed
    template <int CT>
    struct Bwd {
        static __device__ __forceinline__ CtThr<CT>& sh() {
            __shared__ CtThr<CT> s;
            return s;
        }
        __device__ __forceinline__ explicit Bwd(const CtArgs& a) { ct_begin_thr<CT>(a, sh()); }
        template <class LT>
        __device__ __forceinline__ CtPick pick(const CtArgs& a, const LT& lt) const {
            const int k = ct_kstar<CT>(lt, a.g.c);
            return CtPick{k, sh().thr[k]};
        }
        template <class LT>
        __device__ __forceinline__ CtPick pick_max(const CtArgs& a, const LT& lt, float mx) const {
            const int k = ct_argmax<CT>(lt, a.g.c, mx);
            return CtPick{k, sh().thr[k]};
        }
    };
};

__global__ void ct_update_kernel(int C, int adaptive, double lam, double floor_v, double ceil_v, double* __restrict__ state,
                                 float* __restrict__ thr, unsigned long long* __restrict__ table, unsigned long long* __restrict__ epoch) {
    // the table of the definition = the sum of the copies the launches added into (integers: any order); the copies are zeroed
    __shared__ unsigned long long tab[2 + 3 * CT_RT_MAX];
    const int len = ct_table_len(C);
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
        unsigned long long s = 0ull;
        for (int r = 0; r < CMS_CTHRESH_REPLICAS; ++r) {
            s += table[(size_t)r * len + i];
            table[(size_t)r * len + i] = 0ull;
        }
        tab[i] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) ct_update(C, adaptive, lam, floor_v, ceil_v, state, thr, tab, epoch);
}

// ------------------------------------------------------------------------------------------------ host side
static int check_ct(const cms_cthresh_desc* d) {
    CMS_REQUIRE(d != nullptr, "cthresh: null descriptor");
    const int rc = check_cons(&d->cons);
    if (rc) return rc;
    CMS_REQUIRE(d->thr && d->table, "cthresh: thr / table must not be NULL");
    CMS_REQUIRE(d->cons.c <= CT_RT_MAX, "cthresh: at most %d classes", CT_RT_MAX);
    return CMS_OK;
}

static CtArgs make_ct_args(const cms_cthresh_desc* d) {
    CtArgs a;
    static_cast<ConsArgs&>(a) = make_cons_args(&d->cons);
    a.thr = d->thr;
    a.table = d->table;
    return a;
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_cthresh_workspace_bytes(const cms_cthresh_desc* d) {
    return d ? cms_consistency_workspace_bytes(&d->cons) : 0;
}

// The fused launch carries the statistics table in static LDS next to tiled_scatter's own: in the band of a few KB below
// TILE_LDS_MAX where the two together would pass the 160 KB of a workgroup it is not offered (the caller runs the pair instead).
// The static LDS of one instantiation is a constant of the build: asked of the runtime once and kept (0 = not known yet; a failed
// query is not kept, the next call asks again).
template <int CT, int LF>
static size_t ct_fused_static_lds() {
    static size_t known = 0;
    if (known == 0) {
        hipFuncAttributes attr;
        if (hipFuncGetAttributes(&attr, (const void*)cons_fused_tiled_kernel<ClassThresh, CT, LF>) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        known = attr.sharedSizeBytes;
    }
    return known;
}

static bool ct_fused_fits(const CtArgs& a) {
    const size_t lds = tile_lds_bytes(a.g.c, a.g.sy, a.g.sx, 3);
    size_t fixed = 0;
    CMS_DISPATCH_C(a.g.c, fixed = a.d.loss_fn == CMS_LOSS_VAR ? ct_fused_static_lds<CT, LOSS_VAR>() : ct_fused_static_lds<CT, -1>());
    return fixed > 0 && lds + fixed <= 160 * 1024;
}

static int ct_fused_tiles(const CtArgs& a) {
    const int tiles = fused_tiles(a.g, 3);
    return tiles > 0 && ct_fused_fits(a) ? tiles : 0;
}

extern "C" int cms_cthresh_fused_supported(const cms_cthresh_desc* d) {
    if (check_ct(d)) return 0;
    return ct_fused_tiles(make_ct_args(d)) > 0 ? 1 : 0;
}

extern "C" int cms_cthresh_fwd(const cms_cthresh_desc* d, void* workspace, double* stats_out, void* stream) {
    int rc = check_ct(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out, "cthresh_fwd: workspace / stats_out NULL");
    cons_launch_fwd<ClassThresh>(make_ct_args(d), (float*)workspace, stats_out, (hipStream_t)stream);
    return launch_status("cms_cthresh_fwd");
}

extern "C" int cms_cthresh_bwd(const cms_cthresh_desc* d, const float* scalars, float* grad_l_stu, void* stream) {
    int rc = check_ct(d);
    if (rc) return rc;
    CMS_REQUIRE(scalars && grad_l_stu, "cthresh_bwd: scalars / grad NULL");
    rc = cons_launch_bwd<ClassThresh>("cthresh_bwd", make_ct_args(d), scalars, grad_l_stu, (hipStream_t)stream);
    return rc ? rc : launch_status("cms_cthresh_bwd");
}

extern "C" int cms_cthresh_fwd_bwd(const cms_cthresh_desc* d, float grad_unit, void* workspace, double* stats_out, float* grad_l_stu,
                                   void* stream) {
    int rc = check_ct(d);
    if (rc) return rc;
    CMS_REQUIRE(workspace && stats_out && grad_l_stu, "cthresh_fwd_bwd: workspace / stats_out / grad NULL");
    const CtArgs a = make_ct_args(d);
    const int tiles = ct_fused_tiles(a);
    CMS_REQUIRE(tiles > 0, "cthresh_fwd_bwd: not available for this geometry / mode (ask cms_cthresh_fused_supported)");
    cons_launch_fused<ClassThresh>(a, tiles, grad_unit, (float*)workspace, stats_out, grad_l_stu, (hipStream_t)stream);
    return launch_status("cms_cthresh_fwd_bwd");
}

extern "C" int cms_cthresh_update(int n_classes, int adaptive, double ema, double floor_v, double ceil_v, double* state, float* thr,
                                  unsigned long long* table, unsigned long long* epoch, void* stream) {
    CMS_REQUIRE(n_classes > 0 && n_classes <= CT_RT_MAX, "cthresh_update: 1..%d classes", CT_RT_MAX);
    CMS_REQUIRE(state && thr && table && epoch, "cthresh_update: NULL argument");
    CMS_REQUIRE(ema >= 0.0 && ema < 1.0 && floor_v <= ceil_v, "cthresh_update: ema must be in [0, 1) and floor <= ceil");
    hipLaunchKernelGGL(ct_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_classes, adaptive, ema, floor_v, ceil_v, state, thr,
                       table, epoch);
    return launch_status("cms_cthresh_update");
}
