// TEST INFRASTRUCTURE (never shipped, never imported by the product package).
//
// Drives the `__host__ __device__` per-pixel arithmetic of cutmix-semisup-seg_amd/csrc/ict_math.hpp -- the code the ICT
// kernels inline -- in plain host loops over every pixel, with the upsampling done by bilin_tap / bilin_gather, so that the
// formulas (blends, blended confidence, the five losses on blended targets and their analytic gradients, the batch-mean
// confidence weight of --conf_per_pixel) can be checked against tests/_ict_refs.py on a CPU-only machine. The kernels'
// indexing, reductions and LDS tiling are covered by the `-m gpu` tests.
//
// Build: tests/_hostcheck.py (shared object for the tests; `--sanitize`: the stand-alone driver below under ASan + UBSan).
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../cutmix-semisup-seg_amd/csrc/ict_math.hpp"

using namespace cms;

namespace {

struct HostGather {
    const float* base;
    size_t plane;
    int w_in;
    Tap ty, tx;
    float operator()(int c) const { return bilin_gather(base + c * plane, w_in, ty, tx); }
};

template <int CT>
struct HostRegs {
    float v[CT > 0 ? CT : 1];
    float operator()(int c) const { return v[c]; }
};

struct Problem {
    const float *l_stu, *l_t0, *l_t1, *lam, *um0, *um1;
    int n, c, h, w, H, W, align, loss_fn;
    float tau;
    int per_pixel;
};

// CT > 0: the class axis in a register-like array, as the kernels' compile-time instantiations; CT == 0: re-gathering callables
template <int CT>
void run(const Problem& q, double* stats, float gscale, float* grad) {
    const float sy = bilin_scale(q.h, q.H, q.align != 0), sx = bilin_scale(q.w, q.W, q.align != 0);
    const size_t plane = (size_t)q.h * q.w;
    const float inv_root_c = (float)(1.0 / sqrt((double)q.c));
    const bool thresh = q.tau > 0.0f, use_map = thresh && q.per_pixel;
    stats[0] = stats[1] = stats[2] = 0.0;
    auto gathers = [&](int i, int y, int x, HostGather& gs, HostGather& g0, HostGather& g1) {
        gs.base = q.l_stu + (size_t)i * q.c * plane;
        g0.base = q.l_t0 + (size_t)i * q.c * plane;
        g1.base = q.l_t1 + (size_t)i * q.c * plane;
        gs.plane = g0.plane = g1.plane = plane;
        gs.w_in = g0.w_in = g1.w_in = q.w;
        gs.ty = g0.ty = g1.ty = bilin_tap(y, sy, q.h, q.align != 0);
        gs.tx = g0.tx = g1.tx = bilin_tap(x, sx, q.w, q.align != 0);
    };
    auto regs = [&](const HostGather& g, HostRegs<CT>& r) {
        for (int c = 0; c < CT; ++c) r.v[c] = g(c);
    };
    // first pass of --conf_per_pixel: the (H,W) map of sum_i [conf(i,y,x) >= tau]
    std::vector<float> cmap;
    if (use_map) {
        cmap.assign((size_t)q.H * q.W, 0.0f);
        for (int i = 0; i < q.n; ++i)
            for (int y = 0; y < q.H; ++y)
                for (int x = 0; x < q.W; ++x) {
                    HostGather gs, g0, g1;
                    gathers(i, y, x, gs, g0, g1);
                    float conf;
                    if (CT > 0) {
                        HostRegs<CT> r0, r1;
                        regs(g0, r0);
                        regs(g1, r1);
                        conf = ict_conf<CT>(r0, r1, q.lam[i], q.c);
                    } else {
                        conf = ict_conf<0>(g0, g1, q.lam[i], q.c);
                    }
                    if (conf >= q.tau) cmap[(size_t)y * q.W + x] += 1.0f;
                }
    }
    std::vector<float> gv(q.c);
    for (int i = 0; i < q.n; ++i) {
        const float lam = q.lam[i];
        for (int y = 0; y < q.H; ++y)
            for (int x = 0; x < q.W; ++x) {
                const size_t yx = (size_t)y * q.W + x, pix = (size_t)i * q.H * q.W + yx;
                HostGather gs, g0, g1;
                gathers(i, y, x, gs, g0, g1);
                HostRegs<CT> rs, r0, r1;
                if (CT > 0) {
                    regs(gs, rs);
                    regs(g0, r0);
                    regs(g1, r1);
                }
                const PixelFwd r = CT > 0 ? ict_pixel_fwd<CT>(rs, r0, r1, lam, q.c, q.loss_fn, inv_root_c)
                                          : ict_pixel_fwd<0>(gs, g0, g1, lam, q.c, q.loss_fn, inv_root_c);
                const float um = ict_mix(q.um0 ? q.um0[pix] : 1.0f, q.um1 ? q.um1[pix] : 1.0f, 1.0f - lam, lam);
                const float cf = (thresh && r.conf >= q.tau) ? 1.0f : 0.0f;
                const float wgt = use_map ? cmap[yx] / (float)q.n : cf;
                const float lm = r.loss * um;
                stats[0] += (double)lm;
                stats[1] += (double)(lm * wgt);
                stats[2] += cf;
                if (grad) {
                    auto keep = [&](int k, float v) { gv[k] = v; };
                    if (CT > 0) ict_pixel_bwd<CT>(rs, r0, r1, lam, q.c, q.loss_fn, inv_root_c, keep);
                    else ict_pixel_bwd<0>(gs, g0, g1, lam, q.c, q.loss_fn, inv_root_c, keep);
                    float f = gscale * um;
                    if (use_map) f *= cmap[yx] / (float)q.n;
                    float* gp = grad + (size_t)i * q.c * plane;
                    for (int k = 0; k < q.c; ++k) {
                        const float g = f * gv[k];
                        gp[k * plane + (size_t)gs.ty.i0 * q.w + gs.tx.i0] += gs.ty.w0 * gs.tx.w0 * g;
                        gp[k * plane + (size_t)gs.ty.i0 * q.w + gs.tx.i1] += gs.ty.w0 * gs.tx.w1 * g;
                        gp[k * plane + (size_t)gs.ty.i1 * q.w + gs.tx.i0] += gs.ty.w1 * gs.tx.w0 * g;
                        gp[k * plane + (size_t)gs.ty.i1 * q.w + gs.tx.i1] += gs.ty.w1 * gs.tx.w1 * g;
                    }
                }
            }
    }
}

}  // namespace

extern "C" {

// out = x0 * (1 - lam[i]) + x1 * lam[i] per sample of chw elements (the arithmetic of cms_ict_blend in fp32)
void hc_ict_blend(const float* x0, const float* x1, float* out, const float* lam, int n, size_t chw) {
    for (int i = 0; i < n; ++i)
        for (size_t e = 0; e < chw; ++e) out[i * chw + e] = ict_mix(x0[i * chw + e], x1[i * chw + e], 1.0f - lam[i], lam[i]);
}

// stats[3] = {sum loss*um, sum loss*um*weight, count(conf >= tau)} with weight = the batch-mean indicator at the pixel position
// (per_pixel) or the pixel's own indicator; if grad != NULL also accumulates gscale * um [* weight, per_pixel] * d loss / d l_stu
void hc_ict(const float* l_stu, const float* l_t0, const float* l_t1, const float* lam, const float* um0, const float* um1, int n,
            int c, int h, int w, int H, int W, int align, int loss_fn, float tau, int per_pixel, double* stats, float gscale,
            float* grad) {
    Problem q = {l_stu, l_t0, l_t1, lam, um0, um1, n, c, h, w, H, W, align, loss_fn, tau, per_pixel};
    switch (c) {
        case 2: run<2>(q, stats, gscale, grad); break;
        case 5: run<5>(q, stats, gscale, grad); break;
        default: run<0>(q, stats, gscale, grad); break;
    }
}

}  // extern "C"

#ifdef HC_ICT_MAIN
// Stand-alone driver for the sanitizers: every loss x mode x class path on a small upsampling geometry with lambda rows 0, 1
// and interior values; fails on a non-finite sum.
#include <stdio.h>
int main() {
    const int n = 3, h = 6, w = 7, H = 41, W = 50;
    const float lam[3] = {0.0f, 1.0f, 0.37f};
    uint32_t seed = 12345u;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) / 16777216.0f * 2.0f - 1.0f;
    };
    int bad = 0;
    for (int c : {2, 5, 7}) {
        std::vector<float> ls((size_t)n * c * h * w), l0(ls.size()), l1(ls.size()), um0((size_t)n * H * W), um1(um0.size());
        for (auto& v : ls) v = 2.0f * rnd();
        for (auto& v : l0) v = 3.0f * rnd();
        for (auto& v : l1) v = 3.0f * rnd();
        for (auto& v : um0) v = rnd() > -0.4f ? 1.0f : 0.0f;
        for (auto& v : um1) v = rnd() > -0.4f ? 1.0f : 0.0f;
        std::vector<float> mix(um0.size());
        hc_ict_blend(um0.data(), um1.data(), mix.data(), lam, n, (size_t)H * W);
        for (int fn = 0; fn < 5; ++fn)
            for (int mode = 0; mode < 3; ++mode)
                for (int align = 0; align < 2; ++align) {
                    std::vector<float> grad(ls.size(), 0.0f);
                    double stats[3];
                    hc_ict(ls.data(), l0.data(), l1.data(), lam, mode == 2 ? nullptr : um0.data(), mode == 2 ? nullptr : um1.data(), n, c,
                           h, w, H, W, align, fn, mode == 2 ? 0.0f : 0.6f, mode == 1, stats, 1.0f / (n * H * W), grad.data());
                    double gs = 0.0;
                    for (float v : grad) gs += v;
                    if (!(stats[0] == stats[0]) || !(gs == gs)) ++bad;
                }
    }
    printf("hostcheck_ict: %s\n", bad ? "NON-FINITE RESULT" : "ok");
    return bad ? 1 : 0;
}
#endif
