// What the kernels of the masked consistency loss (cons_kernels.hpp: one body for the scalar threshold of losses.hip and the
// per-class thresholds of cthresh.hip) are built on: the kernel argument block, the per-pixel inputs (mask bit, validity, which
// teacher) and the staging of a tile's logit rectangles.
#pragma once
#include "loss_tiles.hpp"

namespace cms {

struct ConsArgs {
    cms_consistency_desc d;
    Geo g;
    float tau, inv_root_c;
};

struct ConsPixel {
    bool m;
    float um;
    const float* tea;
    int which;          // 0: l_tea0, 1: l_tea1 -- for callers that read the teacher logits from an LDS copy
};

__device__ __forceinline__ ConsPixel cons_pixel_inputs(const ConsArgs& a, int n, int y, int x) {
    const cms_consistency_desc& d = a.d;
    const size_t pix = ((size_t)n * d.H + y) * d.W + x;
    ConsPixel p;
    if (d.mask) {
        p.m = d.mask[pix] >= 0.5f;
    } else {
        p.m = box_mask_bit(d.ranges + (size_t)n * d.n_boxes * 4, d.n_boxes, y, x, d.invert != 0);
    }
    const size_t sample = (size_t)n * d.c * d.h * d.w;
    if (d.mode == MODE_MIX) {
        // paste of teacher logits and of the validity masks with the same box mask (:351, :363)
        p.tea = (p.m ? d.l_tea1 : d.l_tea0) + sample;
        p.which = p.m ? 1 : 0;
        const float* um = p.m ? d.um1 : d.um0;
        p.um = um ? um[pix] : 1.0f;
    } else {
        // cut mode: loss_mask = cut_mask * um (:401)
        p.tea = d.l_tea0 + sample;
        p.which = 0;
        p.um = p.m ? (d.um0 ? d.um0[pix] : 1.0f) : 0.0f;
    }
    return p;
}

// student | teacher 0 | teacher 1 rectangles of a tile, `pstride` floats apart
__device__ __forceinline__ void cons_stage(const ConsArgs& a, int n, const Patch& p, float* P, int pstride) {
    const Geo& g = a.g;
    const size_t plane = (size_t)g.h * g.w, sample = (size_t)n * g.c * plane;
    stage_patch(P, a.d.l_stu + sample, g.c, plane, g.w, p);
    stage_patch(P + pstride, a.d.l_tea0 + sample, g.c, plane, g.w, p);
    if (a.d.mode == MODE_MIX) stage_patch(P + 2 * pstride, a.d.l_tea1 + sample, g.c, plane, g.w, p);
}

// the checks of a consistency descriptor and its kernel arguments (defined in losses.hip)
int check_cons(const cms_consistency_desc* d);
ConsArgs make_cons_args(const cms_consistency_desc* d);

}  // namespace cms
