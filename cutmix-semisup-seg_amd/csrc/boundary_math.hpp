// Boundary scores (csrc/boundary.hip): descriptor validation, the workspace layout and the per-pixel arithmetic of the Chebyshev
// distance-to-boundary maps and of the two confusion matrices built on them. Everything here is plain C++ / `__host__ __device__`,
// so tests/hostcheck_boundary drives the very code the kernels are made of on the host; the product never runs it there.
//
//   T = truth, P = pred with every void pixel (truth == ignore_index) set to ignore_index
//   D_M(p)   Chebyshev distance from a non-void p to the nearest q outside the H x W array or with M(q) != M(p); stored min(D, 255),
//            0 at void pixels
//   r_M(p)   the same along p's row only (pass 1); D_M(x, y) = min over dy of (M(x, y + dy) == M(x, y) ? max(|dy|, r_M(x, y + dy))
//            : |dy|), rows outside the array giving |dy| (pass 2); both capped at 255, which commutes with min and max. Where the
//            maps are no output of the call, pass 2 caps at the sample's widest band + 1 instead (bd_walk_cap)
//   bcm[d]   (C+1, C+1): every non-void pixel with T, P < C adds 1 at [D_T <= d ? T : C, D_P <= d ? P : C]
//   tcm[d]   (C, C): every such pixel with D_T <= d adds 1 at [T, P]
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/cutmixseg.h"
#include "tta_math.hpp"

namespace cms {

constexpr int kBdBlock = 256;         // threads per workgroup of every pass
constexpr int kBdLanes = 64;          // pixels of a row that pass 1 resolves together (one wavefront)
constexpr int kBdReach = 4;           // chunks pass 1 looks at on either side: 4 * 64 >= 255, the cap
constexpr int kBdCap = 255;           // stored distances are min(D, 255)
constexpr int kBdMaxWidth = 254;      // so every width the counting pass takes tells D <= d from D > d
constexpr int kBdMaxK = 4;            // widths per sample
constexpr int kBdMaxClasses = 64;
constexpr size_t kBdLdsBytes = 65536; // histogram bytes of one workgroup of the counting pass
constexpr int kBdCountBlocks = 256;   // workgroups of the counting pass: every one ends with an atomic per non-empty bin on the same words

inline bool boundary_geometry_ok(int n, int h, int w) { return n >= 1 && h >= 1 && w >= 1 && tta_count_ok(n, h, w); }

// one uint8 map, rounded up so that the next one starts 16-byte aligned
inline size_t boundary_map_bytes(int n, int h, int w) { return ((size_t)n * h * w + 15) / 16 * 16; }

// what pass 1 leaves per pixel for pass 2: one 32-bit word (T, r_T, P, r_P), so that a step of the column walk is one load
inline size_t boundary_rows_bytes(int n, int h, int w) { return ((size_t)n * h * w * sizeof(uint32_t) + 15) / 16 * 16; }

// the row words, then the uint8 distance maps of T and of P (unused where the caller gives its own)
inline size_t boundary_workspace_bytes(int n, int h, int w) {
    return boundary_geometry_ok(n, h, w) ? boundary_rows_bytes(n, h, w) + 2 * boundary_map_bytes(n, h, w) : 0;
}

// histogram bytes one width needs in the counting pass, and how many widths one launch takes
inline size_t boundary_width_bytes(int C) { return ((size_t)(C + 1) * (C + 1) + (size_t)C * C) * sizeof(unsigned int); }
inline int boundary_widths_per_launch(int C, int k) {
    const int fit = (int)(kBdLdsBytes / boundary_width_bytes(C));          // >= 1 for C <= 64 (33284 bytes)
    return fit < k ? fit : k;
}

// NULL when cms_boundary_confusion accepts the descriptor, else what is wrong with it
inline const char* boundary_check(const cms_boundary_desc* d) {
    if (!d) return "NULL descriptor";
    if (!d->truth) return "truth NULL";
    if (!d->pred) return "pred NULL";
    if (!d->workspace) return "workspace NULL";
    if (!d->bcm && !d->tcm && !d->dist_truth && !d->dist_pred) return "nothing to produce (bcm, tcm and both distance outputs NULL)";
    if ((d->bcm || d->tcm) && !d->widths) return "widths NULL";
    if (d->k < 1 || d->k > kBdMaxK) return "1 <= k <= 4 widths";
    if (d->num_classes < 1 || d->num_classes > kBdMaxClasses) return "1 <= num_classes <= 64";
    if (d->n < 1 || d->h < 1 || d->w < 1) return "bad geometry (n, h, w >= 1)";
    if (!tta_count_ok(d->n, d->h, d->w)) return "more than 2^31 - 1 pixels";
    if (((uintptr_t)d->workspace & 15) != 0) return "workspace not 16-byte aligned";
    if (d->workspace_bytes < boundary_workspace_bytes(d->n, d->h, d->w)) return "workspace too small";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------------------ pass 1: rows
struct BdPair {
    int t, p;
};

// T and P at position x of a row; -1, which no value equals, outside it
CMS_HD BdPair bd_row_values(const uint8_t* trow, const uint8_t* prow, long long x, int W, int ignore) {
    BdPair v;
    v.t = v.p = -1;
    if (x >= 0 && x < W) {
        v.t = trow[x];
        v.p = v.t == ignore ? ignore : (int)prow[x];
    }
    return v;
}

// A run of equal values [a, b] is found through two flags per position: f(x) = M(x) != M(x - 1) marks a run's first pixel,
// g(x) = M(x) != M(x + 1) its last. The flags of 64 consecutive positions make one 64-bit word (a ballot in the kernel, a loop on
// the host); bit i is position chunk + i.
constexpr int kBdNone = -1;
CMS_HD int bd_last_at_or_below(unsigned long long m, int lane) {          // highest set bit <= lane, else kBdNone
    m &= ~0ull >> (63 - lane);
    return m ? 63 - __builtin_clzll(m) : kBdNone;
}
CMS_HD int bd_first_at_or_above(unsigned long long m, int lane) {         // lowest set bit >= lane, else kBdNone
    m &= ~0ull << lane;
    return m ? __builtin_ctzll(m) : kBdNone;
}

// The distance along the row from x: `left` / `right` are how far the run's first / last pixel lies from x, kBdNone when none was
// found within kBdReach chunks (then it is more than 255 away).
CMS_HD int bd_row_dist(long long left, long long right) {
    long long r = kBdCap;
    if (left != kBdNone && left + 1 < r) r = left + 1;
    if (right != kBdNone && right + 1 < r) r = right + 1;
    return (int)r;
}

// the word pass 1 writes per pixel: T, r_T, P, r_P from the low byte up
CMS_HD uint32_t bd_pack(int t, int rt, int p, int rp) {
    return (uint32_t)t | (uint32_t)rt << 8 | (uint32_t)p << 16 | (uint32_t)rp << 24;
}

// ------------------------------------------------------------------------------------------------------------------ pass 2: columns
// One step of a walk: `best` so far, the value v walked for, and the (value, row distance) byte pairs of the rows s above and below.
CMS_HD int bd_walk_step(int best, int s, int v, uint32_t up, uint32_t down) {
    const int a = (int)(up & 255u) == v ? (int)(up >> 8 & 255u) : 0, b = (int)(down & 255u) == v ? (int)(down >> 8 & 255u) : 0;
    const int near = a < b ? a : b;
    if (near <= s) return s;                                            // max(s, r) == s, and nothing further out is smaller
    return near < best ? near : best;
}

struct BdDist {
    int t, p;
};

// D_T and D_P at (x, y) from the words of column x: `own` is the pixel's, load(yy) that of row yy (called for 0 <= yy < H only).
// Each walk stops as soon as |dy| reaches its best value so far, so after fewer than `cap` steps; the results are min(D, cap),
// cap <= 255. Both walks share the two loads of a step.
template <class L>
CMS_HD BdDist bd_column_walk(uint32_t own, int y, int H, L load, int cap) {
    const int vt = (int)(own & 255u), vp = (int)(own >> 16 & 255u);
    BdDist best;
    best.t = (int)(own >> 8 & 255u), best.p = (int)(own >> 24);
    best.t = best.t < cap ? best.t : cap, best.p = best.p < cap ? best.p : cap;
    for (int s = 1; s < best.t || s < best.p; ++s) {
        if (y - s < 0 || H - 1 - y < s) {                               // a row outside the array: |dy|
            best.t = s < best.t ? s : best.t, best.p = s < best.p ? s : best.p;
            break;
        }
        const uint32_t up = load(y - s), down = load(y + s);
        if (s < best.t) best.t = bd_walk_step(best.t, s, vt, up, down);
        if (s < best.p) best.p = bd_walk_step(best.p, s, vp, up >> 16, down >> 16);
    }
    return best;
}

// ------------------------------------------------------------------------------------------------------------------ pass 3: counts
CMS_HD int bd_clamp_width(int d) { return d < 1 ? 1 : (d > kBdMaxWidth ? kBdMaxWidth : d); }

// Where nobody asks for the distance maps, pass 2 need not tell distances beyond the widest band of the sample apart: with
// cap = that width + 1, min(D, cap) <= d exactly when D <= d for every width d of the sample. 255 when the maps are an output.
CMS_HD int bd_walk_cap(const int32_t* widths, int k, bool maps_wanted) {
    if (maps_wanted || !widths) return kBdCap;
    int widest = 1;
    for (int j = 0; j < k; ++j) {
        const int d = bd_clamp_width(widths[j]);
        widest = d > widest ? d : widest;
    }
    return widest + 1;
}

// does a pixel count at all? (t, p: T and P there, as cms_confusion drops values that are no class)
CMS_HD bool bd_counted(int t, int p, int ignore, int C) { return t != ignore && t < C && p < C; }

CMS_HD int bd_bcm_bin(int t, int p, int dt, int dp, int d, int C) { return (dt <= d ? t : C) * (C + 1) + (dp <= d ? p : C); }

CMS_HD int bd_tcm_bin(int t, int p, int dt, int d, int C) { return dt <= d ? t * C + p : -1; }

}  // namespace cms
