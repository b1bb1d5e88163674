// Surface distances (csrc/surface.hip): descriptor validation, the workspace layout and the per-pixel arithmetic of the exact squared
// Euclidean distances between the class surfaces of a truth and a prediction map, and of the per-(sample, class) reduction built on
// them. Everything here is plain C++ / `__host__ __device__`, so tests/hostcheck_surface drives the very code the kernels are made of
// on the host; the product never runs it there.
//
//   T = truth with void pixels (truth == ignore_index) as -1, P = pred with the same pixels as -1; a value >= C is no class either
//   surface   a class pixel p of map M is on the surface of its class when one of its FOUR edge neighbours lies outside the H x W
//             array or has M(q) != M(p). Every pixel is on the surface of at most one class per map: one byte per pixel and map
//             holds that class, kSfNoClass elsewhere (pass 1, which also counts the surface pixels per sample and class)
//   r_c(x, y) for map M and class c, the distance along row y from x to the nearest surface pixel of c, kSfNoRow when the row has
//             none; uint16, one plane per map, sample and class, written only for the scored pairs (pass 2)
//   d2(p)     for a surface pixel p = (x, y) of class c in one map: min over dy of dy^2 + r_c(x, y + dy)^2 in the other map; the walk
//             over dy = 1, 2, ... stops as soon as dy^2 >= the best value so far, so it is exact and bounded by the answer (pass 3)
//   reduction per scored pair, over fixed slabs of the sample: the two maxima and the two fp64 sums of sqrt(d2), partial per slab and
//             summed in slab order (pass 4), then the values of ranks lo and hi of the pooled multiset by a radix select, 8-bit
//             digits from the top (pass 5); a digit above the largest value's top bit is 0 and its pass is skipped
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/cutmixseg.h"
#include "boundary_math.hpp"

namespace cms {

constexpr int kSfBlock = 256;            // threads per workgroup of every pass
constexpr int kSfLanes = 64;             // pixels of a row that pass 2 resolves together (one wavefront)
constexpr int kSfMaxClasses = 64;
constexpr int kSfMaxSide = 16384;        // so that every d2 <= 2 * 16383^2 < 2^30
constexpr int kSfNoClass = 255;          // the surface byte of a pixel on no class's surface
constexpr int kSfNoRow = 0xFFFF;         // the row distance of a row without a surface pixel of the class
constexpr int32_t kSfFar = 0x7FFFFFFF;   // "no distance yet"
constexpr int kSfSlabPixels = 4096;      // pixels of a sample one workgroup of the reduction takes, until there are kSfMaxSlabs
constexpr int kSfMaxSlabs = 64;
constexpr int kSfMarkBlocks = 256;       // workgroups per sample of pass 1, at most

struct SfState {                         // one per (sample, class), in the workspace
    int32_t max_d2;                      // the larger of the two directed maxima; -1: the pair is not scored
    uint32_t prefix[2];                  // the bits of a[lo] / a[hi] found so far
    uint32_t remaining[2];               // rank of a[lo] / a[hi] among the values that share the prefix
    uint32_t pad[3];
};

struct SfPartial {                       // one per (sample, class, slab)
    double sum[2];                       // sum of sqrt(d2) over the slab's surface pixels of P / of T
    int32_t max_d2[2];
    int32_t pad[2];
};

inline size_t sf_align(size_t b) { return (b + 15) / 16 * 16; }

// slabs of a sample in the reduction: a function of the geometry alone, so the order of every sum is
CMS_HD int sf_slabs(int h, int w) {
    const long long hw = (long long)h * w, s = (hw + kSfSlabPixels - 1) / kSfSlabPixels;
    return (int)(s < 1 ? 1 : (s > kSfMaxSlabs ? kSfMaxSlabs : s));
}
CMS_HD long long sf_slab_len(int h, int w) {
    const long long hw = (long long)h * w, s = sf_slabs(h, w);
    return (hw + s - 1) / s;
}

// the last condition keeps the reduction's grid, a workgroup per (sample, class, slab), below 2^31
inline bool surface_geometry_ok(int n, int h, int w, int c) {
    return n >= 1 && h >= 1 && w >= 1 && h <= kSfMaxSide && w <= kSfMaxSide && c >= 1 && c <= kSfMaxClasses && tta_count_ok(n, h, w) &&
           tta_count_ok(n, c, sf_slabs(h, w));
}

// The workspace, in this order, every part 16-byte aligned:
//   counts   (n, C, 2) int32: surface pixels of P / of T        } zeroed by one memset per call
//   hist     (n, C, 2, 256) uint32: the select's digit counts   }
//   state    (n, C) SfState
//   partial  (n, C, slabs) SfPartial
//   surf     2 x (n, h, w) uint8: the surface class of T, of P
//   d2       2 x (n, h, w) int32: d2_pred, d2_truth (unused where the caller gives its own)
//   rows     2 x (n, C, h, w) uint16: r_c in T, in P
struct SfLayout {
    size_t counts, hist, state, partial, surf, d2, rows, total, zeroed, map, d2map, plane;
};
inline SfLayout surface_layout(int n, int h, int w, int c) {
    SfLayout l;
    const size_t nc = (size_t)n * c, pix = (size_t)n * h * w;
    l.map = sf_align(pix), l.d2map = sf_align(pix * sizeof(int32_t)), l.plane = sf_align(pix * c * sizeof(uint16_t));
    l.counts = 0;
    l.hist = l.counts + sf_align(nc * 2 * sizeof(int32_t));
    l.state = l.hist + sf_align(nc * 2 * 256 * sizeof(uint32_t));
    l.zeroed = l.state;
    l.partial = l.state + sf_align(nc * sizeof(SfState));
    l.surf = l.partial + sf_align(nc * sf_slabs(h, w) * sizeof(SfPartial));
    l.d2 = l.surf + 2 * l.map;
    l.rows = l.d2 + 2 * l.d2map;
    l.total = l.rows + 2 * l.plane;
    return l;
}
inline size_t surface_workspace_bytes(int n, int h, int w, int c) {
    return surface_geometry_ok(n, h, w, c) ? surface_layout(n, h, w, c).total : 0;
}

// NULL when cms_surface_distances accepts the descriptor, else what is wrong with it
inline const char* surface_check(const cms_surface_desc* d) {
    if (!d) return "NULL descriptor";
    if (!d->truth) return "truth NULL";
    if (!d->pred) return "pred NULL";
    if (!d->workspace) return "workspace NULL";
    if (!d->stats && !d->sums && !d->d2_pred && !d->d2_truth) return "nothing to produce (stats, sums and both d2 outputs NULL)";
    if (d->num_classes < 1 || d->num_classes > kSfMaxClasses) return "1 <= num_classes <= 64";
    if (d->n < 1 || d->h < 1 || d->w < 1) return "bad geometry (n, h, w >= 1)";
    if (d->h > kSfMaxSide || d->w > kSfMaxSide) return "h and w at most 16384";
    if (!tta_count_ok(d->n, d->h, d->w)) return "more than 2^31 - 1 pixels";
    if (!tta_count_ok(d->n, d->num_classes, sf_slabs(d->h, d->w))) return "more than 2^31 - 1 (sample, class, slab) triples";
    if (((uintptr_t)d->workspace & 15) != 0) return "workspace not 16-byte aligned";
    if (d->workspace_bytes < surface_workspace_bytes(d->n, d->h, d->w, d->num_classes)) return "workspace too small";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------------------ pass 1: surfaces
struct SfPair {
    int t, p;
};

// T and P at (x, y) of a sample whose first pixel is truth / pred; -1, which no class equals, outside the array and at void pixels
CMS_HD SfPair sf_values(const uint8_t* truth, const uint8_t* pred, int x, int y, int H, int W, int ignore) {
    SfPair v;
    v.t = v.p = -1;
    if (x >= 0 && x < W && y >= 0 && y < H) {
        const size_t i = (size_t)y * W + x;
        const int t = truth[i];
        if (t != ignore) v.t = t, v.p = pred[i];
    }
    return v;
}

// the surface bytes of T and of P at (x, y): the pixel's class when it is one and a 4-neighbour differs, else kSfNoClass
CMS_HD SfPair sf_surface(const uint8_t* truth, const uint8_t* pred, int x, int y, int H, int W, int ignore, int C) {
    const SfPair o = sf_values(truth, pred, x, y, H, W, ignore);
    const SfPair l = sf_values(truth, pred, x - 1, y, H, W, ignore), r = sf_values(truth, pred, x + 1, y, H, W, ignore);
    const SfPair u = sf_values(truth, pred, x, y - 1, H, W, ignore), b = sf_values(truth, pred, x, y + 1, H, W, ignore);
    SfPair s;
    s.t = (o.t >= 0 && o.t < C && (l.t != o.t || r.t != o.t || u.t != o.t || b.t != o.t)) ? o.t : kSfNoClass;
    s.p = (o.p >= 0 && o.p < C && (l.p != o.p || r.p != o.p || u.p != o.p || b.p != o.p)) ? o.p : kSfNoClass;
    return s;
}

// a pair is scored when both masks are non-empty, which is when both surfaces are
CMS_HD bool sf_scored(const int32_t* counts /* of the pair: P, T */) { return counts[0] > 0 && counts[1] > 0; }

// ------------------------------------------------------------------------------------------------------------------ pass 2: rows
// The flags "surface pixel of class c" of 64 consecutive positions of a row make one 64-bit word (a ballot in the kernel, a loop on
// the host); bit i is position chunk + i. A sweep from the left carries the position of the last surface pixel of the chunks before
// (`last`, -1 for none), a sweep from the right that of the first one of the chunks after (`next`).
CMS_HD int sf_row_left(unsigned long long m, int lane, int x, int last) {
    const int i = bd_last_at_or_below(m, lane);
    return i != kBdNone ? lane - i : (last >= 0 ? x - last : kSfNoRow);
}
CMS_HD int sf_row_right(unsigned long long m, int lane, int x, int next) {
    const int i = bd_first_at_or_above(m, lane);
    return i != kBdNone ? i - lane : (next >= 0 ? next - x : kSfNoRow);
}
CMS_HD int sf_carry_last(unsigned long long m, int chunk, int last) { return m ? chunk + 63 - __builtin_clzll(m) : last; }
CMS_HD int sf_carry_next(unsigned long long m, int chunk, int next) { return m ? chunk + __builtin_ctzll(m) : next; }

// ------------------------------------------------------------------------------------------------------------------ pass 3: columns
// d2 at (x, y) from the row distances of column x in the other map's plane of the pixel's class: `own` is row y's, load(yy) that of
// row yy (called for 0 <= yy < H only). kSfFar when no row of the plane has a surface pixel, which no scored pair has.
template <class L>
CMS_HD int32_t sf_column_walk(int own, int y, int H, L load) {
    int32_t best = own == kSfNoRow ? kSfFar : own * own;
    for (int dy = 1; dy * dy < best; ++dy) {
        const bool up = y - dy >= 0, down = y + dy < H;
        if (!up && !down) break;
        if (up) {
            const int r = load(y - dy);
            if (r != kSfNoRow && dy * dy + r * r < best) best = dy * dy + r * r;
        }
        if (down) {
            const int r = load(y + dy);
            if (r != kSfNoRow && dy * dy + r * r < best) best = dy * dy + r * r;
        }
    }
    return best;
}

// ------------------------------------------------------------------------------------------------------------------ passes 4, 5
// the sum of kSfBlock values in a fixed tree order (v is overwritten; in the kernel every step is a barrier apart)
CMS_HD void sf_tree_step(double* v, int32_t* m, int t, int stride) {
    v[t] += v[t + stride];
    m[t] = m[t + stride] > m[t] ? m[t + stride] : m[t];
}

// ranks of the pooled multiset of m >= 1 values behind the 95th percentile with linear interpolation
CMS_HD unsigned long long sf_rank_lo(unsigned long long m) { return 19ull * (m - 1) / 20ull; }
CMS_HD unsigned long long sf_rank_hi(unsigned long long m) { return sf_rank_lo(m) + 1 < m ? sf_rank_lo(m) + 1 : m - 1; }

// does value v still share the prefix above digit `shift`?
CMS_HD bool sf_in_prefix(uint32_t v, uint32_t prefix, int shift) { return shift >= 24 || (v >> (shift + 8)) == (prefix >> (shift + 8)); }

// a pass of the select whose digit is 0 for every value of the pair is skipped by both of its kernels
CMS_HD bool sf_pass_skipped(int32_t max_d2, int shift) { return max_d2 < 0 || (shift > 0 && ((uint32_t)max_d2 >> shift) == 0); }

// pick the digit that holds rank `remaining` (0-based) among the counted values; -> the digit, `remaining` made relative to it
CMS_HD int sf_pick_digit(const uint32_t* hist, uint32_t* remaining) {
    uint32_t seen = 0;
    for (int d = 0; d < 256; ++d) {
        const uint32_t c = hist[d];
        if (*remaining < seen + c || d == 255) {
            *remaining -= seen;
            return d;
        }
        seen += c;
    }
    return 255;
}

}  // namespace cms
