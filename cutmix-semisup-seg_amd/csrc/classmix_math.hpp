// ClassMix masks (csrc/classmix.hip): descriptor validation, the launch geometry and the per-pixel / per-sample arithmetic.
// Everything here is plain C++ / `__host__ __device__`, so tests/hostcheck_classmix drives the very code the kernels are made of on
// the host; the product never runs it there. The prediction is tta_math.hpp's single-view pixel (taps, gathers and the argmax
// order of pixel_math.hpp / tta_math.hpp, under their `fp contract(off)` discipline): nothing of it is restated here.
//
//   pred(n,y,x)   argmax_c of the bilinear sample of logits[n,c] (first index keeps a tie, NaN counts as maximal)
//   present_n     bit c set iff some pixel with valid != 0 has pred == c (every pixel without `valid`)
//   chosen_n      the k = (m + 1) / 2 classes of present_n (m = popcount) that come first in the order (keys[n,c], c)
//   mask(n,y,x)   1.0f if valid != 0 and bit pred of chosen_n is set, else 0.0f
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/cutmixseg.h"
#include "tta_math.hpp"

namespace cms {

constexpr int kCmBlock = 256;          // threads per workgroup of both passes
constexpr int kCmMaxSlots = 256;       // words of a sample's slot table: one per workgroup of pass 1
constexpr int kCmMaxSamples = 65535;   // blockIdx.y is the sample

// Pixels per workgroup of pass 1: a multiple of 4 * kCmBlock, at least 1024, and large enough that a sample has at most
// kCmMaxSlots workgroups (pass 2 ORs that many words per workgroup: four per lane of one wave). 1024 pixels, four per thread, is
// what keeps the gathers of pass 1 in flight: with at most 64 slots a batch of 4 x 512 x 1024 was 256 workgroups, one per CU, and
// the pair took 0.108 ms against 0.041 ms of the single-view vote. hw <= 2^31 - 1, so this fits an int (<= 2^23).
inline int classmix_chunk(long long hw) {
    const long long per_slot = (long long)kCmMaxSlots * kCmBlock;
    long long ppt = (hw + per_slot - 1) / per_slot;
    if (ppt < 4) ppt = 4;
    ppt = (ppt + 3) / 4 * 4;
    return (int)(ppt * kCmBlock);
}

inline int classmix_slots(long long hw) {
    const long long chunk = classmix_chunk(hw);
    return (int)((hw + chunk - 1) / chunk);
}

inline bool classmix_geometry_ok(int n, int H, int W) {
    return n >= 1 && H >= 1 && W >= 1 && n <= kCmMaxSamples && tta_count_ok(n, H, W);
}

// [n][kCmMaxSlots] 64-bit slot words, then n * H * W uint8 predictions (used when the caller gives no pred_out), rounded up to 16
inline size_t classmix_pred_offset(int n) { return (size_t)n * kCmMaxSlots * sizeof(unsigned long long); }

inline size_t classmix_workspace_bytes(int n, int H, int W) {
    if (!classmix_geometry_ok(n, H, W)) return 0;
    const size_t pix = (size_t)n * H * W;
    return classmix_pred_offset(n) + (pix + 15) / 16 * 16;
}

// NULL when cms_classmix accepts the descriptor, else what is wrong with it
inline const char* classmix_check(const cms_classmix_desc* d) {
    if (!d) return "NULL descriptor";
    if (!d->logits) return "logits NULL";
    if (!d->keys) return "keys NULL";
    if (!d->mask_out) return "mask_out NULL";
    if (!d->workspace) return "workspace NULL";
    if (d->c < 1 || d->c > kTtaMaxClasses) return "1 <= num_classes <= 64";
    if (d->n < 1 || d->h < 1 || d->w < 1 || d->H < 1 || d->W < 1) return "bad geometry (n, h, w, H, W >= 1)";
    if (d->n > kCmMaxSamples) return "more than 65535 samples";
    if (!tta_count_ok(d->n, d->H, d->W)) return "more than 2^31 - 1 output pixels";
    if (!tta_count_ok(d->n, d->c, d->h, d->w)) return "more than 2^31 - 1 logits";
    if (((uintptr_t)d->workspace & 15) != 0) return "workspace not 16-byte aligned";
    if (d->workspace_bytes < classmix_workspace_bytes(d->n, d->H, d->W)) return "workspace too small";
    return nullptr;
}

// the one view of the prediction: the descriptor's logits at its sizes, unflipped
inline void classmix_views(const cms_classmix_desc* d, TtaViews* v) {
    cms_tta_desc t;
    memset(&t, 0, sizeof(t));
    t.logits[0] = d->logits;
    t.h[0] = d->h, t.w[0] = d->w, t.flip[0] = 0;
    t.n = d->n, t.c = d->c, t.H = d->H, t.W = d->W, t.k = 1, t.align_corners = d->align_corners;
    tta_make_views(&t, v);
}

// what one pixel contributes to its sample's set of present classes (pred <= 63: the shift is 64 bits wide)
CMS_HD unsigned long long classmix_bit(int pred, bool valid) { return valid ? 1ull << pred : 0ull; }

// how many of the m present classes are chosen: ceil(m / 2)
CMS_HD int classmix_keep(unsigned long long present) { return (__builtin_popcountll(present) + 1) / 2; }

// The rank of class c among the present classes in the order (key, class index): the number of present c' that come before it.
// `key(c')` is the key of class c' (a pointer read on the host, a column of LDS in the kernel).
template <class K>
CMS_HD int classmix_rank(unsigned long long present, K key, int C, int c) {
    const double kc = key(c);
    int rank = 0;
    for (int o = 0; o < C; ++o) {
        if (!((present >> o) & 1ull)) continue;
        const double ko = key(o);
        rank += (ko < kc || (ko == kc && o < c)) ? 1 : 0;
    }
    return rank;
}

// is class c chosen? (lane c of one wave in the kernel, a loop on the host)
template <class K>
CMS_HD bool classmix_is_chosen(unsigned long long present, K key, int C, int c) {
    return c < C && ((present >> c) & 1ull) != 0 && classmix_rank(present, key, C, c) < classmix_keep(present);
}

CMS_HD float classmix_mask_value(unsigned long long chosen, int pred, bool valid) {
    return (valid && ((chosen >> pred) & 1ull) != 0) ? 1.0f : 0.0f;
}

// Pass 2 writes a sample's mask as 16-byte stores where the FLAT element index (over the whole (n, H, W) tensor) is a multiple of
// four, whatever H * W is: the sample's elements [start, end) split into a head [start, vec_lo), whole groups of four
// [vec_lo, vec_hi) and a tail [vec_hi, end); head and tail hold at most three elements each (a sample of fewer than four pixels
// may have no group at all).
struct CmSplit {
    size_t vec_lo, vec_hi;
};

CMS_HD CmSplit classmix_split(size_t start, size_t end) {
    const size_t up = (start + 3) / 4 * 4, down = end / 4 * 4;
    CmSplit s;
    s.vec_lo = up < end ? up : end;
    s.vec_hi = down > s.vec_lo ? down : s.vec_lo;
    return s;
}

}  // namespace cms
