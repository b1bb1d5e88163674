// Per-block arithmetic of the Cityscapes converter's downsampling (convert.hip), driven on the host by tests/hostcheck_convert.
// Same conventions as pixel_math.hpp / stage_math.hpp: `__host__ __device__`, no state. Integer arithmetic only.
//
// Reference behaviour restated here (paths relative to the upstream repository):
//   images   convert_cityscapes.py:45      skimage downscale_local_mean(x, (d, d, 1)).astype(uint8): the float64 mean of each
//                                          d x d block, truncated. The mean of d*d bytes is sum / d^2 with sum an integer; where
//                                          it is not whole it is at least 1 / d^2 away from a whole number, far more than the
//                                          rounding of the float64 division, so its truncation is exactly floor(sum / d^2).
//   labels   convert_cityscapes.py:17-24   one-hot, summed over each d x d block, argmax: the most frequent value of the block,
//                                          the LOWEST value among equally frequent ones (argmax takes the first maximum).
//
// Work unit: one GROUP of kCvtGroup consecutive output pixels of one output row. It reads, from each of the d source rows under
// it, one contiguous piece of kCvtGroup * d pixels; consecutive lanes take consecutive groups, so a wave reads one contiguous
// stretch per source row. A piece is loaded as whole 32-bit words where the caller says every piece start is 4-byte aligned
// (`words`) and the group is complete, else byte by byte, and never past `valid` bytes: nothing outside the tensor is touched.
// Bytes sit in the words in memory order (little endian, host and device alike).
#pragma once
#include "pixel_math.hpp"

namespace cms {

constexpr int kCvtGroup = 4;        // output pixels per work unit
constexpr int kCvtMaxD = 8;

// byte k (memory order) of a piece held as words; k is a compile-time constant wherever the loops around it are unrolled
template <int NW>
CMS_HD unsigned cvt_byte(const uint32_t (&q)[NW], int k) {
    return (q[k >> 2] >> (8 * (k & 3))) & 255u;
}

// `valid` <= 4 * NW bytes from p; the bytes beyond `valid` read as 0
template <int NW>
CMS_HD void cvt_load_piece(const uint8_t* p, int valid, bool words, uint32_t (&q)[NW]) {
    if (words && valid == 4 * NW) {
        const uint32_t* p32 = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < NW; ++i) q[i] = p32[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4 * i + b < valid) v |= (uint32_t)p[4 * i + b] << (8 * b);
        q[i] = v;
    }
}

// the first `valid` <= 4 * NW bytes of q to p
template <int NW>
CMS_HD void cvt_store_piece(uint8_t* p, int valid, bool words, const uint32_t (&q)[NW]) {
    if (words && valid == 4 * NW) {
        uint32_t* p32 = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < NW; ++i) p32[i] = q[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4 * i + b < valid) p[4 * i + b] = (uint8_t)(q[i] >> (8 * b));
    }
}

// mean of a d x d block of bytes, truncated
CMS_HD unsigned cvt_block_mean(unsigned sum, unsigned d) { return sum / (d * d); }

// Votes: a candidate value with `votes` occurrences has the key below; the LARGEST key wins -- more votes first, then the
// lower value.
CMS_HD unsigned cvt_vote_key(unsigned votes, unsigned value) { return (votes << 8) | (255u - value); }
CMS_HD unsigned cvt_key_value(unsigned key) { return 255u - (key & 255u); }

// the winner among N values, every index a compile-time constant (N = 4 is the d = 2 vote: sixteen compares in registers)
template <int N>
CMS_HD unsigned cvt_vote_unrolled(const unsigned (&v)[N]) {
    unsigned best = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        unsigned votes = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) votes += v[j] == v[i];
        const unsigned key = cvt_vote_key(votes, v[i]);
        best = key > best ? key : best;
    }
    return cvt_key_value(best);
}

// ---- images: `src` = first byte of the group's piece in the first of its D source rows, rows `row_bytes` apart;
//      npx <= kCvtGroup output pixels are wanted -> their 3 * npx bytes in out (the rest 0)
template <int D>
CMS_HD void cvt_image_group(const uint8_t* src, size_t row_bytes, int npx, bool words, uint32_t (&out)[3 * kCvtGroup / 4]) {
    unsigned sum[kCvtGroup][3] = {};
    for (int r = 0; r < D; ++r) {
        uint32_t q[3 * kCvtGroup * D / 4];
        cvt_load_piece(src + (size_t)r * row_bytes, npx * D * 3, words, q);
#pragma unroll
        for (int g = 0; g < kCvtGroup; ++g)
#pragma unroll
            for (int k = 0; k < D; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) sum[g][c] += cvt_byte(q, (g * D + k) * 3 + c);
    }
#pragma unroll
    for (int i = 0; i < 3 * kCvtGroup / 4; ++i) out[i] = 0;
#pragma unroll
    for (int g = 0; g < kCvtGroup; ++g)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int k = g * 3 + c;
            out[k >> 2] |= cvt_block_mean(sum[g][c], D) << (8 * (k & 3));
        }
}

// ---- labels: as above with one byte per pixel -> npx bytes in out
template <int D>
CMS_HD uint32_t cvt_label_group(const uint8_t* src, size_t row_bytes, int npx, bool words) {
    uint32_t q[D][kCvtGroup * D / 4];
#pragma unroll
    for (int r = 0; r < D; ++r) cvt_load_piece(src + (size_t)r * row_bytes, npx * D, words, q[r]);
    uint32_t out = 0;
    if constexpr (D == 1) {
        out = q[0][0];
    } else if constexpr (D == 2) {
#pragma unroll
        for (int g = 0; g < kCvtGroup; ++g) {
            const unsigned v[4] = {cvt_byte(q[0], 2 * g), cvt_byte(q[0], 2 * g + 1), cvt_byte(q[1], 2 * g), cvt_byte(q[1], 2 * g + 1)};
            out |= cvt_vote_unrolled(v) << (8 * g);
        }
    } else {
        // larger blocks only have to be right: D^2 candidates against D^2 values, the block addressed at run time
        for (int g = 0; g < kCvtGroup; ++g) {
            unsigned best = 0;
            for (int i = 0; i < D * D; ++i) {
                const unsigned vi = cvt_byte(q[i / D], g * D + i % D);
                unsigned votes = 0;
                for (int j = 0; j < D * D; ++j) votes += cvt_byte(q[j / D], g * D + j % D) == vi;
                const unsigned key = cvt_vote_key(votes, vi);
                best = key > best ? key : best;
            }
            out |= cvt_key_value(best) << (8 * g);
        }
    }
    return out;
}

// may pieces that start at `base + row * pitch + 4 * k` be moved as words?
inline bool cvt_words_ok(const void* base, size_t pitch) { return (uintptr_t)base % 4 == 0 && pitch % 4 == 0; }

// ---- work item idx of a batch seen as n * ho output rows of wo pixels (C = 3: images, C = 1: labels): group idx % groups_x of
//      output row idx / groups_x. Source rows D * row ... D * row + D - 1 of the batch lie under output row `row`, because every
//      image has D * ho rows.
template <int D, int C>
CMS_HD void cvt_work_item(const uint8_t* src, uint8_t* dst, size_t idx, int wo, bool in_words, bool out_words) {
    const size_t groups_x = (size_t)(wo + kCvtGroup - 1) / kCvtGroup;
    const size_t in_row = (size_t)wo * D * C, out_row = (size_t)wo * C;
    const size_t row = idx / groups_x;
    const int x0 = (int)(idx - row * groups_x) * kCvtGroup;
    const int npx = wo - x0 < kCvtGroup ? wo - x0 : kCvtGroup;
    const uint8_t* s = src + row * D * in_row + (size_t)x0 * D * C;
    uint8_t* o = dst + row * out_row + (size_t)x0 * C;
    if constexpr (C == 3) {
        uint32_t out[3 * kCvtGroup / 4];
        cvt_image_group<D>(s, in_row, npx, in_words, out);
        cvt_store_piece(o, npx * 3, out_words, out);
    } else {
        const uint32_t out[1] = {cvt_label_group<D>(s, in_row, npx, in_words)};
        cvt_store_piece(o, npx, out_words, out);
    }
}

CMS_HD size_t cvt_work_items(int n, int ho, int wo) { return (size_t)n * ho * ((size_t)(wo + kCvtGroup - 1) / kCvtGroup); }

}  // namespace cms
