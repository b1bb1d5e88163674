// Arithmetic of the ISIC 2017 converter's area resize and image statistics (resize.hip), driven on the host by
// tests/hostcheck_resize. Same conventions as convert_math.hpp: `__host__ __device__`, no state. Integer arithmetic only.
//
// The definition (the project's own; the reference calls cv2.resize(..., interpolation=cv2.INTER_AREA) at convert_isic.py:56-60,
// which is not consulted -- see DESIGN section 8 for the deviations). Along an axis of L source pixels and Lo <= L output cells,
// in units of 1 / Lo pixel:
//     source pixel i covers [i * Lo, (i + 1) * Lo),   output cell o covers [o * L, (o + 1) * L),
//     wt(o, i) = the length of the overlap.
// The weights of a cell sum to L, those of a pixel to Lo, and a pixel has weight in at most two cells. Then
//     num(oy, ox, ch) = sum_iy sum_ix wy(oy, iy) * wx(ox, ix) * p(iy, ix, ch),      out = num / (h * w), ties to even.
// With sides <= 16384: sum_iy wy * p <= 255 * h < 2^22 (32 bits), num <= 255 * 2^28 < 2^36 (64 bits).
//
// Work unit: one output row of one image and one SEGMENT of `seg` consecutive output columns, run by a workgroup of kRszThreads
// threads. The source bytes under the segment are walked in CHUNKS of kRszChunk bytes of the row:
//   phase 1   thread t owns kRszPerThread byte columns of the chunk and sums wy * p over the source rows under the output row
//             (rsz_column_sums), then hands its sums over in a chunk-sized array (LDS on the device);
//   phase 2   thread t < seg * c owns output (ox, ch) and adds wx * column sum over the columns of its cell that lie in the chunk
//             (rsz_add_chunk); after the last chunk it rounds (rsz_round_div) and stores its byte.
// A chunk starts at a multiple of four bytes of the row. Where the base and the row pitch are on four bytes (`words`) a thread's
// columns are four consecutive 32-bit words kRszThreads words apart, so a wave reads 256 contiguous bytes per load; otherwise
// they are single bytes kRszThreads bytes apart. Nothing outside the row is touched on either path.
#pragma once
#include "pixel_math.hpp"

namespace cms {

constexpr int kRszThreads = 256;
constexpr int kRszPerThread = 16;                           // byte columns per thread and chunk
constexpr int kRszChunk = kRszThreads * kRszPerThread;      // 4096 byte columns: 16 KiB of 32-bit sums
constexpr int kRszMaxSide = 16384;

// ---- one axis: cell o of Lo over L pixels covers pixels [rsz_cell_first, rsz_cell_end). o * L <= 2^28: int is enough
CMS_HD int rsz_cell_first(int o, int L, int Lo) { return o * L / Lo; }
CMS_HD int rsz_cell_end(int o, int L, int Lo) { return ((o + 1) * L + Lo - 1) / Lo; }
CMS_HD int rsz_weight(int o, int i, int L, int Lo) {
    const int lo = i * Lo > o * L ? i * Lo : o * L;
    const int hi = (i + 1) * Lo < (o + 1) * L ? (i + 1) * Lo : (o + 1) * L;
    return hi > lo ? hi - lo : 0;
}

// num / den to the nearest whole number, an exact half to the even neighbour (cv2's cvRound rule); den >= 1
CMS_HD uint64_t rsz_round_div(uint64_t num, uint64_t den) {
    const uint64_t q = num / den, r = num - q * den;
    if (2 * r > den) return q + 1;
    if (2 * r == den) return q + (q & 1);
    return q;
}

// ---- segments: as many output columns as have their source bytes in one chunk (less the up to three bytes in front of the
//      first one that alignment adds) and their outputs in one workgroup's threads, halved while that leaves the machine short of
//      workgroups and a segment still spans a full load of every thread. At least one column: a wider cell takes several chunks.
CMS_HD int rsz_span_bytes(int seg, int w, int wo, int c) {
    const long long px = ((long long)seg * w + wo - 1) / wo + 1;
    return (int)(px * c > 0x7fffffff ? 0x7fffffff : px * c);
}
inline int rsz_plan_segment(long long rows, int w, int c, int wo) {
    int seg = wo < kRszThreads / c ? wo : kRszThreads / c;
    while (seg > 1 && rsz_span_bytes(seg, w, wo, c) > kRszChunk - 3) seg = (seg + 1) / 2;
    while (seg > 1 && rows * ((wo + seg - 1) / seg) < 1024 && rsz_span_bytes((seg + 1) / 2, w, wo, c) >= 4 * kRszThreads)
        seg = (seg + 1) / 2;
    return seg;
}

struct RszGeom {
    int h, w, c, ho, wo;
    int seg, nseg;          // output columns per segment, segments per output row
    int words;              // base and row pitch on four bytes: word loads
};

CMS_HD size_t rsz_work_items(int n, const RszGeom& g) { return (size_t)n * g.ho * g.nseg; }

// the work unit `item`: its row of the batch seen as n * ho output rows, its image's first source row, its columns and chunks
struct RszItem {
    size_t out_row;         // n * ho + oy
    int oy, ox0, nox;       // output row in its image, first output column, output columns
    int iy0, iy1;           // source rows [iy0, iy1) of the image
    size_t src_row0;        // row index of source row 0 of the image in the batch seen as n * h rows
    int b0, b1;             // source bytes [b0, b1) of a row lie under the segment
    int a0;                 // b0 rounded down to four bytes: where the first chunk starts
};

CMS_HD RszItem rsz_item(size_t item, const RszGeom& g) {
    RszItem it;
    it.out_row = item / g.nseg;
    const int s = (int)(item - it.out_row * g.nseg);
    const size_t img = it.out_row / g.ho;
    it.oy = (int)(it.out_row - img * g.ho);
    it.src_row0 = img * g.h;
    it.ox0 = s * g.seg;
    it.nox = g.wo - it.ox0 < g.seg ? g.wo - it.ox0 : g.seg;
    it.iy0 = rsz_cell_first(it.oy, g.h, g.ho);
    it.iy1 = rsz_cell_end(it.oy, g.h, g.ho);
    it.b0 = rsz_cell_first(it.ox0, g.w, g.wo) * g.c;
    it.b1 = rsz_cell_end(it.ox0 + it.nox - 1, g.w, g.wo) * g.c;
    it.a0 = it.b0 & ~3;
    return it;
}

// byte column (of the row) of accumulator j of thread t in the chunk that starts at cb
template <bool WORDS>
CMS_HD int rsz_column(int cb, int t, int j) {
    return WORDS ? cb + 4 * ((j >> 2) * kRszThreads + t) + (j & 3) : cb + j * kRszThreads + t;
}

// phase 1 of thread t: acc[j] = sum over the item's source rows of wy * p at column rsz_column(cb, t, j), for the columns below
// `b1`. A load whose column is at or past b1 is sent to the chunk's first column instead (cb < b1, on four bytes), so that the loads
// of a row are unconditional and independent of one another; what it sums is stored like the rest and never read, because phase 2
// reads the columns below b1 only. `img` = first byte of source row 0 of the item's image, rows `pitch` bytes apart. On the word
// path the pitch is a multiple of four, so a word that starts below b1 <= pitch ends inside its row.
template <bool WORDS>
CMS_HD void rsz_column_sums(const uint8_t* img, size_t pitch, const RszGeom& g, const RszItem& it, int cb, int t,
                            uint32_t (&acc)[kRszPerThread]) {
    constexpr int kLoads = WORDS ? kRszPerThread / 4 : kRszPerThread;          // per thread and source row
    int off[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
        const int col = rsz_column<WORDS>(cb, t, WORDS ? 4 * k : k);
        off[k] = col < it.b1 ? col : cb;
    }
#pragma unroll
    for (int j = 0; j < kRszPerThread; ++j) acc[j] = 0;
#pragma unroll 2
    for (int iy = it.iy0; iy < it.iy1; ++iy) {
        const uint32_t wy = (uint32_t)rsz_weight(it.oy, iy, g.h, g.ho);
        const uint8_t* row = img + (size_t)iy * pitch;
        if constexpr (WORDS) {
            uint32_t q[kLoads];
#pragma unroll
            for (int k = 0; k < kLoads; ++k) q[k] = *reinterpret_cast<const uint32_t*>(row + off[k]);
#pragma unroll
            for (int k = 0; k < kLoads; ++k)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[4 * k + b] += wy * ((q[k] >> (8 * b)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < kLoads; ++k) acc[k] += wy * row[off[k]];
        }
    }
}

// ... handed over: sums[column - cb]
template <bool WORDS>
CMS_HD void rsz_store_sums(const uint32_t (&acc)[kRszPerThread], int t, uint32_t* sums) {
#pragma unroll
    for (int j = 0; j < kRszPerThread; ++j) sums[rsz_column<WORDS>(0, t, j)] = acc[j];
}

// phase 2 of the thread that owns output (ox, ch): the share of its numerator that the chunk [cb, cb + kRszChunk) holds
CMS_HD uint64_t rsz_add_chunk(const uint32_t* sums, const RszGeom& g, int cb, int ox, int ch) {
    int ix = rsz_cell_first(ox, g.w, g.wo);
    const int ix1 = rsz_cell_end(ox, g.w, g.wo);
    if (ix * g.c + ch < cb) ix = (cb - ch + g.c - 1) / g.c;                 // the first pixel whose byte lies in the chunk
    uint64_t num = 0;
    for (; ix < ix1 && ix * g.c + ch < cb + kRszChunk; ++ix)
        num += (uint64_t)rsz_weight(ox, ix, g.w, g.wo) * sums[ix * g.c + ch - cb];
    return num;
}

// ---- statistics: thread t of nt adds the pixels t, t + nt, ... of one image to acc = { sum p per channel, then sum p^2 }
CMS_HD void rsz_sum_sumsq_thread(const uint8_t* img, int pixels, int c, int t, int nt, uint64_t (&acc)[6]) {
    for (int px = t; px < pixels; px += nt)
        for (int ch = 0; ch < c; ++ch) {
            const uint64_t v = img[(size_t)px * c + ch];
            acc[ch] += v;
            acc[c + ch] += v * v;
        }
}

}  // namespace cms
