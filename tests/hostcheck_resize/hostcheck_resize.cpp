// test infrastructure: a stand-alone host driver of the product's area-resize arithmetic (csrc/resize_math.hpp), the very
// functions the kernels of csrc/resize.hip call, walked over the same work items, chunks and threads a launch covers.
//
//   hostcheck_resize REQUEST RESULT
//
// REQUEST: nine little-endian int32 -- kind and eight arguments (unused ones 0) -- then the payload.
//   kind 0  weights     L, Lo                                -> int32: the Lo x L weights, then the Lo first pixels and the Lo ends
//   kind 1  division    den                                  -> int64: rsz_round_div(num, den) for num = 0 .. 255 * den
//   kind 2  resize      n, h, w, c, ho, wo, source and destination misalignment (bytes, 0..3), then the n * h * w * c source
//                       bytes                                -> the n * ho * wo * c output bytes
//   kind 3  statistics  n, pixels, c, then the source bytes  -> int64 (n, 2c)
// Source and destination of kind 2 live in exactly-sized heap blocks (a sanitizer build sees every byte outside them) at the
// requested misalignment, so both the word and the byte path of the column loads can be driven. The destination is poisoned and
// every byte of it must be written exactly once. Exit code 2 for a request the product refuses.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cutmix-semisup-seg_amd/csrc/resize_math.hpp"

using namespace cms;

// one launch: what resize_area_u8<WORDS> does, the threads of a workgroup one after the other between its barriers
template <bool WORDS>
static bool run_resize(const uint8_t* src, uint8_t* dst, int n, const RszGeom& g, std::vector<int>& writes) {
    const size_t pitch = (size_t)g.w * g.c, total = rsz_work_items(n, g);
    std::vector<uint32_t> sums(kRszChunk);
    std::vector<uint64_t> num(kRszThreads);
    for (size_t item = 0; item < total; ++item) {
        const RszItem it = rsz_item(item, g);
        if (it.nox * g.c > kRszThreads) return false;          // more outputs than the workgroup has threads
        const uint8_t* img = src + it.src_row0 * pitch;
        for (int t = 0; t < kRszThreads; ++t) num[t] = 0;
        for (int cb = it.a0; cb < it.b1; cb += kRszChunk) {
            for (int t = 0; t < kRszThreads; ++t) {
                uint32_t acc[kRszPerThread];
                rsz_column_sums<WORDS>(img, pitch, g, it, cb, t, acc);
                rsz_store_sums<WORDS>(acc, t, sums.data());
            }
            for (int t = 0; t < it.nox * g.c; ++t) num[t] += rsz_add_chunk(sums.data(), g, cb, it.ox0 + t / g.c, t % g.c);
        }
        for (int t = 0; t < it.nox * g.c; ++t) {
            const size_t at = (it.out_row * g.wo + it.ox0 + t / g.c) * g.c + t % g.c;
            dst[at] = (uint8_t)rsz_round_div(num[t], (uint64_t)g.h * g.w);
            ++writes[at];
        }
    }
    return true;
}

static int write_result(const char* path, const void* data, size_t bytes) {
    FILE* f = fopen(path, "wb");
    if (!f) return 1;
    if (bytes && fwrite(data, 1, bytes, f) != bytes) return 1;
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_resize REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t a[9];
    if (fread(a, sizeof(int32_t), 9, f) != 9) return 1;
    const int kind = a[0];
    if (kind == 0) {
        const int L = a[1], Lo = a[2];
        if (Lo < 1 || L < Lo || L > kRszMaxSide) return 2;
        std::vector<int32_t> out;
        for (int o = 0; o < Lo; ++o)
            for (int i = 0; i < L; ++i) out.push_back(rsz_weight(o, i, L, Lo));
        for (int o = 0; o < Lo; ++o) out.push_back(rsz_cell_first(o, L, Lo));
        for (int o = 0; o < Lo; ++o) out.push_back(rsz_cell_end(o, L, Lo));
        fclose(f);
        return write_result(argv[2], out.data(), out.size() * sizeof(int32_t));
    }
    if (kind == 1) {
        const int den = a[1];
        if (den < 1) return 2;
        std::vector<int64_t> out;
        for (int64_t num = 0; num <= 255 * (int64_t)den; ++num) out.push_back((int64_t)rsz_round_div((uint64_t)num, (uint64_t)den));
        fclose(f);
        return write_result(argv[2], out.data(), out.size() * sizeof(int64_t));
    }
    if (kind == 3) {
        const int n = a[1], pixels = a[2], c = a[3];
        if (n < 1 || pixels < 1 || (c != 1 && c != 3)) return 2;
        const size_t per = (size_t)pixels * c;
        uint8_t* in = (uint8_t*)malloc(n * per);
        if (!in || fread(in, 1, n * per, f) != n * per) return 1;
        fclose(f);
        std::vector<int64_t> out((size_t)n * 2 * c);
        for (int i = 0; i < n; ++i) {
            uint64_t total[6] = {};
            for (int t = 0; t < kRszThreads; ++t) {
                uint64_t acc[6] = {};
                rsz_sum_sumsq_thread(in + i * per, pixels, c, t, kRszThreads, acc);
                for (int k = 0; k < 6; ++k) total[k] += acc[k];
            }
            for (int k = 0; k < 2 * c; ++k) out[(size_t)i * 2 * c + k] = (int64_t)total[k];
        }
        free(in);
        return write_result(argv[2], out.data(), out.size() * sizeof(int64_t));
    }
    if (kind != 2) return 1;
    const int n = a[1], h = a[2], w = a[3], c = a[4], ho = a[5], wo = a[6], in_off = a[7], out_off = a[8];
    if (n < 1 || h < 1 || w < 1 || ho < 1 || wo < 1 || (c != 1 && c != 3) || ho > h || wo > w || h > kRszMaxSide || w > kRszMaxSide)
        return 2;
    if (in_off < 0 || in_off > 3 || out_off < 0 || out_off > 3) return 1;
    const size_t in_bytes = (size_t)n * h * w * c, out_bytes = (size_t)n * ho * wo * c;
    // malloc returns 16-byte aligned blocks: base + offset has exactly the requested misalignment, and the block ends with the data
    uint8_t* in_block = (uint8_t*)malloc(in_bytes + in_off);
    uint8_t* out_block = (uint8_t*)malloc(out_bytes + out_off);
    if (!in_block || !out_block) return 1;
    if (fread(in_block + in_off, 1, in_bytes, f) != in_bytes) return 1;
    fclose(f);
    memset(out_block, 0xA5, out_bytes + out_off);
    const uint8_t* src = in_block + in_off;
    RszGeom g;
    g.h = h, g.w = w, g.c = c, g.ho = ho, g.wo = wo;
    g.seg = rsz_plan_segment((long long)n * ho, w, c, wo);
    g.nseg = (wo + g.seg - 1) / g.seg;
    g.words = (uintptr_t)src % 4 == 0 && ((size_t)w * c) % 4 == 0;
    std::vector<int> writes(out_bytes, 0);
    const bool ok = g.words ? run_resize<true>(src, out_block + out_off, n, g, writes)
                            : run_resize<false>(src, out_block + out_off, n, g, writes);
    if (!ok) return 3;
    for (size_t i = 0; i < out_bytes; ++i)
        if (writes[i] != 1) return 3;                          // an output byte skipped or written twice
    for (int i = 0; i < out_off; ++i)
        if (out_block[i] != 0xA5) return 3;                    // a store in front of the destination
    const int rc = write_result(argv[2], out_block + out_off, out_bytes);
    free(in_block);
    free(out_block);
    return rc;
}
