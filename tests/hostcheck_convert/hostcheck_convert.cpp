// test infrastructure: a stand-alone host driver of the product's converter arithmetic (csrc/convert_math.hpp), the very
// functions the kernels of csrc/convert.hip call, walked over the same work items a launch covers.
//
//   hostcheck_convert REQUEST RESULT
//
// REQUEST: seven little-endian int32 -- kind (0 images, 1 labels), n, h, w, d, source misalignment, destination misalignment (bytes,
// 0..3) -- then the n * h * w * (3 or 1) source bytes. RESULT: the n * (h / d) * (w / d) * (3 or 1) output bytes. Source and
// destination live in exactly-sized heap blocks (a sanitizer build sees every byte outside them) at the requested misalignment,
// so both the word and the byte paths of the piece loads and stores can be driven. Exit code 2 for a request the product refuses.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../cutmix-semisup-seg_amd/csrc/convert_math.hpp"

using namespace cms;

template <int D, int C>
static void run(const uint8_t* src, uint8_t* dst, int n, int ho, int wo) {
    const bool in_words = cvt_words_ok(src, (size_t)wo * D * C), out_words = cvt_words_ok(dst, (size_t)wo * C);
    const size_t total = cvt_work_items(n, ho, wo);
    for (size_t idx = 0; idx < total; ++idx) cvt_work_item<D, C>(src, dst, idx, wo, in_words, out_words);
}

template <int C>
static bool dispatch(int d, const uint8_t* src, uint8_t* dst, int n, int ho, int wo) {
    switch (d) {
        case 1: run<1, C>(src, dst, n, ho, wo); return true;
        case 2: run<2, C>(src, dst, n, ho, wo); return true;
        case 3: run<3, C>(src, dst, n, ho, wo); return true;
        case 4: run<4, C>(src, dst, n, ho, wo); return true;
        case 5: run<5, C>(src, dst, n, ho, wo); return true;
        case 6: run<6, C>(src, dst, n, ho, wo); return true;
        case 7: run<7, C>(src, dst, n, ho, wo); return true;
        case 8: run<8, C>(src, dst, n, ho, wo); return true;
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: hostcheck_convert REQUEST RESULT\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[7];
    if (fread(head, sizeof(int32_t), 7, f) != 7) return 1;
    const int kind = head[0], n = head[1], h = head[2], w = head[3], d = head[4], in_off = head[5], out_off = head[6];
    if (kind < 0 || kind > 1 || n < 1 || h < 1 || w < 1 || d < 1 || d > kCvtMaxD || h % d || w % d) return 2;
    if (in_off < 0 || in_off > 3 || out_off < 0 || out_off > 3) return 1;
    const int c = kind == 0 ? 3 : 1, ho = h / d, wo = w / d;
    const size_t in_bytes = (size_t)n * h * w * c, out_bytes = (size_t)n * ho * wo * c;
    // malloc returns 16-byte aligned blocks: base + offset has exactly the requested misalignment, and the block ends with the data
    uint8_t* in_block = (uint8_t*)malloc(in_bytes + in_off);
    uint8_t* out_block = (uint8_t*)malloc(out_bytes + out_off);
    if (!in_block || !out_block) return 1;
    if (fread(in_block + in_off, 1, in_bytes, f) != in_bytes) return 1;
    fclose(f);
    memset(out_block, 0xA5, out_bytes + out_off);
    const bool ok = kind == 0 ? dispatch<3>(d, in_block + in_off, out_block + out_off, n, ho, wo)
                              : dispatch<1>(d, in_block + in_off, out_block + out_off, n, ho, wo);
    if (!ok) return 2;
    for (int i = 0; i < out_off; ++i)
        if (out_block[i] != 0xA5) return 3;                    // a store in front of the destination
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 1;
    if (fwrite(out_block + out_off, 1, out_bytes, g) != out_bytes) return 1;
    fclose(g);
    free(in_block);
    free(out_block);
    return 0;
}
