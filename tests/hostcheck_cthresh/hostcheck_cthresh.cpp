// Host driver of csrc/cthresh_math.hpp (tests/test_cthresh_hostcheck.py): the per-pixel pieces of the class-threshold consistency --
// k* with its tie rule, the pass bit, the fixed-point statistics -- over every pixel of a case, and the update arithmetic, with the
// very functions the kernels of csrc/cthresh.hip call. A stand-alone program: the test also builds it with the host sanitizers.
//
//   hostcheck_cthresh pixels IN OUT     IN : int32[10] n c h w H W align mode n_boxes flags(1 l1, 2 mask, 4 um0, 8 um1), then fp32
//                                            l0[n c h w], l1, thr[c], int32 ranges[n nb 4], fp32 mask[n H W], um0, um1 (those given)
//                                       OUT: int32 kstar[n H W], uint8 pass[n H W], uint64 table[2 + 3c]
//   hostcheck_cthresh update IN OUT     IN : int32[2] c adaptive, fp64[3] ema floor ceil, fp64 state[1 + c], fp32 thr[c],
//                                            uint64 table[2 + 3c], uint64 epoch[1 + 2c];  OUT: state, thr, table, epoch
// Exit codes: 0 ok, 2 refused arguments, 3 the compile-time and run-time class paths disagree, 4 file trouble.
#include <cstdio>
#include <cstring>
#include <vector>

#include "cthresh_math.hpp"

using namespace cms;

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <int CT>
static bool same_as_runtime(const float* row, int c, int k_rt, float conf_rt, const std::vector<uint32_t>& q_rt) {
    auto lt = [&](int i) { return row[i]; };
    float conf;
    std::vector<uint32_t> q(c);
    ct_pixel_stats<CT>(lt, c, conf, [&](int i, uint32_t v) { q[i] = v; });
    const int k = ct_kstar<CT>(lt, c);
    const bool conf_same = (conf == conf_rt) || (conf != conf && conf_rt != conf_rt);
    return k == k_rt && conf_same && q == q_rt;
}

static int run_pixels(FILE* in, FILE* out) {
    int32_t hd[10];
    if (fread(hd, sizeof(int32_t), 10, in) != 10) return 4;
    const int n = hd[0], c = hd[1], h = hd[2], w = hd[3], H = hd[4], W = hd[5], align = hd[6], mode = hd[7], nb = hd[8], flags = hd[9];
    if (n <= 0 || c <= 0 || c > 128 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || h > H || w > W || nb < 0) return 2;
    if (mode != MODE_MIX && mode != MODE_CUT) return 2;
    if ((nb > 0) == ((flags & 2) != 0)) return 2;                     // exactly one of ranges / mask
    if (mode == MODE_MIX && !(flags & 1)) return 2;
    const size_t lo = (size_t)n * c * h * w, P = (size_t)n * H * W;
    std::vector<float> l0, l1, thr, mask, um0, um1;
    std::vector<int32_t> ranges;
    if (!read_n(in, l0, lo) || !read_n(in, l1, (flags & 1) ? lo : 0) || !read_n(in, thr, (size_t)c) ||
        !read_n(in, ranges, (size_t)n * nb * 4) || !read_n(in, mask, (flags & 2) ? P : 0) || !read_n(in, um0, (flags & 4) ? P : 0) ||
        !read_n(in, um1, (flags & 8) ? P : 0))
        return 4;
    const float sy = bilin_scale(h, H, align != 0), sx = bilin_scale(w, W, align != 0);
    const bool ident = h == H && w == W;
    std::vector<int32_t> kstar(P);
    std::vector<uint8_t> pass(P);
    std::vector<unsigned long long> table((size_t)ct_table_len(c), 0ull);
    std::vector<float> row(c);
    std::vector<uint32_t> q(c);
    for (int s = 0; s < n; ++s)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t pix = ((size_t)s * H + y) * W + x;
                const bool m = (flags & 2) ? mask[pix] >= 0.5f : box_mask_bit(ranges.data() + (size_t)s * nb * 4, nb, y, x, true);
                const bool take1 = mode == MODE_MIX && m;
                const float* base = (take1 ? l1.data() : l0.data()) + (size_t)s * c * h * w;
                bool valid;
                if (mode == MODE_MIX) {
                    const std::vector<float>& um = take1 ? um1 : um0;
                    valid = um.empty() ? true : um[pix] >= 0.5f;
                } else {
                    valid = um0.empty() ? true : um0[pix] >= 0.5f;
                }
                const Tap ty = bilin_tap(y, sy, h, align != 0), tx = bilin_tap(x, sx, w, align != 0);
                for (int k = 0; k < c; ++k)
                    row[k] = ident ? base[(size_t)k * h * w + (size_t)y * w + x] : bilin_gather(base + (size_t)k * h * w, w, ty, tx);
                auto lt = [&](int k) { return row[k]; };
                float conf;
                ct_pixel_stats<0>(lt, c, conf, [&](int k, uint32_t v) { q[k] = v; });
                const int ks = ct_kstar<0>(lt, c);
                bool agree = true;
                if (c == 2) agree = same_as_runtime<2>(row.data(), c, ks, conf, q);
                if (c == 5) agree = same_as_runtime<5>(row.data(), c, ks, conf, q);
                if (c == 19) agree = same_as_runtime<19>(row.data(), c, ks, conf, q);
                if (c == 21) agree = same_as_runtime<21>(row.data(), c, ks, conf, q);
                if (!agree) return 3;
                const bool ps = ct_pass(conf, thr[ks]);
                kstar[pix] = ks;
                pass[pix] = ps ? 1 : 0;
                if (!valid) continue;
                table[0] += 1;
                table[1] += ct_fix24(conf);
                for (int k = 0; k < c; ++k) table[ct_slot_s(c, k)] += q[k];
                table[ct_slot_pred(c, ks)] += 1;
                if (ps) table[ct_slot_pass(c, ks)] += 1;
            }
    fwrite(kstar.data(), sizeof(int32_t), P, out);
    fwrite(pass.data(), 1, P, out);
    fwrite(table.data(), sizeof(unsigned long long), table.size(), out);
    return 0;
}

static int run_update(FILE* in, FILE* out) {
    int32_t hd[2];
    double par[3];
    if (fread(hd, sizeof(int32_t), 2, in) != 2 || fread(par, sizeof(double), 3, in) != 3) return 4;
    const int c = hd[0];
    if (c <= 0 || c > 128 || !(par[0] >= 0.0 && par[0] < 1.0) || !(par[1] <= par[2])) return 2;
    std::vector<double> state;
    std::vector<float> thr;
    std::vector<unsigned long long> table, epoch;
    if (!read_n(in, state, (size_t)1 + c) || !read_n(in, thr, (size_t)c) || !read_n(in, table, (size_t)ct_table_len(c)) ||
        !read_n(in, epoch, (size_t)ct_epoch_len(c)))
        return 4;
    ct_update(c, hd[1], par[0], par[1], par[2], state.data(), thr.data(), table.data(), epoch.data());
    fwrite(state.data(), sizeof(double), state.size(), out);
    fwrite(thr.data(), sizeof(float), thr.size(), out);
    fwrite(table.data(), sizeof(unsigned long long), table.size(), out);
    fwrite(epoch.data(), sizeof(unsigned long long), epoch.size(), out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = fopen(argv[2], "rb");
    if (!in) return 4;
    FILE* out = fopen(argv[3], "wb");
    if (!out) {
        fclose(in);
        return 4;
    }
    int rc = 2;
    if (!strcmp(argv[1], "pixels")) rc = run_pixels(in, out);
    else if (!strcmp(argv[1], "update")) rc = run_update(in, out);
    fclose(in);
    fclose(out);
    return rc;
}
