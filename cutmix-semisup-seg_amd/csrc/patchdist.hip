// The kernels around the FFT of the patch-distance analysis (gfx950): patch_dist.py:107-154 (sliding-window squared distance of a
// query patch to every patch of an image) and intra_inter_class_patch_dist.py:186-211 (the nearest same-class / other-class pixels).
// All arithmetic is on integer grey levels:
//     D2[n,i,j] = P2[i,j] + Q2[n] - 2 PQ[n,i,j],   PQ = `valid` cross-correlation of the symmetric-padded image with patch n
// PQ comes out of the fp64 FFT (csrc/fft.hip) within ~1e-5 of an integer and is rounded back; the largest distance from an integer
// seen is reported so the caller can refuse a result whose exactness is not certain.
//
//   load      a pool entry (uint8 [Hs][Ws][3]) -> three symmetric-padded planes, zero up to the FFT size; N patches cut from padded
//             pool entries -> planes holding the FLIPPED patches of a pair in the real and imaginary parts, so that
//             F_image * F_pair (no conjugate) transforms back to PQ of the first patch (real) and of the second (imaginary)
//   product   sum over the three channels of F_image[c] * F_pair[k][c]
//   finish    rint, D2 as int64, the selection key D2 << 24 | flat index, the rounding residual (a 64-bit atomicMax on the bit
//             pattern of a non-negative double)
//   select    radix select of the k smallest masked keys: eight 8-bit histogram passes find the k-th key, one pass compacts the
//             keys <= it. No sort of the map; the caller sorts the <= k survivors.
// and, without the FFT, patch_dist.py:39-104 (the distance of a patch to the patches centred on its four neighbours):
//   squares   squared neighbour differences of the symmetric extension of a pool entry, two int32 planes
//   box sum   exact separable running sums in int64, loads per output independent of the box
#include "common.hpp"

namespace cms {

// numpy's `symmetric` padding: the edge pixel repeats; any number of reflections (pad >= n)
__device__ __forceinline__ int sym_index(int i, int n) {
    const int period = 2 * n;
    int m = i % period;
    if (m < 0) m += period;
    return m < n ? m : period - 1 - m;
}

__global__ void pd_load_image(const uint8_t* __restrict__ img, int hs, int ws, int pad_h, int pad_w, int hp, int wp, int fh, int fw,
                              double2* __restrict__ planes, long long* __restrict__ sq) {
    const size_t plane = (size_t)fh * fw;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < plane; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / fw), x = (int)(i % fw);
        int v[3] = {0, 0, 0};
        if (y < hp && x < wp) {
            const uint8_t* p = img + ((size_t)sym_index(y - pad_h, hs) * ws + sym_index(x - pad_w, ws)) * 3;
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
            if (sq) sq[(size_t)y * wp + x] = (long long)(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) planes[c * plane + i] = make_double2((double)v[c], 0.0);
    }
}

__device__ __forceinline__ int patch_pixel(const uint8_t* __restrict__ pool, const cms_pd_patch& q, int u, int v, int c, int pad_h,
                                           int pad_w) {
    return pool[q.img_off + ((size_t)sym_index(q.cy - pad_h + u, q.hs) * q.ws + sym_index(q.cx - pad_w + v, q.ws)) * 3 + c];
}

// grid (blocks, n_pairs): planes (n_pairs, 3, fh, fw)
__global__ void pd_load_patches(const uint8_t* __restrict__ pool, const cms_pd_patch* __restrict__ patches, int n, int ph, int pw,
                                int fh, int fw, double2* __restrict__ planes) {
    const int pair = blockIdx.y;
    const int n0 = 2 * pair, n1 = 2 * pair + 1;
    const cms_pd_patch q0 = patches[n0];
    const cms_pd_patch q1 = patches[n1 < n ? n1 : n0];
    const int pad_h = (ph - 1) / 2, pad_w = (pw - 1) / 2;
    const size_t plane = (size_t)fh * fw;
    double2* out = planes + (size_t)pair * 3 * plane;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < plane; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / fw), x = (int)(i % fw);
        // flipped: patch element (u, v) sits at (-u mod fh, -v mod fw)
        const int u = (fh - y) & (fh - 1), v = (fw - x) & (fw - 1);
        const bool in = u < ph && v < pw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double re = 0.0, im = 0.0;
            if (in) {
                re = (double)patch_pixel(pool, q0, u, v, c, pad_h, pad_w);
                if (n1 < n) im = (double)patch_pixel(pool, q1, u, v, c, pad_h, pad_w);
            }
            out[c * plane + i] = make_double2(re, im);
        }
    }
}

// out[n] += sum over the patch of (a - b)^2 (b == NULL: of a^2). grid (blocks, n); out zeroed by the caller
__global__ void pd_patch_sqdiff(const uint8_t* __restrict__ pool, const cms_pd_patch* __restrict__ a, const cms_pd_patch* __restrict__ b,
                                int ph, int pw, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[16];
    const int n = blockIdx.y;
    const cms_pd_patch qa = a[n];
    cms_pd_patch qb = qa;
    if (b) qb = b[n];
    const int pad_h = (ph - 1) / 2, pad_w = (pw - 1) / 2;
    const int count = ph * pw;
    unsigned long long acc = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const int u = i / pw, v = i % pw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int d = patch_pixel(pool, qa, u, v, c, pad_h, pad_w);
            if (b) d -= patch_pixel(pool, qb, u, v, c, pad_h, pad_w);
            acc += (unsigned long long)(d * d);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += part[w];
        if (s) atomicAdd(&out[n], s);
    }
}

// grid (blocks, n_pairs): out[k] = sum_c f_img[c] * f_pair[k][c]
__global__ void pd_spectrum_product(const double2* __restrict__ f_img, const double2* __restrict__ f_pairs, size_t plane,
                                    double2* __restrict__ out) {
    const double2* fp = f_pairs + (size_t)blockIdx.y * 3 * plane;
    double2* o = out + (size_t)blockIdx.y * plane;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < plane; i += (size_t)gridDim.x * blockDim.x) {
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double2 a = f_img[c * plane + i], b = fp[c * plane + i];
            re += a.x * b.x - a.y * b.y;
            im += a.x * b.y + a.y * b.x;
        }
        o[i] = make_double2(re, im);
    }
}

// grid (blocks, n)
__global__ void pd_finish(const double2* __restrict__ corr, const long long* __restrict__ p2, const long long* __restrict__ q2, int h,
                          int w, int fh, int fw, long long* __restrict__ d2_out, long long* __restrict__ keys,
                          unsigned long long* __restrict__ residual_bits) {
    __shared__ unsigned long long part[16];
    const int n = blockIdx.y;
    const double2* c = corr + (size_t)(n >> 1) * fh * fw;
    const bool imag = n & 1;
    const long long q = q2[n];
    const int m = h * w;
    double worst = 0.0;
    bool not_finite = false;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const int y = i / w, x = i % w;
        const double2 z = c[(size_t)y * fw + x];
        const double v = imag ? z.y : z.x;
        const double r = rint(v);
        const double e = fabs(v - r);
        not_finite |= e != e;               // NaN, or inf - inf
        worst = fmax(worst, e);
        const long long d2 = p2[i] + q - 2 * (long long)r;
        if (d2_out) d2_out[(size_t)n * m + i] = d2;
        if (keys) keys[(size_t)n * m + i] = (long long)(((unsigned long long)d2 << 24) | (unsigned long long)i);
    }
    // non-negative doubles order as their bit patterns; a value that is not finite is reported as NaN, which sorts above them all
    unsigned long long bits = not_finite ? 0x7ff8000000000000ULL : (unsigned long long)__double_as_longlong(worst);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(bits, off, 64);
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s = part[k] > s ? part[k] : s;
        if (s) atomicMax(residual_bits, s);
    }
}

// ---------------------------------------------------------------------------------------------------------------- selection
struct SelectState {                 // one per row of keys, in the workspace
    unsigned long long prefix;       // the bits of the k-th key found so far
    unsigned int remaining;          // rank of the k-th key among the keys that share `prefix`
    unsigned int take_all;           // the row has no more than k masked keys: keep every one
};

struct SelectMask {
    const uint8_t* mask;             // mode 0: (n, m) bytes, non-zero = candidate
    const uint8_t* labels;           // modes 1, 2: (m) label map shared by every row
    const int* cls;                  //             (n) class of each row
    int mode;                        // 1: label == cls[row]; 2: label != cls[row] and label != 255
};

__device__ __forceinline__ bool select_masked(const SelectMask& k, int row, size_t m, size_t i, int cls) {
    if (k.mode == 0) return k.mask[(size_t)row * m + i] != 0;
    const int l = k.labels[i];
    return k.mode == 1 ? l == cls : (l != cls && l != 255);
}

constexpr int kSelectThreads = 256;

// hist[row][digit] += number of masked keys of the row that share the prefix above `shift + 8` and have `digit` at `shift`
__global__ __launch_bounds__(kSelectThreads) void select_histogram(const unsigned long long* __restrict__ keys, SelectMask km, size_t m,
                                                                   int shift, const SelectState* __restrict__ state,
                                                                   unsigned int* __restrict__ hist) {
    __shared__ unsigned int bins[256];
    const int row = blockIdx.y;
    bins[threadIdx.x] = 0;
    __syncthreads();
    const SelectState st = state[row];
    if (!st.take_all) {
        const int cls = km.mode ? km.cls[row] : 0;
        const int hi = shift + 8;
        const unsigned long long* kr = keys + (size_t)row * m;
        for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
            if (!select_masked(km, row, m, i, cls)) continue;
            const unsigned long long key = kr[i];
            if (hi < 64 && (key >> hi) != (st.prefix >> hi)) continue;
            atomicAdd(&bins[(unsigned)(key >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    const unsigned int c = bins[threadIdx.x];
    if (c) atomicAdd(&hist[row * 256 + threadIdx.x], c);
}

// one thread per row: pick the digit that holds the k-th key, clear the histogram for the next pass
__global__ void select_pick(SelectState* __restrict__ state, unsigned int* __restrict__ hist, int n, int shift, unsigned int k,
                            int first_pass) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    SelectState st = state[row];
    unsigned int* h = hist + row * 256;
    if (first_pass) {
        unsigned long long total = 0;
        for (int d = 0; d < 256; ++d) total += h[d];
        st.prefix = 0;
        st.remaining = k;
        st.take_all = total <= k;
    }
    if (!st.take_all) {
        unsigned int seen = 0;
        for (int d = 0; d < 256; ++d) {
            const unsigned int c = h[d];
            if (seen + c >= st.remaining) {
                st.prefix |= (unsigned long long)d << shift;
                st.remaining -= seen;
                break;
            }
            seen += c;
        }
    }
    for (int d = 0; d < 256; ++d) h[d] = 0;
    state[row] = st;
}

// out[row][count[row]++] = every masked key <= the k-th (every masked key when the row has no more than k)
__global__ __launch_bounds__(kSelectThreads) void select_compact(const unsigned long long* __restrict__ keys, SelectMask km, size_t m,
                                                                 const SelectState* __restrict__ state, unsigned int k,
                                                                 long long* __restrict__ out, int* __restrict__ count) {
    const int row = blockIdx.y;
    const SelectState st = state[row];
    const int cls = km.mode ? km.cls[row] : 0;
    const unsigned long long* kr = keys + (size_t)row * m;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
        if (!select_masked(km, row, m, i, cls)) continue;
        const unsigned long long key = kr[i];
        if (!st.take_all && key > st.prefix) continue;
        const int pos = atomicAdd(&count[row], 1);
        if ((unsigned)pos < k) out[(size_t)row * k + pos] = (long long)key;
    }
}

__global__ void select_init(SelectState* state, unsigned int* hist, int* count, long long* out, int n, unsigned int k) {
    const size_t total = (size_t)n * k;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        out[i] = 0x7fffffffffffffffLL;
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t < (size_t)n * 256) hist[t] = 0;
    if (t < (size_t)n) {
        SelectState st;
        st.prefix = 0; st.remaining = k; st.take_all = 0;
        state[t] = st;
        count[t] = 0;
    }
}

static size_t select_workspace(int n) { return n > 0 ? (size_t)n * (sizeof(SelectState) + 256 * sizeof(unsigned int)) : 0; }

// ------------------------------------------------------------------------------------------- neighbouring-patch distances
// patch_dist.py:57-104: the distance of the patch centred on a pixel to the patches centred on its four neighbours. Moving a patch
// by one pixel turns the sum over the patch of (c - neighbour)^2 into a box sum of squared neighbour DIFFERENCES of the padded
// image, so nothing here multiplies patches: one pass writes the squared differences, an exact separable box sum finishes them.
// With a = (ph - 1) / 2, b = (pw - 1) / 2, I the symmetric extension of the entry and (y, x) over the (hs + ph - 1, ws + pw - 1)
// domain of the centre view:
//     hq[y][x] = sum_c (I[y-a][x-b] - I[y-a][x-b-1])^2    x <= wp: left = box(hq)[:, :ws],  right = box(hq)[:, 1:]
//     vq[y][x] = sum_c (I[y-a][x-b] - I[y-a-1][x-b])^2    y <= hp: up   = box(vq)[:hs, :],  down  = box(vq)[1:, :]
// (the right neighbour's difference at x is the left one's at x + 1, reflections at the edge included).

// grid (blocks over x, rows): one thread per (y, x) of the (hp + 1, wp + 1) domain both planes fit in
__global__ void pd_neighbour_squares(const uint8_t* __restrict__ img, int hs, int ws, int pad_h, int pad_w, int hp, int wp,
                                     int* __restrict__ hq, int* __restrict__ vq) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x > wp) return;
    const int sx = sym_index(x - pad_w, ws), sl = sym_index(x - pad_w - 1, ws);
    for (int y = blockIdx.y; y <= hp; y += gridDim.y) {
        const uint8_t* row = img + (size_t)sym_index(y - pad_h, hs) * ws * 3;
        const uint8_t* above = img + (size_t)sym_index(y - pad_h - 1, hs) * ws * 3;
        int h2 = 0, v2 = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int v = row[(size_t)sx * 3 + c];
            const int dh = v - row[(size_t)sl * 3 + c], dv = v - above[(size_t)sx * 3 + c];
            h2 += dh * dh;
            v2 += dv * dv;
        }
        if (y < hp) hq[(size_t)y * (wp + 1) + x] = h2;
        if (x < wp) vq[(size_t)y * wp + x] = v2;
    }
}

// The box sum is separable, and each pass is a running sum: a window moved by one gains one element and loses one, so an output
// costs two loads whatever the window. A line is cut into segments that run in parallel; a segment starts from a window summed
// directly, and the host sizes the segments by the window so that this start stays a bounded number of loads per output (at most
// 4 more in pass 1, 1 more in pass 2), however large the window.
//
// pass 1, down the columns: tmp[i][x] = sum_{u < ph} in[i + u][x]. One thread per column and segment of `seg` output rows: lanes
// are adjacent columns, so every load and store of a wave is one contiguous row piece. grid (blocks over x, segments)
template <class T>
__global__ void pd_box_columns(const T* __restrict__ in, int wp, int ho, int ph, int seg, long long* __restrict__ tmp) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= wp) return;
    for (long long first = (long long)blockIdx.y * seg; first < ho; first += (long long)gridDim.y * seg) {
        const int i0 = (int)first, i1 = (int)min(first + seg, (long long)ho);
        const T* p = in + (size_t)i0 * wp + x;
        long long acc = 0;
#pragma unroll 8
        for (int u = 0; u < ph; ++u) acc += (long long)p[(size_t)u * wp];       // (unrolled: the loads of a thread are in flight together)
        long long* o = tmp + (size_t)i0 * wp + x;
        o[0] = acc;
#pragma unroll 4
        for (int i = i0 + 1; i < i1; ++i) {
            acc += (long long)p[(size_t)(ph - 1 + i - i0) * wp] - (long long)p[(size_t)(i - 1 - i0) * wp];
            o[(size_t)(i - i0) * wp] = acc;
        }
    }
}

struct BoxOut {                      // where the box sums go: value (i, j) of the (ho, wo) result is written to
    long long* a;                    //   a[i * ld + j]                 if i < ha and j < wa
    long long* b;                    //   b[(i - di) * ld + (j - dj)]   if b, i >= di and j >= dj: the same plane seen one step on
    int ld, ha, wa, di, dj;
};

// pass 2, along the rows: out[i][j] = sum_{v < pw} tmp[i][j + v]. One WAVE per row and segment of `seg` outputs, lanes adjacent
// outputs: out[j0 + m] = window(j0) + sum_{k <= m} (tmp[j0 + pw - 1 + k] - tmp[j0 + k - 1]), the sum being a wave-wide inclusive
// scan of 64 differences (six shuffle steps) plus the carry of the chunks before. All loads and stores are contiguous per wave
// and nothing passes through LDS.
__global__ __launch_bounds__(256) void pd_box_rows(const long long* __restrict__ tmp, int wp, int ho, int wo, int pw, int seg,
                                                   int n_seg, BoxOut out) {
    const int lane = threadIdx.x & 63;
    const long long items = (long long)ho * n_seg;
    const long long step = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long item = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); item < items; item += step) {
        const int i = (int)(item / n_seg);
        const int j0 = (int)(item % n_seg) * seg, j1 = min(j0 + seg, wo);
        const long long* row = tmp + (size_t)i * wp;
        long long window = 0;
        for (int v = lane; v < pw; v += 64) window += row[j0 + v];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) window += __shfl_xor(window, off, 64);
        for (int m0 = 0; j0 + m0 < j1; m0 += 64) {
            const int j = j0 + m0 + lane;
            const bool live = j < j1;
            long long d = 0;
            if (live && j > j0) d = row[j + pw - 1] - row[j - 1];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const long long below = __shfl_up(d, off, 64);
                if (lane >= off) d += below;
            }
            const long long v = window + d;
            window += __shfl(d, 63, 64);
            if (live) {
                if (i < out.ha && j < out.wa) out.a[(size_t)i * out.ld + j] = v;
                if (out.b && i >= out.di && j >= out.dj) out.b[(size_t)(i - out.di) * out.ld + (j - out.dj)] = v;
            }
        }
    }
}

constexpr int kBoxMinSegment = 32;       // output rows per thread of pass 1, at least
constexpr int kBoxMinRowSegment = 256;   // outputs per wave of pass 2, at least

// the two passes of one plane (hp, wp) -> (hp - ph + 1, wp - pw + 1); tmp holds (hp - ph + 1) * wp int64
template <class T>
static void box_sum_launch(const T* in, int hp, int wp, int ph, int pw, long long* tmp, const BoxOut& out, hipStream_t s) {
    const int ho = hp - ph + 1, wo = wp - pw + 1;
    // a segment no shorter than a quarter of the window: the direct sum that starts it adds at most 4 loads per output
    const int seg = max(kBoxMinSegment, (ph + 3) / 4);
    const int n_seg = (ho + seg - 1) / seg;
    hipLaunchKernelGGL(pd_box_columns<T>, dim3((wp + 63) / 64, min(n_seg, 65535)), dim3(64), 0, s, in, wp, ho, ph, seg, tmp);
    // a wave sums its first window 64 elements at a time: a segment as long as the window makes that one more load per output
    const int row_seg = max(kBoxMinRowSegment, (pw + 63) / 64 * 64);
    const int n_row_seg = (wo + row_seg - 1) / row_seg;
    const long long waves = (long long)ho * n_row_seg;
    hipLaunchKernelGGL(pd_box_rows, dim3((unsigned)min((waves + 3) / 4, (long long)(256 * 16))), dim3(256), 0, s, tmp, wp, ho, wo,
                       pw, row_seg, n_row_seg, out);
}

constexpr long long kBoxMaxElements = 1LL << 30;     // of a plane: rows and columns stay ints with room to spare, offsets are size_t

static int box_geometry_ok(long long hp, long long wp, int ph, int pw) {
    return ph > 0 && pw > 0 && hp >= ph && wp >= pw && hp * wp < kBoxMaxElements;
}

static size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct NeighbourLayout {             // the workspace of cms_pd_neighbour_maps: tmp | hq | vq
    int hp, wp;
    size_t tmp_bytes, hq_bytes, vq_bytes;
    size_t total() const { return tmp_bytes + hq_bytes + vq_bytes; }
};

static int neighbour_layout(int hs, int ws, int ph, int pw, NeighbourLayout* l) {
    if (hs <= 0 || ws <= 0 || ph <= 0 || pw <= 0 || !(ph & 1) || !(pw & 1)) return 0;
    const long long hp = (long long)hs + ph - 1, wp = (long long)ws + pw - 1;
    if ((hp + 1) * (wp + 1) >= kBoxMaxElements) return 0;
    l->hp = (int)hp;
    l->wp = (int)wp;
    const size_t th = (size_t)hs * (size_t)(wp + 1), tv = (size_t)(hs + 1) * (size_t)wp;
    l->tmp_bytes = align16((th > tv ? th : tv) * sizeof(long long));
    l->hq_bytes = align16((size_t)hp * (size_t)(wp + 1) * sizeof(int));
    l->vq_bytes = align16((size_t)(hp + 1) * (size_t)wp * sizeof(int));
    return 1;
}

static int patch_geometry_ok(int ph, int pw, int fh, int fw) {
    return ph > 0 && pw > 0 && (ph & 1) && (pw & 1) && fh >= 8 && fw >= 8 && fh <= 4096 && fw <= 4096 && !(fh & (fh - 1)) &&
           !(fw & (fw - 1));
}

}  // namespace cms

using namespace cms;

extern "C" int cms_pd_load_image(const uint8_t* pool_img, const cms_stage_entry* entry_host, int ph, int pw, int fh, int fw,
                                 void* planes, int64_t* sq, void* stream) {
    CMS_REQUIRE(pool_img && entry_host && planes, "pd_load_image: NULL pointer");
    CMS_REQUIRE(patch_geometry_ok(ph, pw, fh, fw), "pd_load_image: odd patch sizes and power-of-two FFT sizes in 8 ... 4096 required");
    const int hs = entry_host->hs, ws = entry_host->ws;
    CMS_REQUIRE(hs > 0 && ws > 0 && entry_host->img_off >= 0, "pd_load_image: bad pool entry");
    const long long hp = (long long)hs + ph - 1, wp = (long long)ws + pw - 1;
    CMS_REQUIRE(hp <= fh && wp <= fw, "pd_load_image: padded image %lld x %lld exceeds the FFT size %d x %d", hp, wp, fh, fw);
    hipLaunchKernelGGL(pd_load_image, dim3(grid_for((size_t)fh * fw, 256)), dim3(256), 0, (hipStream_t)stream,
                       pool_img + entry_host->img_off, hs, ws, (ph - 1) / 2, (pw - 1) / 2, (int)hp, (int)wp, fh, fw, (double2*)planes,
                       (long long*)sq);
    return launch_status("cms_pd_load_image");
}

extern "C" int cms_pd_load_patches(const uint8_t* pool_img, const cms_pd_patch* patches, int n, int ph, int pw, int fh, int fw,
                                   void* planes, void* stream) {
    CMS_REQUIRE(pool_img && patches && planes, "pd_load_patches: NULL pointer");
    CMS_REQUIRE(patch_geometry_ok(ph, pw, fh, fw), "pd_load_patches: odd patch sizes and power-of-two FFT sizes in 8 ... 4096 required");
    CMS_REQUIRE(ph <= fh && pw <= fw, "pd_load_patches: patch %d x %d exceeds the FFT size %d x %d", ph, pw, fh, fw);
    CMS_REQUIRE(n > 0 && n <= 2 * 65535, "pd_load_patches: n must be in 1 ... 131070 (got %d)", n);
    hipLaunchKernelGGL(pd_load_patches, dim3(grid_for((size_t)fh * fw, 256, 1024), (n + 1) / 2), dim3(256), 0, (hipStream_t)stream,
                       pool_img, patches, n, ph, pw, fh, fw, (double2*)planes);
    return launch_status("cms_pd_load_patches");
}

extern "C" int cms_pd_patch_sqdiff(const uint8_t* pool_img, const cms_pd_patch* a, const cms_pd_patch* b, int n, int ph, int pw,
                                   int64_t* out, void* stream) {
    CMS_REQUIRE(pool_img && a && out, "pd_patch_sqdiff: NULL pointer");
    CMS_REQUIRE(ph > 0 && pw > 0 && (ph & 1) && (pw & 1) && (long long)ph * pw <= (1LL << 24), "pd_patch_sqdiff: bad patch size");
    CMS_REQUIRE(n > 0 && n <= 65535, "pd_patch_sqdiff: n must be in 1 ... 65535 (got %d)", n);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, (size_t)n * sizeof(int64_t), s) != hipSuccess) return launch_status("cms_pd_patch_sqdiff");
    hipLaunchKernelGGL(pd_patch_sqdiff, dim3(grid_for((size_t)ph * pw, 256, 64), n), dim3(256), 0, s, pool_img, a, b, ph, pw,
                       (unsigned long long*)out);
    return launch_status("cms_pd_patch_sqdiff");
}

extern "C" int cms_pd_spectrum_product(const void* f_img, const void* f_pairs, int n_pairs, int fh, int fw, void* out, void* stream) {
    CMS_REQUIRE(f_img && f_pairs && out, "pd_spectrum_product: NULL pointer");
    CMS_REQUIRE(n_pairs > 0 && n_pairs <= 65535 && fh > 0 && fw > 0, "pd_spectrum_product: bad geometry");
    hipLaunchKernelGGL(pd_spectrum_product, dim3(grid_for((size_t)fh * fw, 256, 1024), n_pairs), dim3(256), 0, (hipStream_t)stream,
                       (const double2*)f_img, (const double2*)f_pairs, (size_t)fh * fw, (double2*)out);
    return launch_status("cms_pd_spectrum_product");
}

extern "C" int cms_pd_finish(const void* corr, const int64_t* p2, const int64_t* q2, int n, int h, int w, int fh, int fw, int64_t* d2,
                             int64_t* keys, uint64_t* residual_bits, void* stream) {
    CMS_REQUIRE(corr && p2 && q2 && residual_bits, "pd_finish: NULL pointer");
    CMS_REQUIRE(d2 || keys, "pd_finish: nothing to produce");
    CMS_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0 && h <= fh && w <= fw, "pd_finish: bad geometry");
    CMS_REQUIRE((long long)h * w <= (1LL << 24), "pd_finish: h * w must not exceed 2^24 (the key holds a 24-bit flat index)");
    hipLaunchKernelGGL(pd_finish, dim3(grid_for((size_t)h * w, 256, 1024), n), dim3(256), 0, (hipStream_t)stream, (const double2*)corr,
                       (const long long*)p2, (const long long*)q2, h, w, fh, fw, (long long*)d2, (long long*)keys,
                       (unsigned long long*)residual_bits);
    return launch_status("cms_pd_finish");
}

extern "C" size_t cms_select_workspace_bytes(int n) { return select_workspace(n); }

extern "C" int cms_select_k_smallest(const int64_t* keys, const uint8_t* mask, const uint8_t* labels, const int32_t* cls, int mode,
                                     int n, long long m, int k, int64_t* out, int32_t* count, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    CMS_REQUIRE(keys && out && count, "select_k_smallest: NULL pointer");
    CMS_REQUIRE(mode >= 0 && mode <= 2, "select_k_smallest: mode must be 0 (mask), 1 (label == cls) or 2 (label != cls, != 255)");
    CMS_REQUIRE(mode == 0 ? mask != NULL : (labels != NULL && cls != NULL), "select_k_smallest: the mask source of mode %d is NULL", mode);
    CMS_REQUIRE(n > 0 && n <= 65535 && m > 0 && m <= (1LL << 31) && k > 0, "select_k_smallest: bad geometry");
    CMS_REQUIRE(workspace && workspace_bytes >= select_workspace(n), "select_k_smallest: workspace too small (%zu bytes needed)",
                select_workspace(n));
    hipStream_t s = (hipStream_t)stream;
    SelectState* state = (SelectState*)workspace;
    unsigned int* hist = (unsigned int*)(state + n);
    SelectMask km;
    km.mask = mask; km.labels = labels; km.cls = cls; km.mode = mode;
    const size_t init_items = (size_t)n * ((size_t)k > 256 ? (size_t)k : 256);
    hipLaunchKernelGGL(select_init, dim3((unsigned)((init_items + 255) / 256)), dim3(256), 0, s, state, hist, count, (long long*)out, n,
                       (unsigned)k);
    const dim3 grid(grid_for((size_t)m, kSelectThreads, 256), n);
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(select_histogram, grid, dim3(kSelectThreads), 0, s, (const unsigned long long*)keys, km, (size_t)m, shift, state,
                           hist);
        hipLaunchKernelGGL(select_pick, dim3((n + 63) / 64), dim3(64), 0, s, state, hist, n, shift, (unsigned)k, shift == 56 ? 1 : 0);
    }
    hipLaunchKernelGGL(select_compact, grid, dim3(kSelectThreads), 0, s, (const unsigned long long*)keys, km, (size_t)m, state, (unsigned)k,
                       (long long*)out, count);
    return launch_status("cms_select_k_smallest");
}

extern "C" int cms_pd_box_sum(const void* in, int in_is_int64, int hp, int wp, int ph, int pw, void* work, int64_t* out, void* stream) {
    CMS_REQUIRE(in && work && out, "pd_box_sum: NULL pointer");
    CMS_REQUIRE(box_geometry_ok(hp, wp, ph, pw), "pd_box_sum: a box of %d x %d in a plane of %d x %d (fewer than 2^30 elements) required",
                ph, pw, hp, wp);
    BoxOut o;
    o.a = (long long*)out; o.b = NULL;
    o.ha = hp - ph + 1; o.wa = o.ld = wp - pw + 1; o.di = o.dj = 0;
    if (in_is_int64) box_sum_launch((const long long*)in, hp, wp, ph, pw, (long long*)work, o, (hipStream_t)stream);
    else box_sum_launch((const int*)in, hp, wp, ph, pw, (long long*)work, o, (hipStream_t)stream);
    return launch_status("cms_pd_box_sum");
}

extern "C" size_t cms_pd_neighbour_workspace_bytes(int hs, int ws, int ph, int pw) {
    NeighbourLayout l;
    return neighbour_layout(hs, ws, ph, pw, &l) ? l.total() : 0;
}

extern "C" int cms_pd_neighbour_maps(const uint8_t* pool_img, const cms_stage_entry* entry_host, int ph, int pw, void* work,
                                     int64_t* out_d2, void* stream) {
    CMS_REQUIRE(pool_img && entry_host && work && out_d2, "pd_neighbour_maps: NULL pointer");
    CMS_REQUIRE(ph > 0 && pw > 0 && (ph & 1) && (pw & 1), "pd_neighbour_maps: odd patch sizes required (got %d x %d)", ph, pw);
    const int hs = entry_host->hs, ws = entry_host->ws;
    CMS_REQUIRE(hs > 0 && ws > 0 && entry_host->img_off >= 0, "pd_neighbour_maps: bad pool entry");
    NeighbourLayout l;
    CMS_REQUIRE(neighbour_layout(hs, ws, ph, pw, &l), "pd_neighbour_maps: the padded image (%d + %d) x (%d + %d) must stay below 2^30 pixels",
                hs, ph, ws, pw);
    hipStream_t s = (hipStream_t)stream;
    long long* tmp = (long long*)work;
    int* hq = (int*)((char*)work + l.tmp_bytes);
    int* vq = (int*)((char*)work + l.tmp_bytes + l.hq_bytes);
    hipLaunchKernelGGL(pd_neighbour_squares, dim3((l.wp + 1 + 255) / 256, min(l.hp + 1, 65535)), dim3(256), 0, s,
                       pool_img + entry_host->img_off, hs, ws, (ph - 1) / 2, (pw - 1) / 2, l.hp, l.wp, hq, vq);
    const size_t map = (size_t)hs * ws;
    BoxOut o;
    o.ld = ws; o.ha = hs; o.wa = ws;
    o.a = (long long*)out_d2; o.b = (long long*)out_d2 + map; o.di = 0; o.dj = 1;                  // left, right
    box_sum_launch(hq, l.hp, l.wp + 1, ph, pw, tmp, o, s);
    o.a = (long long*)out_d2 + 2 * map; o.b = (long long*)out_d2 + 3 * map; o.di = 1; o.dj = 0;    // up, down
    box_sum_launch(vq, l.hp + 1, l.wp, ph, pw, tmp, o, s);
    return launch_status("cms_pd_neighbour_maps");
}
