// The skeleton every loss family of the library shares (gfx950): consistency and cross entropy (losses.hip), ICT (ict.hip) and the
// augmentation consistency (aug_loss.hip). Device side: the accessors of a pixel's class vector, the LDS-staged low-resolution
// rectangles, the forward tile walk, the flat pixel walk, the tiled adjoint of the bilinear upsample and the two-stage reduction
// of the loss sums. Host side: the geometry, its checks, and ONE launch path each for the forward, the backward and the fused kernels. A
// family supplies its per-pixel arithmetic (the *_math.hpp headers) as lambdas and its kernels as thin shells.
#pragma once
#include <algorithm>
#include <cstdlib>
#include "common.hpp"

namespace cms {

// ------------------------------------------------------------------------------------------------ accessors
template <bool IDENT>
struct Gather {
    const float* base;  // class-0 plane of sample n
    size_t plane;       // h*w
    int w_in;
    Tap ty, tx;
    size_t off;  // y*w + x, IDENT only
    __device__ __forceinline__ float operator()(int c) const {
        if (IDENT) return base[c * plane + off];
        return bilin_gather(base + c * plane, w_in, ty, tx);
    }
};

template <int CT>
struct RegVec {
    float v[CT > 0 ? CT : 1];
    __device__ __forceinline__ float operator()(int c) const { return v[c]; }
};

template <int CT, bool IDENT>
__device__ __forceinline__ void fill(RegVec<CT>& r, const Gather<IDENT>& g) {
#pragma unroll
    for (int c = 0; c < CT; ++c) r.v[c] = g(c);
}

struct Geo {
    int n, c, h, w, H, W, align;
    float sy, sx;
    // tiled backward: this launch covers the tiles (col_x + i * col_kx, col_y + j * col_ky) -- one COLOUR class of the tile
    // grid, chosen on the host so that no two tiles of a launch touch the same low-resolution cell (see tiled_launches)
    int col_kx, col_ky, col_x, col_y;
};

inline Geo make_geo(int n, int c, int h, int w, int H, int W, int align) {
    Geo g;
    g.n = n; g.c = c; g.h = h; g.w = w; g.H = H; g.W = W; g.align = align;
    g.col_kx = g.col_ky = 1;
    g.col_x = g.col_y = 0;
    g.sy = bilin_scale(h, H, align != 0);
    g.sx = bilin_scale(w, W, align != 0);
    return g;
}

// every loss descriptor carries the same n, c, h, w, H, W, align_corners
template <class D>
inline Geo geo_of(const D* d) {
    return make_geo(d->n, d->c, d->h, d->w, d->H, d->W, d->align_corners);
}

inline bool is_ident(const Geo& g) { return g.h == g.H && g.w == g.W; }

// The geometry checks every family makes, in two halves (the augmentation consistency has a check of its own between them).
// `of`: what the full-resolution geometry is the geometry of ("loss", or "label" for the cross entropy)
template <class D>
inline int check_sizes_positive(const D* d, const char* name) {
    CMS_REQUIRE(d->n > 0 && d->c > 0 && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0, "%s: bad geometry", name);
    return CMS_OK;
}
template <class D>
inline int check_logits_fit(const D* d, const char* name, const char* of = "loss") {
    CMS_REQUIRE(d->h <= d->H && d->w <= d->W, "%s: logits larger than the %s geometry", name, of);
    return CMS_OK;
}
template <class D>
inline int check_geometry(const D* d, const char* name, const char* of = "loss") {
    const int rc = check_sizes_positive(d, name);
    return rc ? rc : check_logits_fit(d, name, of);
}

template <class D>
inline int check_loss_fn(const D* d) {
    CMS_REQUIRE(d->loss_fn >= CMS_LOSS_VAR && d->loss_fn <= CMS_LOSS_KLD, "Unknown consistency loss function %d", d->loss_fn);
    return CMS_OK;
}

// ---- LDS-staged low-resolution patches (round 5) ---------------------------------------------------------------
// A workgroup owns a tile of output pixels of ONE sample; the bilinear taps of the whole tile fall into a small rectangle
// of low-resolution cells (3 rows x 11 columns at the 1/8 scale of the DeepLab heads). The kernels used to gather every tap
// of every class of every pixel from global memory (168 four-byte loads per pixel for 21 classes and two tensors: latency-
// bound, 0.07-0.08 of the HBM rate on moved bytes); now the rectangle of each logit tensor is copied to LDS once
// per workgroup, [class][row][column], and the per-pixel gathers read it there with the taps rebased -- the same arithmetic
// (bilin_gather) on the same values, so every per-pixel result is bit-identical.
constexpr int TILE_W = 64;
constexpr int FWD_TILE_H = 8;               // forward kernels: 64 x 8 pixels per workgroup, 2 per thread
struct Patch {
    int x_lo, n_cols, y_lo, n_rows;
};

__device__ __forceinline__ Patch tile_patch(const Geo& g, int x0, int y0, int tw, int th) {
    // i0 / i1 are monotone in the output coordinate: the first pixel's i0 and the last pixel's i1 bound the rectangle
    const Tap xa = bilin_tap(x0, g.sx, g.w, g.align != 0), xb = bilin_tap(x0 + tw - 1, g.sx, g.w, g.align != 0);
    const Tap ya = bilin_tap(y0, g.sy, g.h, g.align != 0), yb = bilin_tap(y0 + th - 1, g.sy, g.h, g.align != 0);
    Patch p;
    p.x_lo = xa.i0; p.n_cols = xb.i1 - xa.i0 + 1;
    p.y_lo = ya.i0; p.n_rows = yb.i1 - ya.i0 + 1;
    return p;
}

// dst[c][r][j] = src[c][y_lo + r][x_lo + j] for the C class planes of one sample (`src` = its class-0 plane)
__device__ __forceinline__ void stage_patch(float* __restrict__ dst, const float* __restrict__ src, int C, size_t plane, int w,
                                            const Patch& p) {
    const int per = p.n_rows * p.n_cols, total = C * per;
    for (int i = (int)threadIdx.x; i < total; i += (int)blockDim.x) {
        const int c = i / per, rj = i - c * per;
        const int r = rj / p.n_cols, j = rj - r * p.n_cols;
        dst[i] = src[(size_t)c * plane + (size_t)(p.y_lo + r) * w + (p.x_lo + j)];
    }
}

__device__ __forceinline__ void rebase(Tap& ty, Tap& tx, const Patch& p) {
    ty.i0 -= p.y_lo; ty.i1 -= p.y_lo;
    tx.i0 -= p.x_lo; tx.i1 -= p.x_lo;
}

inline int tile_max_cols(float sx) { return (int)((TILE_W - 1) * sx) + 3; }
inline int tile_max_rows_of(float sy, int tile_h) { return (int)((tile_h - 1) * sy) + 3; }
inline size_t patch_floats(int C, float sy, float sx, int tile_h) {
    return (size_t)C * tile_max_rows_of(sy, tile_h) * tile_max_cols(sx);
}
constexpr size_t FWD_PATCH_LDS_MAX = 96 * 1024;      // beyond (scales near 1 with many classes): the direct-gather kernels

// the class vector of pixel (y, x) gathered from a sample's global planes (`base` = its class-0 plane)
template <bool IDENT>
__device__ __forceinline__ Gather<IDENT> gather_at(const float* base, const Geo& g, int y, int x) {
    Gather<IDENT> r;
    r.base = base;
    r.plane = (size_t)g.h * g.w;
    r.w_in = g.w;
    if (IDENT) {
        r.off = (size_t)y * g.w + x;
    } else {
        r.ty = bilin_tap(y, g.sy, g.h, g.align != 0);
        r.tx = bilin_tap(x, g.sx, g.w, g.align != 0);
    }
    return r;
}

// ... from the LDS copy `base` of the rectangle `p`, with taps already rebased to it
__device__ __forceinline__ Gather<false> gather_staged(const float* base, const Patch& p, const Tap& ty, const Tap& tx) {
    Gather<false> r;
    r.base = base;
    r.plane = (size_t)p.n_rows * p.n_cols;
    r.w_in = p.n_cols;
    r.ty = ty;
    r.tx = tx;
    return r;
}

// a tile of one sample: origin and clipped extent
struct ScatterTile {
    int n, x0, y0, tw, th;
};

// the 64 x FWD_TILE_H tile of this workgroup in a launch of the LDS-staged forward kernels
__device__ __forceinline__ ScatterTile fwd_tile(const Geo& g) {
    const int tiles_x = (g.W + TILE_W - 1) / TILE_W, tiles_y = (g.H + FWD_TILE_H - 1) / FWD_TILE_H;
    int b = blockIdx.x;
    const int tx_i = b % tiles_x;
    b /= tiles_x;
    const int ty_i = b % tiles_y;
    ScatterTile t;
    t.n = b / tiles_y;
    t.x0 = tx_i * TILE_W;
    t.y0 = ty_i * FWD_TILE_H;
    t.tw = min(TILE_W, g.W - t.x0);
    t.th = min(FWD_TILE_H, g.H - t.y0);
    return t;
}

// The forward tile walk: `stage(n, patch, smem)` copies the tile's rectangle(s) to LDS, then -- behind the barrier -- every valid
// pixel of the tile gets `pixel(n, y, x, ty, tx, patch)` with its taps rebased to the rectangle. UNROLL: the two pixels of a
// thread unrolled or not (register allocation, per family).
template <bool UNROLL, class Stage, class Pixel>
__device__ __forceinline__ void fwd_tile_walk(const Geo& g, float* smem, Stage stage, Pixel pixel) {
    const ScatterTile t = fwd_tile(g);
    const Patch p = tile_patch(g, t.x0, t.y0, t.tw, t.th);
    stage(t.n, p, smem);
    __syncthreads();
    const int col = threadIdx.x & (TILE_W - 1);
    auto rows = [&](int rr) {
        const int row = (threadIdx.x >> 6) + rr * 4;
        if (col < t.tw && row < t.th) {
            const int y = t.y0 + row, x = t.x0 + col;
            Tap ty = bilin_tap(y, g.sy, g.h, g.align != 0), tx = bilin_tap(x, g.sx, g.w, g.align != 0);
            rebase(ty, tx, p);
            pixel(t.n, y, x, ty, tx, p);
        }
    };
    if (UNROLL) {
#pragma unroll
        for (int rr = 0; rr < FWD_TILE_H / 4; ++rr) rows(rr);
    } else {
#pragma unroll 1
        for (int rr = 0; rr < FWD_TILE_H / 4; ++rr) rows(rr);
    }
}

// The flat pixel walk of the direct-gather kernels: `f(pix, n, y, x)` for every output pixel, pix = (n * H + y) * W + x.
template <class F>
__device__ __forceinline__ void pixel_walk(const Geo& g, F f) {
    const size_t P = (size_t)g.n * g.H * g.W;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < P; idx += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(idx % g.W);
        const size_t t = idx / g.W;
        const int y = (int)(t % g.H);
        const int n = (int)(t / g.H);
        f(idx, n, y, x);
    }
}

// first stage of the loss sums: this workgroup's K sums -> partials[blockIdx.x][K]. `red` (K * 16 floats) is the calling kernel's
// OWN __shared__ array: a static of this function would be one LDS variable shared by every kernel of the module, and with it
// cons_fused_tiled_kernel<21, VAR>, which sits at its 128-register bound, spills (profiles/loss_kernels_resources_refactor.md)
template <int K>
__device__ __forceinline__ void store_partials(float (&acc)[K], float* red, float* __restrict__ partials) {
    block_sum<K>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partials[blockIdx.x * K + k] = acc[k];
    }
}

// second stage: fixed-order sum of the per-workgroup partials in double
template <int K>
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partials, int nblocks,
                                                              double* __restrict__ out, double extra, int extra_slot) {
    __shared__ double sm[K][256];
    double loc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) loc[k] = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
#pragma unroll
        for (int k = 0; k < K; ++k) loc[k] += (double)partials[i * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sm[k][threadIdx.x] = loc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < K; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = sm[k][0];
        if (extra_slot >= 0) out[extra_slot] = extra;
    }
}

// ---- backward with upsampling: LDS-tiled adjoint of the bilinear interpolation ---------------------------------
// Workgroup = 256 threads = one tile of TILE_H x TILE_W output pixels of one sample.
//   phase 1  every thread computes the gradient vector of its 2 pixels -> G[row][class][col]        (LDS)
//   phase 2  x-adjoint:  R[row][class][j] = sum_col wx(col -> cell j) * G[row][class][col]          (LDS)
//   phase 3  y-adjoint:  out[class][i][j] = sum_row wy(row -> cell i) * R[row][class][j]  -> one global atomicAdd
// Summation order inside a tile is fixed. Neighbouring tiles share low-resolution cells; so that their sums do not meet in
// an order that changes from run to run, the tile grid is issued as kx * ky COLOUR classes, one launch each, in a fixed
// order on the stream: within a launch every cell receives exactly one add (round 3: the logit gradients, and with them
// every weight gradient downstream, are run-to-run reproducible).
#ifndef CMS_LOSS_TILE_H
#define CMS_LOSS_TILE_H 4
#endif
constexpr int TILE_H = CMS_LOSS_TILE_H;     // 4 or 8 (256 threads = 64 columns x 4 rows, TILE_H / 4 pixels per thread). Measured with 4
                                            // (half the LDS, twice the workgroups): consistency / CE backward 205 -> 160 / 170 -> 120 us,
                                            // the step unchanged (620.4 vs 619.4 img/s, profiles/r04zw_*): these launches run beside the
                                            // operand re-pack and are no longer what the step waits for. Round 5: 4 is the default --
                                            // with the logit rectangles staged in LDS next to G and R a 4-row tile keeps 4 workgroups per CU
constexpr int G_LD = TILE_W + 1;  // +1 float: conflict-free column access for class-major readers

struct TileTables {
    int xi0[TILE_W], xi1[TILE_W];
    float xw1[TILE_W];
    int yi0[TILE_H], yi1[TILE_H];
    float yw1[TILE_H];
    int xbeg[TILE_W + 2], xend[TILE_W + 2];
};

inline int tile_max_rows(float sy) { return tile_max_rows_of(sy, TILE_H); }

// G + R + `n_patches` staged logit rectangles (student / teacher 0 / teacher 1, or the one tensor of the cross entropy)
inline size_t tile_lds_bytes(int C, float sy, float sx, int n_patches) {
    size_t g = (size_t)TILE_H * C * G_LD;
    size_t r = (size_t)TILE_H * C * tile_max_cols(sx);
    return (g + r + (size_t)n_patches * patch_floats(C, sy, sx, TILE_H)) * sizeof(float);
}

// the tile of this workgroup in a launch of tiled_scatter
__device__ __forceinline__ ScatterTile scatter_tile(const Geo& g) {
    const int tiles_x = (g.W + TILE_W - 1) / TILE_W;
    const int tiles_y = (g.H + TILE_H - 1) / TILE_H;
    const int ctx = (tiles_x - g.col_x + g.col_kx - 1) / g.col_kx;      // tiles of this colour class per row / column
    const int cty = (tiles_y - g.col_y + g.col_ky - 1) / g.col_ky;
    int b = blockIdx.x;
    const int tx_i = g.col_x + (b % ctx) * g.col_kx;
    b /= ctx;
    const int ty_i = g.col_y + (b % cty) * g.col_ky;
    ScatterTile t;
    t.n = b / cty;
    t.x0 = tx_i * TILE_W;
    t.y0 = ty_i * TILE_H;
    t.tw = min(TILE_W, g.W - t.x0);
    t.th = min(TILE_H, g.H - t.y0);
    return t;
}

template <class Stage, class PixelGrad>
__device__ __forceinline__ void tiled_scatter(const Geo& g, Stage stage, PixelGrad pixel_grad, float* __restrict__ grad_lo,
                                              float* smem) {
    __shared__ TileTables tb;
    const ScatterTile tile = scatter_tile(g);
    const int n = tile.n, x0 = tile.x0, y0 = tile.y0, tw = tile.tw, th = tile.th;
    const int C = g.c;
    const int tid = threadIdx.x;

    if (tid < TILE_W) {
        Tap t = bilin_tap(min(x0 + tid, g.W - 1), g.sx, g.w, g.align != 0);
        tb.xi0[tid] = t.i0;
        tb.xi1[tid] = t.i1;
        tb.xw1[tid] = t.w1;
    } else if (tid < TILE_W + TILE_H) {
        const int r = tid - TILE_W;
        Tap t = bilin_tap(min(y0 + r, g.H - 1), g.sy, g.h, g.align != 0);
        tb.yi0[r] = t.i0;
        tb.yi1[r] = t.i1;
        tb.yw1[r] = t.w1;
    }
    __syncthreads();
    // the tile's rectangle of low-resolution cells: every thread reads it off the tables (four broadcast LDS reads) -- no
    // single-thread section and no second barrier in front of the staging (round 6)
    const int r_x_lo = tb.xi0[0], r_n_cols = tb.xi1[tw - 1] - r_x_lo + 1;
    const int r_y_lo = tb.yi0[0], r_n_rows = tb.yi1[th - 1] - r_y_lo + 1;
    // contiguous range [xbeg, xend) of tile columns that touch low-res column x_lo + j (i0 is monotone in x). (round 6) every tile
    // column reports itself to its two cells with LDS atomics -- one step for 64 lanes -- instead of n_cols lanes scanning all 64
    // columns in a dependent loop while the other three waves of the workgroup wait (same table, bit-identical results)
    if (tid < r_n_cols) {
        tb.xbeg[tid] = tw;
        tb.xend[tid] = 0;
    }
    __syncthreads();
    if (tid < tw) {
        const int j0 = tb.xi0[tid] - r_x_lo, j1 = tb.xi1[tid] - r_x_lo;
        atomicMin(&tb.xbeg[j0], tid);
        atomicMax(&tb.xend[j0], tid + 1);
        atomicMin(&tb.xbeg[j1], tid);
        atomicMax(&tb.xend[j1], tid + 1);
    }

    float* G = smem;                                 // [TILE_H][C][G_LD]
    float* R = smem + (size_t)TILE_H * C * G_LD;     // [TILE_H][C][n_cols]
    // (round 5) phase 0: the tile's rectangle of every logit tensor -> LDS behind G and R; phase 1 gathers from there
    Patch patch;
    patch.x_lo = r_x_lo; patch.n_cols = r_n_cols; patch.y_lo = r_y_lo; patch.n_rows = r_n_rows;
    float* P = R + (size_t)TILE_H * C * r_n_cols;
    stage(n, patch, P);
    // (round 6) x-adjoint weights as a table: wtab[j][u] = weight of tile column xbeg[j] + u in low-res column j -- phase 2's inner
    // loop is then two LDS reads and an FMA per term instead of three table reads, two compares and two selects (same values, same
    // order: bit-identical). Small tables only (the DeepLab scales: 11-19 columns, <= 18 terms); otherwise the comparing loop.
    constexpr int WT_COLS = 24, WT_SPAN = 20;
    __shared__ float wtab[WT_COLS * WT_SPAN];
    const bool wide = tid < r_n_cols && (tb.xend[tid] - tb.xbeg[tid]) > WT_SPAN;
    const bool table = __syncthreads_or(wide ? 1 : 0) == 0 && r_n_cols <= WT_COLS;      // (also the barrier behind the staging)
    if (table) {
        for (int e = tid; e < r_n_cols * WT_SPAN; e += blockDim.x) {
            const int j = e / WT_SPAN, u = e - j * WT_SPAN;
            const int c = tb.xbeg[j] + u;
            float wv = 0.0f;
            if (c < tb.xend[j]) {
                const int X = r_x_lo + j;
                const float w1 = tb.xw1[c];
                wv = (tb.xi0[c] == X ? 1.0f - w1 : 0.0f) + (tb.xi1[c] == X ? w1 : 0.0f);
            }
            wtab[e] = wv;
        }
    }

    // phase 1
    const int col = tid & (TILE_W - 1);
#pragma unroll
    for (int rr = 0; rr < TILE_H / 4; ++rr) {
        const int row = (tid >> 6) + rr * 4;
        float* gcol = G + ((size_t)row * C) * G_LD + col;
        const bool valid = col < tw && row < th;
        bool wrote = false;
        if (valid) {
            Tap ty, tx;
            ty.i0 = tb.yi0[row]; ty.i1 = tb.yi1[row]; ty.w1 = tb.yw1[row]; ty.w0 = 1.0f - ty.w1;
            tx.i0 = tb.xi0[col]; tx.i1 = tb.xi1[col]; tx.w1 = tb.xw1[col]; tx.w0 = 1.0f - tx.w1;
            rebase(ty, tx, patch);
            wrote = pixel_grad(n, y0 + row, x0 + col, ty, tx, patch, P, [&](int k, float v) { gcol[(size_t)k * G_LD] = v; });
        }
        if (!wrote) {
            for (int k = 0; k < C; ++k) gcol[(size_t)k * G_LD] = 0.0f;
        }
    }
    __syncthreads();

    // phase 2: items (row, j, class), class fastest across lanes -> stride G_LD reads, conflict-free
    const int n_cols = r_n_cols, n_rows = r_n_rows;
    const int items2 = th * n_cols * C;
    for (int it = tid; it < items2; it += blockDim.x) {
        const int k = it % C;
        const int rj = it / C;
        const int j = rj % n_cols;
        const int row = rj / n_cols;
        const int X = r_x_lo + j;
        const float* gr = G + ((size_t)row * C + k) * G_LD;
        float s = 0.0f;
        if (table) {
            const int cb = tb.xbeg[j], nterm = tb.xend[j] - cb;
            const float* wt = wtab + j * WT_SPAN;
            for (int u = 0; u < nterm; ++u) s += wt[u] * gr[cb + u];
        } else {
            for (int c = tb.xbeg[j]; c < tb.xend[j]; ++c) {
                const float w1 = tb.xw1[c];
                float wgt = (tb.xi0[c] == X ? 1.0f - w1 : 0.0f) + (tb.xi1[c] == X ? w1 : 0.0f);
                s += wgt * gr[c];
            }
        }
        R[((size_t)row * C + k) * n_cols + j] = s;
    }
    __syncthreads();

    // phase 3: items (class, i, j), j fastest -> coalesced atomics
    const int items3 = C * n_rows * n_cols;
    const size_t plane = (size_t)g.h * g.w;
    float* out_n = grad_lo + (size_t)n * C * plane;
    for (int it = tid; it < items3; it += blockDim.x) {
        const int j = it % n_cols;
        const int ki = it / n_cols;
        const int i = ki % n_rows;
        const int k = ki / n_rows;
        const int Y = r_y_lo + i;
        float s = 0.0f;
        for (int row = 0; row < th; ++row) {
            const float w1 = tb.yw1[row];
            float wgt = (tb.yi0[row] == Y ? 1.0f - w1 : 0.0f) + (tb.yi1[row] == Y ? w1 : 0.0f);
            s += wgt * R[((size_t)row * C + k) * n_cols + j];
        }
        if (s != 0.0f) atomicAdd(out_n + (size_t)k * plane + (size_t)Y * g.w + (r_x_lo + j), s);
    }
}

// Smallest tile distance k along one axis such that tiles t and t + k never touch the same low-resolution cell.
inline int tile_colour_period(int full, int low, float scale, bool align, int tile) {
    const int T = (full + tile - 1) / tile;
    int k = 1;
    for (;;) {
        bool clash = false;
        for (int t = 0; t + k < T && !clash; ++t) {
            const Tap hi = bilin_tap(std::min(t * tile + tile - 1, full - 1), scale, low, align);
            const Tap lo = bilin_tap((t + k) * tile, scale, low, align);
            clash = lo.i0 <= hi.i1;
        }
        if (!clash || k >= T) return k;
        ++k;
    }
}

// The once-read switch state lives in losses.hip, its single definition: run-to-run reproducible backward
// (cms_loss_set_deterministic / CMS_LOSS_DETERMINISTIC), the tile count of the LDS-staged forward kernels (CMS_LOSS_FWD_TILED;
// 0 = use the direct-gather kernels) and of the fused forward + backward launches (CMS_LOSS_FUSED; 0 = not available).
bool loss_deterministic();
int fwd_tiles(const Geo& g, int n_patches, size_t* lds_out, int* stride_out);
int fused_tiles(const Geo& g, int n_patches);

// Issues `launch(geo, tiles)` once per colour class of the tile grid, in a fixed order (or once for all tiles, see above).
template <class F>
inline void tiled_launches(Geo g, F launch) {
    const int tiles_x = (g.W + TILE_W - 1) / TILE_W, tiles_y = (g.H + TILE_H - 1) / TILE_H;
    if (!loss_deterministic()) {
        g.col_kx = g.col_ky = 1;
        g.col_x = g.col_y = 0;
        launch(g, tiles_x * tiles_y * g.n);
        return;
    }
    g.col_kx = tile_colour_period(g.W, g.w, g.sx, g.align != 0, TILE_W);
    g.col_ky = tile_colour_period(g.H, g.h, g.sy, g.align != 0, TILE_H);
    for (int cy = 0; cy < g.col_ky; ++cy)
        for (int cx = 0; cx < g.col_kx; ++cx) {
            const int ctx = (tiles_x - cx + g.col_kx - 1) / g.col_kx, cty = (tiles_y - cy + g.col_ky - 1) / g.col_ky;
            if (ctx <= 0 || cty <= 0) continue;
            g.col_x = cx;
            g.col_y = cy;
            launch(g, ctx * cty * g.n);
        }
}

#define CMS_DISPATCH_C(C, ...)                    \
    switch (C) {                                  \
        case 2: { constexpr int CT = 2; __VA_ARGS__; } break;   \
        case 5: { constexpr int CT = 5; __VA_ARGS__; } break;   \
        case 19: { constexpr int CT = 19; __VA_ARGS__; } break; \
        case 21: { constexpr int CT = 21; __VA_ARGS__; } break; \
        default: { constexpr int CT = 0; __VA_ARGS__; } break;  \
    }

// ------------------------------------------------------------------------------------------------ launch paths
constexpr size_t TILE_LDS_MAX = 160 * 1024 - 4096;      // G + R + the staged rectangles of a backward / fused tile, at most

inline int fwd_grid(size_t P) { return grid_for(P, 256, 2048); }
inline int fwd_blocks(const Geo& g, int n_patches) {
    const int t = fwd_tiles(g, n_patches, nullptr, nullptr);
    return t > 0 ? t : fwd_grid((size_t)g.n * g.H * g.W);
}

template <class K>
inline void allow_lds(K kern, size_t lds) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// what a forward launch runs: `tiles` workgroups of the LDS-staged kernel (lds bytes, rectangles `pstride` floats apart), or,
// with tiles == 0, `grid` workgroups of a direct-gather kernel
struct FwdPlan {
    int tiles, grid, pstride;
    size_t lds;
};

inline FwdPlan fwd_plan(const Geo& g, int n_patches) {
    FwdPlan p;
    p.lds = 0;
    p.pstride = 0;
    p.tiles = fwd_tiles(g, n_patches, &p.lds, &p.pstride);
    p.grid = p.tiles > 0 ? p.tiles : fwd_grid((size_t)g.n * g.H * g.W);
    return p;
}

// One forward launch of a family -- its tiled, identity or direct kernel (`tiled_extra`: what the tiled kernel takes behind the
// partials) -- and, unless stats_out is NULL, the fixed-order reduction of its K partial sums (+ `extra` into out[extra_slot]).
template <int K, class Args, class Tiled, class Direct, class... Extra>
inline void launch_fwd(Tiled tiled, Direct ident, Direct direct, const Args& a, const FwdPlan& p, float* partials, double* stats_out,
                       double extra, int extra_slot, hipStream_t s, Extra... tiled_extra) {
    if (p.tiles > 0) {
        allow_lds(tiled, p.lds);
        hipLaunchKernelGGL(tiled, dim3(p.grid), dim3(256), p.lds, s, a, partials, tiled_extra...);
    } else {
        hipLaunchKernelGGL(is_ident(a.g) ? ident : direct, dim3(p.grid), dim3(256), 0, s, a, partials);
    }
    if (stats_out) hipLaunchKernelGGL((reduce_partials_kernel<K>), dim3(1), dim3(256), 0, s, partials, p.grid, stats_out, extra, extra_slot);
}

// One backward of a family: its identity kernel over the flat pixel grid, or its tiled kernel once per colour class with
// G + R + `n_patches` rectangles (+ `lds_extra` bytes) of LDS. `tiled_extra`: what the tiled kernel takes behind the gradient.
template <class Args, class Ident, class Tiled, class... Extra>
inline int launch_bwd(const char* what, Ident ident, Tiled tiled, const Args& a, int n_patches, size_t lds_extra, const float* scalars,
                      float* grad, hipStream_t s, Extra... tiled_extra) {
    const Geo& g = a.g;
    if (is_ident(g)) {
        hipLaunchKernelGGL(ident, dim3(fwd_grid((size_t)g.n * g.H * g.W)), dim3(256), 0, s, a, scalars, grad);
        return CMS_OK;
    }
    size_t lds = tile_lds_bytes(g.c, g.sy, g.sx, n_patches);
    CMS_REQUIRE(lds <= TILE_LDS_MAX, "%s: %d classes at this scale need %zu B of LDS", what, g.c, lds);
    lds += lds_extra;
    allow_lds(tiled, lds);
    tiled_launches(g, [&](const Geo& gc, int tiles) {
        Args ac = a;
        ac.g = gc;
        hipLaunchKernelGGL(tiled, dim3(tiles), dim3(256), lds, s, ac, scalars, grad, tiled_extra...);
    });
    return CMS_OK;
}

// The one-launch forward + backward of a family over `tiles` tiles (`args`: what its kernel takes in front of the partials), and the
// reduction of its K partial sums.
template <int K, class Kern, class... Args>
inline void launch_fused(Kern kern, int tiles, size_t lds, hipStream_t s, float* partials, double* stats_out, double extra, int extra_slot,
                         Args... args) {
    allow_lds(kern, lds);
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(256), lds, s, args..., partials);
    hipLaunchKernelGGL((reduce_partials_kernel<K>), dim3(1), dim3(256), 0, s, partials, tiles, stats_out, extra, extra_slot);
}

}  // namespace cms
