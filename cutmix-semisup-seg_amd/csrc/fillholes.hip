// Hole filling of binary predictions (gfx950): scipy.ndimage.binary_fill_holes(pred != 0), default structure, on the device.
//   evaluation.py:53-55   EvaluatorIoU.sample with fill_holes (the ISIC 2017 configuration's --bin_fill_holes)
// A background pixel (value 0) survives iff it is 4-connected, through background pixels, to the outside of the image; every
// other background pixel is a hole and becomes 1. That is connected-component labelling of the background with one virtual
// "outside" node, done as a block-based union-find in three stream-ordered launches -- no host read-back, no cooperative launch,
// no workgroup ever waits for another, and the launch count does not depend on the image content:
//   A  fill_label_tiles    one workgroup per 64 x 64 tile: background mask as one 64-bit __ballot word per row in LDS, runs taken from
//                          the words with bit operations, vertical unions in an LDS union-find, then the global parent of every pixel
//   B  fill_merge_seams    unions across tile edges and of image-edge pixels with the outside node (atomicCAS on the parents)
//   C  fill_resolve        out = foreground || find(pixel) != outside; optionally the 2 x 2 histogram against a truth map
// Parent array (int32, caller's workspace): per image h*w + 1 nodes; node 0 is the outside, pixel i is node i + 1; -1 marks a
// foreground pixel (never a node).
//
// INVARIANT (every loop below leans on it): parent[x] <= x, with equality only at roots. A union links the LARGER root under the
// smaller node, a path shortcut replaces a parent by one of its ancestors (smaller still), and nothing else writes a parent. So
// a walk x -> parent[x] descends strictly and ends at a root after at most x steps, whatever other workgroups do meanwhile, and
// the outside node (0, the smallest) is the root of everything connected to it.
#include "common.hpp"

namespace cms {

constexpr int kFillTile = 64;              // tile edge = wave width: one __ballot word is one tile row
constexpr int kFillFg = -1;                // parent value of a foreground pixel

// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for the LDS forest of launch A, __HIP_MEMORY_SCOPE_AGENT for the global one of launch B.
// The loads are atomic (relaxed) so that the compiler cannot keep a parent in a register while other waves / workgroups merge.
template <int SCOPE>
__device__ __forceinline__ int uf_load(int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, SCOPE);
}

// Root of x, shortcutting every visited node to its grandparent on the way (path halving).
// Terminates: p = parent[x] < x whenever the loop body runs (invariant), and x takes the value p, so x descends strictly.
// The shortcut keeps the invariant: gp <= p < x, gp is an ancestor of x, and the min never raises a parent. It touches
// non-roots only (parent[x] = p != x, and a node that stopped being a root never becomes one again), so it cannot collide
// with the compare-and-swap of uf_union, which succeeds on roots only.
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* parent, int x) {
    int p = uf_load<SCOPE>(parent, x);
    while (p != x) {
        const int gp = uf_load<SCOPE>(parent, p);
        if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, SCOPE);
        x = p;
        p = gp;
    }
    return x;
}

// Unite the sets of a and b: the larger root is linked under the smaller one.
// Terminates: an iteration that does not return replaces the larger of the two roots by `seen`, the parent somebody else gave
// it in the meantime, and seen < hi (invariant); the finds never raise a or b. So a + b descends strictly and is >= 0.
// A link is made by compare-and-swap from "hi is its own parent", i.e. from roots only, so no link is ever lost.
template <int SCOPE>
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(parent, a);
        b = uf_find<SCOPE>(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return;
        a = expected;      // hi's new parent, < hi
        b = lo;
    }
}

// first column of the background run that holds column c (bit c of `row` set): one past the highest clear bit below c
__device__ __forceinline__ int run_start(unsigned long long row, int c) {
    const unsigned long long clear_below = ~row & ((1ull << c) - 1ull);
    return clear_below ? 64 - __builtin_clzll(clear_below) : 0;
}

// ---- launch A: one workgroup (4 waves) per 64 x 64 tile; grid = n * tiles_y * tiles_x ----
__global__ __launch_bounds__(256) void fill_label_tiles(const uint8_t* __restrict__ pred, int* __restrict__ parents, int H,
                                                        int W, int tiles_x, int tiles_y) {
    __shared__ unsigned long long mask[kFillTile];          // bit c of mask[r]: pixel (r, c) of the tile is background
    __shared__ int forest[kFillTile * kFillTile];           // LDS union-find over run starts, indexed r * 64 + c
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    const int img = b / tiles_y;
    const size_t plane = (size_t)H * W;
    const uint8_t* src = pred + (size_t)img * plane;
    int* parent = parents + (size_t)img * (plane + 1);
    const int x = tx * kFillTile + lane, y0 = ty * kFillTile;
    if (blockIdx.x % (tiles_x * tiles_y) == 0 && threadIdx.x == 0) parent[0] = 0;      // the outside node of this image

    // rows wave, wave + 4, ...: lanes beyond the image count as foreground, so they never become nodes and are never written
    for (int r = wave; r < kFillTile; r += 4) {
        const int y = y0 + r;
        const bool bg = y < H && x < W && src[(size_t)y * W + x] == 0;
        const unsigned long long word = __ballot(bg);
        if (lane == 0) mask[r] = word;
    }
    __syncthreads();
    for (int r = wave; r < kFillTile; r += 4) {
        const unsigned long long m = mask[r];
        if (((m >> lane) & 1ull) && (lane == 0 || !((m >> (lane - 1)) & 1ull))) forest[r * kFillTile + lane] = r * kFillTile + lane;
    }
    __syncthreads();
    // one union per pair of vertically touching runs: at the first column of each stretch where both rows are background
    for (int r = wave + 4 * (wave == 0); r < kFillTile; r += 4) {      // r >= 1
        const unsigned long long m = mask[r], up = mask[r - 1], both = m & up;
        if (((both >> lane) & 1ull) && (lane == 0 || !((both >> (lane - 1)) & 1ull)))
            uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(forest, r * kFillTile + run_start(m, lane),
                                                   (r - 1) * kFillTile + run_start(up, lane));
    }
    __syncthreads();
    for (int r = wave; r < kFillTile; r += 4) {
        const int y = y0 + r;
        if (y >= H || x >= W) continue;
        const unsigned long long m = mask[r];
        int node = kFillFg;
        if ((m >> lane) & 1ull) {
            // the root is the tile's smallest (row, column) of the component, hence also its smallest node: parent <= self
            const int root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(forest, r * kFillTile + run_start(m, lane));
            node = (y0 + root / kFillTile) * W + tx * kFillTile + root % kFillTile + 1;
        }
        parent[(size_t)y * W + x + 1] = node;
    }
}

// ---- launch B: one thread per seam item; per image  (tiles_x - 1) * H  +  (tiles_y - 1) * W  +  2 * W  +  2 * H  items ----
// An item is a pixel and its partner across a tile edge (or the outside node, for image-edge pixels). An item whose predecessor
// along the same seam is connected in the same way is skipped where launch A has already joined the two pixels on either side
// of the seam to their predecessors, i.e. where the step along the seam stays inside one tile: the union is then implied. At a
// tile corner that step crosses the other seam, whose item there could lean on this one in turn, so nothing is skipped there.
// Image-edge items skip behind ANY background predecessor: neighbours along the edge are joined by launch A or by a seam item,
// and seam items never lean on edge items.
__device__ __forceinline__ bool fill_is_bg(int* parent, int node) {
    return uf_load<__HIP_MEMORY_SCOPE_AGENT>(parent, node) != kFillFg;
}

__global__ __launch_bounds__(256) void fill_merge_seams(int* __restrict__ parents, int N, int H, int W, int tiles_x,
                                                        int tiles_y) {
    const int n_vert = (tiles_x - 1) * H, n_horz = (tiles_y - 1) * W;
    const int per_image = n_vert + n_horz + 2 * W + 2 * H;
    const size_t total = (size_t)N * per_image;
    const size_t plane = (size_t)H * W;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int img = (int)(idx / per_image);
        int i = (int)(idx % per_image);
        int* parent = parents + (size_t)img * (plane + 1);
        if (i < n_vert) {                                   // vertical seam: (y, x - 1) | (y, x), x a multiple of 64
            const int y = i % H, x = (i / H + 1) * kFillTile;
            const int a = y * W + x, b = a + 1;             // nodes of (y, x - 1) and (y, x)
            if (!fill_is_bg(parent, a) || !fill_is_bg(parent, b)) continue;
            if (y % kFillTile != 0 && fill_is_bg(parent, a - W) && fill_is_bg(parent, b - W)) continue;
            uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, a, b);
            continue;
        }
        i -= n_vert;
        if (i < n_horz) {                                   // horizontal seam: (y - 1, x) above (y, x), y a multiple of 64
            const int x = i % W, y = (i / W + 1) * kFillTile;
            const int b = y * W + x + 1, a = b - W;
            if (!fill_is_bg(parent, a) || !fill_is_bg(parent, b)) continue;
            if (x % kFillTile != 0 && fill_is_bg(parent, a - 1) && fill_is_bg(parent, b - 1)) continue;
            uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, a, b);
            continue;
        }
        i -= n_horz;
        int node, prev;                                     // image edge: the pixel and its predecessor along that edge
        if (i < 2 * W) {                                    // first and last row
            const int x = i % W, y = i < W ? 0 : H - 1;
            node = y * W + x + 1;
            prev = x > 0 ? node - 1 : 0;
        } else {                                            // first and last column
            i -= 2 * W;
            const int y = i % H, x = i < H ? 0 : W - 1;
            node = y * W + x + 1;
            prev = y > 0 ? node - W : 0;
        }
        if (!fill_is_bg(parent, node)) continue;
        if (prev && fill_is_bg(parent, prev)) continue;
        uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, node, 0);
    }
}

// ---- launch C: the parents are final (kernel boundary), plain loads; reads neither pred nor writes a parent ----
__global__ __launch_bounds__(256) void fill_resolve(const int* __restrict__ parents, uint8_t* __restrict__ out,
                                                    const uint8_t* __restrict__ truth, int ignore_index, int N, int H, int W,
                                                    unsigned long long* __restrict__ cm) {
    __shared__ unsigned int hist[4];
    if (threadIdx.x < 4) hist[threadIdx.x] = 0;
    __syncthreads();
    const size_t plane = (size_t)H * W, P = (size_t)N * plane;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < P; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t img = idx / plane;
        const int* parent = parents + img * (plane + 1);
        int x = (int)(idx - img * plane) + 1;
        int p = parent[x];
        int filled = 1;
        if (p != kFillFg) {
            // terminates: p = parent[x] < x inside the loop (invariant; nothing writes parents in this launch), x descends strictly
            while (p != x) {
                x = p;
                p = parent[x];
            }
            filled = x != 0;
        }
        if (out) out[idx] = (uint8_t)filled;
        if (truth) {
            const int tr = truth[idx];
            if (tr != ignore_index && tr < 2) atomicAdd(&hist[tr * 2 + filled], 1u);
        }
    }
    __syncthreads();
    if (cm && threadIdx.x < 4) {
        const unsigned int v = hist[threadIdx.x];
        if (v) atomicAdd(&cm[threadIdx.x], (unsigned long long)v);
    }
}

// number of parent entries, or 0 when the geometry is bad or the node indices would not fit an int32
static long long fill_nodes(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const long long per_image = (long long)h * w + 1;
    if (per_image > 0x7fffffffLL / n) return 0;
    return per_image * n;
}

}  // namespace cms

using namespace cms;

extern "C" size_t cms_fill_holes_workspace_bytes(int n, int h, int w) {
    return (size_t)fill_nodes(n, h, w) * sizeof(int);
}

extern "C" int cms_fill_holes(const uint8_t* pred, uint8_t* out, const uint8_t* truth, int ignore_index, int64_t* cm, int n,
                              int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
    CMS_REQUIRE(pred, "fill_holes: pred NULL");
    CMS_REQUIRE(out || cm, "fill_holes: nothing to produce");
    CMS_REQUIRE(!truth || cm, "fill_holes: truth given without cm");
    CMS_REQUIRE(!cm || truth, "fill_holes: cm given without truth");
    CMS_REQUIRE(n > 0 && h > 0 && w > 0, "fill_holes: bad geometry");
    const long long nodes = fill_nodes(n, h, w);
    CMS_REQUIRE(nodes > 0, "fill_holes: n * (h * w + 1) must stay below 2^31");
    CMS_REQUIRE(workspace && workspace_bytes >= (size_t)nodes * sizeof(int), "fill_holes: workspace too small (%zu bytes needed)",
                (size_t)nodes * sizeof(int));
    const int tiles_x = (w + kFillTile - 1) / kFillTile, tiles_y = (h + kFillTile - 1) / kFillTile;
    hipStream_t s = (hipStream_t)stream;
    int* parents = (int*)workspace;
    // n * tiles_y * tiles_x <= nodes / 4096 + n * (tiles_x + tiles_y) < 2^31: fits the grid's x dimension
    hipLaunchKernelGGL(fill_label_tiles, dim3((unsigned)((size_t)n * tiles_y * tiles_x)), dim3(256), 0, s, pred, parents, h, w,
                       tiles_x, tiles_y);
    const size_t seam_items = (size_t)n * ((size_t)(tiles_x - 1) * h + (size_t)(tiles_y - 1) * w + 2 * (size_t)w + 2 * (size_t)h);
    hipLaunchKernelGGL(fill_merge_seams, dim3(grid_for(seam_items, 256, 1024)), dim3(256), 0, s, parents, n, h, w, tiles_x,
                       tiles_y);
    hipLaunchKernelGGL(fill_resolve, dim3(grid_for((size_t)n * h * w, 256, 1024)), dim3(256), 0, s, parents, out, truth,
                       ignore_index, n, h, w, (unsigned long long*)cm);
    return launch_status("cms_fill_holes");
}
