// teeflow_ccl.hip.h -- connected-component labelling of planes on the device: the one implementation behind tf_clean_masks,
// tf_otsu_masks (4-connected, two labellings per plane) and tf_av_centroids (8-connected, one).  It is the block-based union-find of
// Playne & Hawick (IEEE TPDS 2018):
//   k_ccl_local    64 x 16 tile in LDS: lock-free atomicMin union, root = smallest raster index; par[p] = global index of p's tile root
//   k_ccl_merge    tile edges: the same union on the global parent array (parents only decrease, so every loop is bounded)
//   k_ccl_flatten  par[p] = final root, and what the components collect meanwhile: an accumulator policy (below)
// Compile-time parameters: the connectivity CONN (4: left and upper neighbour; 8: the two upper diagonals as well), the set being
// labelled as a functor in(q, p) -- plane q of the chunk, pixel p of the plane -- and the accumulator.
// Every union / find loop carries an explicit bound; running out sets *err (bit 1: k_ccl_local, bit 2: k_ccl_merge) instead of
// hanging.  What leaves the atomics are flags and integer sums: their order cannot change a bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ccl {

constexpr int TW = 64, TH = 16, TPX = TW * TH;   // tile: 256 threads x 4 pixels, a wave per 64-pixel row
constexpr uint32_t NONE = 0xffffffffu;          // "not in the set being labelled"

__device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t glb_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of i: parents strictly decrease, so a path has at most `bound` steps
template <bool LDS>
__device__ __forceinline__ uint32_t find_root(const uint32_t* par, uint32_t i, uint32_t bound)
{
    for (uint32_t s = 0; s < bound; ++s) {
        const uint32_t q = LDS ? lds_ld(par + i) : glb_ld(par + i);
        if (q == i) break;
        i = q;
    }
    return i;
}

// joins the sets of a and b (larger root under the smaller); false if the bound ran out (cannot happen: each failed try means another
// link was made, and a plane has fewer than `bound` of them)
template <bool LDS>
__device__ __forceinline__ bool unite(uint32_t* par, uint32_t a, uint32_t b, uint32_t bound)
{
    for (uint32_t it = 0; it < bound; ++it) {
        a = find_root<LDS>(par, a, bound);
        b = find_root<LDS>(par, b, bound);
        if (a == b) return true;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(par + a, b);
        if (old == a) return true;
        a = old;                                       // a was linked meanwhile: go on from what it was linked to
    }
    return false;
}

// grid (tiles, planes): par[p] = global index of p's tile root, NONE outside the set; LR: also lr[p] = that root's tile-local index,
// for an accumulator that counts per tile-local component.
// `set` may read the parents of an earlier labelling from par itself (msk::FilledByLabels), so par is not __restrict__: a thread
// evaluates the set on its own four pixels before it writes them, and reads and writes no other pixel of par.
template <int CONN, bool LR, class Set>
__global__ __launch_bounds__(256) void k_ccl_local(const Set set, uint32_t* par, uint16_t* __restrict__ lr, int H, int W, int tiles_x, unsigned* err)
{
    static_assert(CONN == 4 || CONN == 8, "connectivity");
    __shared__ uint32_t lp[TPX];
    const int q = blockIdx.y;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)q * HW;
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        const bool v = x < W && y < H && set(q, (size_t)y * W + x);
        in[k] = v;
        lp[i] = v ? (uint32_t)i : NONE;
    }
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, lx = i & (TW - 1);
        if (!in[k]) continue;
        if (lx > 0 && lds_ld(lp + i - 1) != NONE) ok &= unite<true>(lp, i, i - 1, 2 * TPX);
        if (i >= TW) {
            if (lds_ld(lp + i - TW) != NONE) ok &= unite<true>(lp, i, i - TW, 2 * TPX);
            if (CONN == 8 && lx > 0 && lds_ld(lp + i - TW - 1) != NONE) ok &= unite<true>(lp, i, i - TW - 1, 2 * TPX);
            if (CONN == 8 && lx < TW - 1 && lds_ld(lp + i - TW + 1) != NONE) ok &= unite<true>(lp, i, i - TW + 1, 2 * TPX);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        if (x >= W || y >= H) continue;
        const size_t p = (size_t)y * W + x;
        if (in[k]) {
            const uint32_t r = find_root<true>(lp, i, TPX);
            P[p] = (uint32_t)(y0 + (int)r / TW) * (uint32_t)W + (uint32_t)(x0 + (int)(r & (TW - 1)));
            if (LR) lr[(size_t)q * HW + p] = (uint16_t)r;
        } else
            P[p] = NONE;
    }
    if (!ok) atomicOr(err, 1u);
}

// grid (tiles, planes): threads 0-63 take the tile's top row against the row above, threads 64-79 its left column against the column
// to the left.  CONN 4: the one neighbour straight across the edge; CONN 8: the three across it, corners included, so that every
// 8-neighbour pair that spans two tiles is met.  Pairs inside one tile were joined by k_ccl_local; pairs met twice are harmless.
template <int CONN>
__global__ __launch_bounds__(256) void k_ccl_merge(uint32_t* __restrict__ par, int H, int W, int tiles_x, unsigned* err)
{
    static_assert(CONN == 4 || CONN == 8, "connectivity");
    const int t = threadIdx.x;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)blockIdx.y * HW;
    int x, y;
    const bool top = t < TW;
    if (top) {
        x = x0 + t; y = y0;
        if (y0 == 0 || x >= W) return;
    } else if (t < TW + TH) {
        x = x0; y = y0 + t - TW;
        if (x0 == 0 || y >= H) return;
    } else
        return;
    const uint32_t a = (uint32_t)y * W + x;
    if (glb_ld(P + a) == NONE) return;
    const uint32_t bound = (uint32_t)(2 * HW < 0xfffffffeu ? 2 * HW : 0xfffffffeu);
    constexpr int D = CONN == 8 ? 1 : 0;
    bool ok = true;
#pragma unroll
    for (int d = -D; d <= D; ++d) {
        const int nx = top ? x + d : x - 1, ny = top ? y - 1 : y + d;
        if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
        const uint32_t b = (uint32_t)ny * W + nx;
        if (glb_ld(P + b) == NONE) continue;
        ok &= unite<false>(P, a, b, bound);
    }
    if (!ok) atomicOr(err, 2u);
}

// grid (tiles, planes): par[p] = the final root of p.  The accumulator policy Acc says what a component collects on the way:
//   Acc::WORDS                              LDS words per tile-local component (the kernel's LDS is WORDS x 4 KiB)
//   WORDS == 0: acc.pixel(q, HW, r, x, y, H, W)      per pixel (x, y) of the set, r its root
//   WORDS >= 2: word 0 counts the component's pixels in the tile and word 1 holds its root; k_ccl_local's lr names the component.
//               Acc::add(w, li, dy, dx)              WORDS > 2: adds the pixel at tile-relative (dy, dx) to words 2.. of component li
//               acc.component(q, HW, r, w, i, y0, x0)  once per tile-local component i with pixels: adds its words to root r's totals
//               (one global atomic per total and tile-local component: a blob's root is otherwise one hot address)
// The totals are zeroed before.  Instances: msk::BorderFlag, msk::ComponentSize, cen::AreaAndSums.
template <class Acc>
__global__ __launch_bounds__(256) void k_ccl_flatten(uint32_t* __restrict__ par, const uint16_t* __restrict__ lr, const Acc acc, int H, int W,
                                                    int tiles_x)
{
    constexpr int WORDS = Acc::WORDS;
    __shared__ uint32_t w[WORDS ? WORDS * TPX : 1];    // [WORDS][TPX]
    const int q = blockIdx.y;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)q * HW;
    const uint32_t bound = (uint32_t)(HW < 0xfffffffeu ? HW : 0xfffffffeu);
    if constexpr (WORDS != 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + 256 * k;
            w[i] = 0u;
#pragma unroll
            for (int j = 2; j < WORDS; ++j) w[j * TPX + i] = 0u;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        if (x >= W || y >= H) continue;
        const size_t p = (size_t)y * W + x;
        const uint32_t l = P[p];                       // only this thread writes par[p]; other threads may read it (an ancestor either way)
        if (l == NONE) continue;
        const uint32_t r = find_root<false>(P, l, bound);
        if constexpr (WORDS == 0) {
            acc.pixel(q, HW, r, x, y, H, W);
        } else {
            const int li = lr[(size_t)q * HW + p];
            w[TPX + li] = r;                           // (every pixel of that tile-local component writes the same root)
            atomicAdd(w + li, 1u);
            if constexpr (WORDS > 2) Acc::add(w, li, (uint32_t)(y - y0), (uint32_t)(x - x0));
        }
        P[p] = r;
    }
    if constexpr (WORDS != 0) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + 256 * k;
            if (w[i]) acc.component(q, HW, w[TPX + i], w, i, y0, x0);
        }
    }
}

}  // namespace ccl
