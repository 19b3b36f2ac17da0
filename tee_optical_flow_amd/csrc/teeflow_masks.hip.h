// teeflow_masks.hip.h -- clean_mask of the reference on the device (/root/reference/optical_flow/calculate_optical_flow.py:90-111,
// :113-182; host restatement tee_optical_flow_amd/masks.py).  For every (label, frame) plane of a class map:
//   m      = moving_avg_mask(arr == cls) with its defaults: count of set frames among clamp(j-1), j, clamp(j+1), clamp(j+2), / 4 > 0.49
//   filled = binary_fill_holes(m): background not 4-connected to the image border becomes foreground
//   clean  = remove_small_objects(filled, min_size): 4-connected foreground components of fewer than min_size pixels are dropped
// and the store writes clean (and bkgd = not OR over the labels) with the channel duplicated: 0x0101 per pixel.
//
// Both morphological steps are one 4-connected component labelling of a plane (fill holes: of the background of m; small objects: of
// the foreground of filled).  The labelling is the block-based union-find of Playne & Hawick (IEEE TPDS 2018):
//   k_mask_local   64 x 16 tile in LDS: lock-free atomicMin union, root = smallest raster index; par[p] = global index of p's tile root
//   k_mask_merge   tile edges: the same union on the global parent array (parents only decrease, so every loop is bounded)
//   k_mask_flatten par[p] = final root; pass 0 flags roots with a pixel on the image border, pass 1 counts component sizes (one atomicAdd
//                  per tile-local component, counted in LDS first: a blob's root is otherwise one hot address)
// Every union / find loop carries an explicit bound; running out sets *err instead of hanging.  Outputs are booleans: atomic order
// cannot change a bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msk {

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

// The set that the first labelling of a plane works on, as a functor in(q, p): plane q of the chunk, pixel p of the frame.
// clean_mask: the background of m, computed from the class map (the temporal window is fused into the load); plane q = label q / nf,
// frame f0 + q % nf of the chunk.
struct ClassWindowBackground {
    const uint8_t* __restrict__ cls; const uint8_t* __restrict__ ids;
    int N, f0, nf; size_t HW;
    __device__ __forceinline__ bool operator()(int q, size_t p) const
    {
        const int l = q / nf, f = f0 + q % nf;
        const uint8_t c = ids[l];
        const int fa = f > 0 ? f - 1 : 0, fc = f + 1 < N ? f + 1 : N - 1, fd = f + 2 < N ? f + 2 : N - 1;
        const int count = (cls[(size_t)fa * HW + p] == c) + (cls[(size_t)f * HW + p] == c) + (cls[(size_t)fc * HW + p] == c) +
                          (cls[(size_t)fd * HW + p] == c);
        return !((double)count / 4.0 > 0.49);          // numpy: float64 window sum / n > threshold; the set is m's background
    }
};
struct NoSet {                                         // PASS 1 derives its set from PASS 0's labelling, not from an input
    __device__ __forceinline__ bool operator()(int, size_t) const { return false; }
};

// grid (tiles, planes).
// PASS 0: the set is the background of m, as `set` gives it.
// PASS 1: the set is filled = m or background not flagged as touching the border: par[p] == NONE (p in m) or aux[par[p]] == 0.  Also
//         writes lr[p] = p's root inside the tile (tile-local index) for the size count of k_mask_flatten<1>.
template <int PASS, class Set>
__global__ __launch_bounds__(256) void k_mask_local(const Set set, uint32_t* __restrict__ par, const uint32_t* __restrict__ aux,
                                                   uint16_t* __restrict__ lr, int H, int W, int tiles_x, unsigned* err)
{
    __shared__ uint32_t lp[TPX];
    const int q = blockIdx.y;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)q * HW;
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        bool v = false;
        if (x < W && y < H) {
            const size_t p = (size_t)y * W + x;
            if (PASS == 0) {
                v = set(q, p);
            } else {
                const uint32_t r = P[p];
                v = r == NONE || aux[(size_t)q * HW + r] == 0u;
            }
        }
        in[k] = v;
        lp[i] = v ? (uint32_t)i : NONE;
    }
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (!in[k]) continue;
        if ((i & (TW - 1)) > 0 && lds_ld(lp + i - 1) != NONE) ok &= unite<true>(lp, i, i - 1, 2 * TPX);
        if (i >= TW && lds_ld(lp + i - TW) != NONE) ok &= unite<true>(lp, i, i - TW, 2 * TPX);
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
            if (PASS == 1) lr[(size_t)q * HW + p] = (uint16_t)r;
        } else
            P[p] = NONE;
    }
    if (!ok) atomicOr(err, 1u);
}

// grid (tiles, planes): the tile's top edge against the row above, its left edge against the column to the left
__global__ __launch_bounds__(256) void k_mask_merge(uint32_t* __restrict__ par, int H, int W, int tiles_x, unsigned* err)
{
    const int t = threadIdx.x;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)blockIdx.y * HW;
    uint32_t a = NONE, b = NONE;
    if (t < TW) {
        const int x = x0 + t;
        if (y0 > 0 && x < W) { a = (uint32_t)y0 * W + x; b = a - W; }
    } else if (t < TW + TH) {
        const int y = y0 + t - TW;
        if (x0 > 0 && y < H) { a = (uint32_t)y * W + x0; b = a - 1; }
    }
    if (a == NONE || glb_ld(P + a) == NONE || glb_ld(P + b) == NONE) return;
    if (!unite<false>(P, a, b, (uint32_t)(2 * HW < 0xfffffffeu ? 2 * HW : 0xfffffffeu))) atomicOr(err, 2u);
}

// grid (tiles, planes): par[p] = the final root of p.  PASS 0: aux[root] = 1 for a component with a pixel on the image border.
// PASS 1: aux[root] += the component's pixels (aux zeroed before), counted per tile-local root in LDS first.
template <int PASS>
__global__ __launch_bounds__(256) void k_mask_flatten(uint32_t* __restrict__ par, uint32_t* __restrict__ aux, const uint16_t* __restrict__ lr,
                                                     int H, int W, int tiles_x)
{
    __shared__ uint32_t cnt[PASS == 1 ? TPX : 1], root[PASS == 1 ? TPX : 1];
    const int q = blockIdx.y;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)q * HW;
    uint32_t* A = aux + (size_t)q * HW;
    const uint32_t bound = (uint32_t)(HW < 0xfffffffeu ? HW : 0xfffffffeu);
    if (PASS == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[threadIdx.x + 256 * k] = 0u;
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
        if (PASS == 0) {
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) A[r] = 1u;
        } else {
            const int li = lr[(size_t)q * HW + p];
            root[li] = r;                              // (every pixel of that tile-local component writes the same root)
            atomicAdd(cnt + li, 1u);
        }
        P[p] = r;
    }
    if (PASS == 1) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = threadIdx.x + 256 * k;
            if (cnt[i]) atomicAdd(A + root[i], cnt[i]);
        }
    }
}

// grid (ceil(H*W / 256), nf): per pixel of a frame of the chunk, every label's clean mask and bkgd, both channels at once.
// out: [n_labels + 1][nf][H*W] x uint16 (0x0101 = true in both bytes)
__global__ __launch_bounds__(256) void k_mask_store(const uint32_t* __restrict__ par, const uint32_t* __restrict__ aux, int n_labels, int nf,
                                                   size_t HW, long long min_size, uint16_t* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int fi = blockIdx.y;
    bool any = false;
    for (int l = 0; l < n_labels; ++l) {
        const size_t q = (size_t)l * nf + fi;
        const uint32_t r = par[q * HW + p];
        const bool keep = r != NONE && (long long)aux[q * HW + r] >= min_size;
        any |= keep;
        out[q * HW + p] = keep ? 0x0101 : 0;
    }
    out[((size_t)n_labels * nf + fi) * HW + p] = any ? 0 : 0x0101;
}

}  // namespace msk
