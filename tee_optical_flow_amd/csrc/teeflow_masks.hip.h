// teeflow_masks.hip.h -- clean_mask of the reference on the device (/root/reference/optical_flow/calculate_optical_flow.py:90-111,
// :113-182; host restatement tee_optical_flow_amd/masks.py).  For every (label, frame) plane of a class map:
//   m      = moving_avg_mask(arr == cls) with its defaults: count of set frames among clamp(j-1), j, clamp(j+1), clamp(j+2), / 4 > 0.49
//   filled = binary_fill_holes(m): background not 4-connected to the image border becomes foreground
//   clean  = remove_small_objects(filled, min_size): 4-connected foreground components of fewer than min_size pixels are dropped
// and the store writes clean (and bkgd = not OR over the labels) with the channel duplicated: 0x0101 per pixel.
//
// Both morphological steps are one 4-connected component labelling of a plane by the kernels of teeflow_ccl.hip.h (fill holes: of the
// background of m; small objects: of the foreground of filled).  What is only about masks is here:
//   ClassWindowBackground   the set of the first labelling: the background of m, the temporal window fused into the load
//   FilledByLabels          the set of the second labelling, read from the first one's parents and border flags
//   BorderFlag              accumulator of the first labelling: flags roots with a pixel on the image border
//   ComponentSize           accumulator of the second labelling: counts component sizes
//   k_mask_store            the clean planes and bkgd from the second labelling's roots and sizes
// Outputs are booleans: atomic order cannot change a bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "teeflow_ccl.hip.h"

namespace msk {

using ccl::NONE;

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
// The set that the second labelling works on: filled = m or background not flagged as touching the border, that is par[p] == NONE
// (p in m) or aux[par[p]] == 0 in the first labelling's parents and flags.  par is the array that k_ccl_local then overwrites.
struct FilledByLabels {
    const uint32_t* par; const uint32_t* __restrict__ aux;
    size_t HW;
    __device__ __forceinline__ bool operator()(int q, size_t p) const
    {
        const uint32_t r = par[(size_t)q * HW + p];
        return r == NONE || aux[(size_t)q * HW + r] == 0u;
    }
};

// Accumulators of k_ccl_flatten; clear() zeroes the totals of n pixels (all planes of the call) on the stream.
// aux[root] = 1 for a component with a pixel on the image border
struct BorderFlag {
    static constexpr int WORDS = 0;
    uint32_t* __restrict__ aux;
    hipError_t clear(size_t n, hipStream_t s) const { return hipMemsetAsync(aux, 0, n * 4, s); }
    __device__ __forceinline__ void pixel(int q, size_t HW, uint32_t r, int x, int y, int H, int W) const
    {
        if (x == 0 || y == 0 || x == W - 1 || y == H - 1) aux[(size_t)q * HW + r] = 1u;
    }
};
// aux[root] = the component's pixels
struct ComponentSize {
    static constexpr int WORDS = 2;
    uint32_t* __restrict__ aux;
    hipError_t clear(size_t n, hipStream_t s) const { return hipMemsetAsync(aux, 0, n * 4, s); }
    __device__ __forceinline__ void component(int q, size_t HW, uint32_t r, const uint32_t* w, int i, int, int) const
    {
        atomicAdd(aux + (size_t)q * HW + r, w[i]);
    }
};

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
