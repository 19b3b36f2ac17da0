// teeflow_area.hip.h -- the per-frame area loop of AreaDetector.detect of the reference on the device
// (/root/reference/optical_flow/cardiac_cycle_detection.py:159-172; host restatement tee_optical_flow_amd/analysis.py::area_series).
// Per frame n of a mask [N][H][W][C] the reference takes skimage.measure.label(mask[n, :, :, 0]), regionprops, props[0].area:
//   label joins 8-connected pixels of EQUAL value (0 is background) and numbers the regions by their first pixel in raster order, so
//   props[0] is the region that owns the frame's first non-zero pixel -- the seed -- whatever its size: the 8-connected component of
//   {mask == value at the seed} that contains the seed.
//
// The labelling is the 8-connected one of teeflow_ccl.hip.h.  What is only about this area is here:
//   k_area_seed    one block per frame: the seed (smallest raster index with a non-zero byte), its value, and the frame's area word zeroed
//   SeedValueSet   the set being labelled: channel 0 equal to the frame's seed value (nothing in a frame without a seed)
//   SeedArea       accumulator: a tile-local component's pixel count goes to the frame's area when the component's root is the seed.
//                  The seed is the smallest index of its set and the labelling's root is the smallest index of a component, so the
//                  seed is its own root.  One integer atomicAdd per tile the region touches; no per-root array, nothing to clear.
// Sums are integers: atomic order cannot change a bit.
#pragma once
#include "teeflow_ccl.hip.h"

namespace fra {

using ccl::NONE;
using ccl::TPX;

constexpr int SEG = 16 * 256;                          // pixels a block scans between two looks at whether it has a seed

// grid (frames of the chunk): seed[q] = the smallest p with m[(q * HW + p) * C] != 0 (NONE for an empty frame), val[q] = that byte
// (0 for an empty frame), area[q] = 0.  The frame is scanned in segments of SEG pixels, in raster order; the first segment with a
// non-zero byte ends the scan.  Every thread reads the same four partial minima, so the decision is uniform over the block.
__global__ __launch_bounds__(256) void k_area_seed(const uint8_t* __restrict__ m, int C, size_t HW, uint32_t* __restrict__ seed,
                                                  uint8_t* __restrict__ val, unsigned long long* __restrict__ area)
{
    __shared__ uint32_t part[4];
    const int q = blockIdx.x;
    const uint8_t* M = m + (size_t)q * HW * C;
    uint32_t found = NONE;
    for (size_t base = 0; base < HW && found == NONE; base += SEG) {
        uint32_t best = NONE;
#pragma unroll 4
        for (int k = 0; k < SEG / 256; ++k) {
            const size_t p = base + (size_t)k * 256 + threadIdx.x;
            if (p < HW && M[p * C] != 0 && (uint32_t)p < best) best = (uint32_t)p;   // (HW < 2^31: an index is never NONE)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_down(best, off, 64);
            best = o < best ? o : best;
        }
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
        __syncthreads();
        for (int w = 0; w < 4; ++w) found = part[w] < found ? part[w] : found;
        __syncthreads();                               // part is written again in the next segment
    }
    if (threadIdx.x != 0) return;
    seed[q] = found;
    val[q] = found == NONE ? (uint8_t)0 : M[(size_t)found * C];
    area[q] = 0ull;
}

// m: the chunk's masks [nf][H][W][C] bytes; plane q of the chunk is its frame q
struct SeedValueSet {
    const uint8_t* __restrict__ m; const uint32_t* __restrict__ seed; const uint8_t* __restrict__ val; int C; size_t HW;
    __device__ __forceinline__ bool operator()(int q, size_t p) const { return seed[q] != NONE && m[((size_t)q * HW + p) * C] == val[q]; }
};

// area[q] = the pixels of the component whose root is seed[q]; k_area_seed zeroed it.  (The count fits 32 bits; the word is 64 wide so
// that the words are the call's int64 output as they stand.)
struct SeedArea {
    static constexpr int WORDS = 2;                    // pixels, root
    const uint32_t* __restrict__ seed; unsigned long long* __restrict__ area;
    hipError_t clear(size_t, hipStream_t) const { return hipSuccess; }
    __device__ __forceinline__ void component(int q, size_t, uint32_t r, const uint32_t* w, int i, int, int) const
    {
        if (r == seed[q]) atomicAdd(area + q, (unsigned long long)w[i]);
    }
};

}  // namespace fra
