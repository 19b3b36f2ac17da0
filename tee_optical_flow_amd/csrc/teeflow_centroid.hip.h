// teeflow_centroid.hip.h -- calc_AV_centroid of the reference on the device (/root/reference/optical_flow/analyze_optical_flow.py:202-244;
// host restatement tee_optical_flow_amd/analysis.py::av_centroids).  Per frame n of an AV mask [N][H][W][C]:
//   label the set mask[n, :, :, 0] != 0 with 8-connectivity (skimage.measure.label of a bool image = ndimage.label, 3x3 structure),
//   take the component of largest area -- on a tie the one whose first pixel in raster order comes first (ndimage numbers labels in
//   that order, np.argmax over regionprops areas takes the first maximum) -- and return its area and centroid
//   (sum of rows / area, sum of columns / area): 64-bit integer sums divided in double, which is what coords.mean(axis=0) gives
//   (every partial sum of its float64 reduction is an exact integer).
//
// The labelling is the 8-connected one of teeflow_ccl.hip.h.  What is only about centroids is here:
//   ChannelZeroSet  the set being labelled: channel 0 of the chunk's masks non-zero
//   AreaAndSums     accumulator: area, sum of rows, sum of columns per tile-local component in LDS (tile-relative, 32-bit), then one
//                   64-bit atomicAdd each per component
//   k_cent_pick     one block per frame: the root with the largest (area, -raster index) key
// Sums are integers: atomic order cannot change a bit.
#pragma once
#include "teeflow_ccl.hip.h"

namespace cen {

using ccl::NONE;
using ccl::TPX;

// m: the chunk's masks [nf][H][W][C] bytes; plane q of the chunk is its frame q
struct ChannelZeroSet {
    const uint8_t* __restrict__ m; int C; size_t HW;
    __device__ __forceinline__ bool operator()(int q, size_t p) const { return m[((size_t)q * HW + p) * C] != 0; }
};

// area[root] = the component's pixels, sums[root] = (sum of its rows, sum of its columns); clear() zeroes both for n pixels
struct AreaAndSums {
    static constexpr int WORDS = 4;                    // pixels, root, sum of rows, sum of columns
    uint32_t* __restrict__ area; unsigned long long* __restrict__ sums /* [nf][HW][2] */;
    hipError_t clear(size_t n, hipStream_t s) const
    {
        const hipError_t e = hipMemsetAsync(area, 0, n * 4, s);
        return e != hipSuccess ? e : hipMemsetAsync(sums, 0, n * 16, s);
    }
    __device__ static __forceinline__ void add(uint32_t* w, int li, uint32_t dy, uint32_t dx)
    {
        atomicAdd(w + 2 * TPX + li, dy);               // tile-relative: at most 1024 * 63, no overflow
        atomicAdd(w + 3 * TPX + li, dx);
    }
    __device__ __forceinline__ void component(int q, size_t HW, uint32_t r, const uint32_t* w, int i, int y0, int x0) const
    {
        const unsigned long long n = w[i];
        atomicAdd(area + (size_t)q * HW + r, w[i]);
        atomicAdd(sums + ((size_t)q * HW + r) * 2, (unsigned long long)w[2 * TPX + i] + n * (unsigned long long)y0);
        atomicAdd(sums + ((size_t)q * HW + r) * 2 + 1, (unsigned long long)w[3 * TPX + i] + n * (unsigned long long)x0);
    }
};

// grid (frames of the chunk): the winning component of frame q.  cent[q] = (rows / area, columns / area), area_out[q] = its area
// (0 and centroid (0, 0) for an empty frame).  Key: area in the high word, ~raster index of the root (= the component's first pixel)
// in the low word, so the largest key is the largest area and, on a tie, the earliest first pixel.
__global__ __launch_bounds__(256) void k_cent_pick(const uint32_t* __restrict__ par, const uint32_t* __restrict__ area,
                                                  const unsigned long long* __restrict__ sums, size_t HW, double* __restrict__ cent,
                                                  long long* __restrict__ area_out)
{
    __shared__ unsigned long long part[4];
    const int q = blockIdx.x;
    const uint32_t* P = par + (size_t)q * HW;
    const uint32_t* A = area + (size_t)q * HW;
    unsigned long long best = 0ull;
    for (size_t p = threadIdx.x; p < HW; p += 256) {
        if (P[p] != (uint32_t)p) continue;             // roots only (NONE is never an index: HW < 2^31)
        const unsigned long long key = ((unsigned long long)A[p] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)p);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) best = part[w] > best ? part[w] : best;
    if (best == 0ull) {
        cent[2 * q] = 0.0; cent[2 * q + 1] = 0.0; area_out[q] = 0;
        return;
    }
    const uint32_t r = 0xffffffffu - (uint32_t)(best & 0xffffffffull);
    const unsigned long long a = best >> 32;
    const unsigned long long* S = sums + ((size_t)q * HW + r) * 2;
    cent[2 * q] = (double)S[0] / (double)a;
    cent[2 * q + 1] = (double)S[1] / (double)a;
    area_out[q] = (long long)a;
}

}  // namespace cen
