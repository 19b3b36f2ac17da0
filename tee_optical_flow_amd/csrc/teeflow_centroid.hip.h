// teeflow_centroid.hip.h -- calc_AV_centroid of the reference on the device (/root/reference/optical_flow/analyze_optical_flow.py:202-244;
// host restatement tee_optical_flow_amd/analysis.py::av_centroids).  Per frame n of an AV mask [N][H][W][C]:
//   label the set mask[n, :, :, 0] != 0 with 8-connectivity (skimage.measure.label of a bool image = ndimage.label, 3x3 structure),
//   take the component of largest area -- on a tie the one whose first pixel in raster order comes first (ndimage numbers labels in
//   that order, np.argmax over regionprops areas takes the first maximum) -- and return its area and centroid
//   (sum of rows / area, sum of columns / area): 64-bit integer sums divided in double, which is what coords.mean(axis=0) gives
//   (every partial sum of its float64 reduction is an exact integer).
//
// The labelling is the block union-find of teeflow_masks.hip.h (its helpers are shared; its kernels are untouched), with the diagonal
// unions added:
//   k_cent_local    64 x 16 tile in LDS: unions with the left, upper, upper-left and upper-right neighbour; root = smallest raster index
//   k_cent_merge    a tile's top row against its three upper neighbours each (corners included), its left column against its three left
//                   neighbours each: every 8-neighbour pair that spans two tiles is one of these
//   k_cent_flatten  par[p] = final root; area, sum of rows, sum of columns per tile-local component in LDS (tile-relative, 32-bit),
//                   then one 64-bit atomicAdd each per component
//   k_cent_pick     one block per frame: the root with the largest (area, -raster index) key
// Every union / find loop carries an explicit bound; running out sets *err instead of hanging.  Sums are integers: atomic order cannot
// change a bit.
#pragma once
#include "teeflow_masks.hip.h"

namespace cen {

using msk::NONE;
using msk::TH;
using msk::TPX;
using msk::TW;

// grid (tiles, frames of the chunk); m: the chunk's masks [nf][H][W][C] bytes, the set is channel 0 != 0.
// par[p] = global index of p's tile root (NONE outside the set), lr[p] = that root's tile-local index.
__global__ __launch_bounds__(256) void k_cent_local(const uint8_t* __restrict__ m, int C, uint32_t* __restrict__ par, uint16_t* __restrict__ lr,
                                                   int H, int W, int tiles_x, unsigned* err)
{
    __shared__ uint32_t lp[TPX];
    const int q = blockIdx.y;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    const uint8_t* M = m + (size_t)q * HW * C;
    uint32_t* P = par + (size_t)q * HW;
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        const bool v = x < W && y < H && M[((size_t)y * W + x) * C] != 0;
        in[k] = v;
        lp[i] = v ? (uint32_t)i : NONE;
    }
    __syncthreads();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, lx = i & (TW - 1);
        if (!in[k]) continue;
        if (lx > 0 && msk::lds_ld(lp + i - 1) != NONE) ok &= msk::unite<true>(lp, i, i - 1, 2 * TPX);
        if (i >= TW) {
            if (msk::lds_ld(lp + i - TW) != NONE) ok &= msk::unite<true>(lp, i, i - TW, 2 * TPX);
            if (lx > 0 && msk::lds_ld(lp + i - TW - 1) != NONE) ok &= msk::unite<true>(lp, i, i - TW - 1, 2 * TPX);
            if (lx < TW - 1 && msk::lds_ld(lp + i - TW + 1) != NONE) ok &= msk::unite<true>(lp, i, i - TW + 1, 2 * TPX);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        if (x >= W || y >= H) continue;
        const size_t p = (size_t)y * W + x;
        if (in[k]) {
            const uint32_t r = msk::find_root<true>(lp, i, TPX);
            P[p] = (uint32_t)(y0 + (int)r / TW) * (uint32_t)W + (uint32_t)(x0 + (int)(r & (TW - 1)));
            lr[(size_t)q * HW + p] = (uint16_t)r;
        } else
            P[p] = NONE;
    }
    if (!ok) atomicOr(err, 1u);
}

// grid (tiles, frames of the chunk): threads 0-63 take the tile's top row (upper-left, upper, upper-right neighbour), threads 64-79 its
// left column (upper-left, left, lower-left neighbour).  Pairs inside one tile were joined by k_cent_local; pairs met twice are harmless.
__global__ __launch_bounds__(256) void k_cent_merge(uint32_t* __restrict__ par, int H, int W, int tiles_x, unsigned* err)
{
    const int t = threadIdx.x;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)blockIdx.y * HW;
    int x, y, dx[3], dy[3];
    if (t < TW) {
        x = x0 + t; y = y0;
        if (y0 == 0 || x >= W) return;
        dx[0] = -1; dx[1] = 0; dx[2] = 1; dy[0] = dy[1] = dy[2] = -1;
    } else if (t < TW + TH) {
        x = x0; y = y0 + t - TW;
        if (x0 == 0 || y >= H) return;
        dx[0] = dx[1] = dx[2] = -1; dy[0] = -1; dy[1] = 0; dy[2] = 1;
    } else
        return;
    const uint32_t a = (uint32_t)y * W + x;
    if (msk::glb_ld(P + a) == NONE) return;
    const uint32_t bound = (uint32_t)(2 * HW < 0xfffffffeu ? 2 * HW : 0xfffffffeu);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int nx = x + dx[j], ny = y + dy[j];
        if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
        const uint32_t b = (uint32_t)ny * W + nx;
        if (msk::glb_ld(P + b) == NONE) continue;
        ok &= msk::unite<false>(P, a, b, bound);
    }
    if (!ok) atomicOr(err, 2u);
}

// grid (tiles, frames of the chunk): par[p] = the final root of p; area[root] += pixels, sums[root] += (sum of rows, sum of columns),
// counted per tile-local component in LDS first (area and sums zeroed before)
__global__ __launch_bounds__(256) void k_cent_flatten(uint32_t* __restrict__ par, const uint16_t* __restrict__ lr, uint32_t* __restrict__ area,
                                                     unsigned long long* __restrict__ sums /* [nf][HW][2] */, int H, int W, int tiles_x)
{
    __shared__ uint32_t cnt[TPX], root[TPX], sy[TPX], sx[TPX];
    const int q = blockIdx.y;
    const int x0 = (blockIdx.x % tiles_x) * TW, y0 = (blockIdx.x / tiles_x) * TH;
    const size_t HW = (size_t)H * W;
    uint32_t* P = par + (size_t)q * HW;
    const uint32_t bound = (uint32_t)(HW < 0xfffffffeu ? HW : 0xfffffffeu);
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int i = threadIdx.x + 256 * k; cnt[i] = 0u; sy[i] = 0u; sx[i] = 0u; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k, x = x0 + (i & (TW - 1)), y = y0 + i / TW;
        if (x >= W || y >= H) continue;
        const size_t p = (size_t)y * W + x;
        const uint32_t l = P[p];                       // only this thread writes par[p]; other threads may read it (an ancestor either way)
        if (l == NONE) continue;
        const uint32_t r = msk::find_root<false>(P, l, bound);
        const int li = lr[(size_t)q * HW + p];
        root[li] = r;                                  // (every pixel of that tile-local component writes the same root)
        atomicAdd(cnt + li, 1u);
        atomicAdd(sy + li, (uint32_t)(y - y0));        // tile-relative: at most 1024 * 63, no overflow
        atomicAdd(sx + li, (uint32_t)(x - x0));
        P[p] = r;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (!cnt[i]) continue;
        const uint32_t r = root[i];
        atomicAdd(area + (size_t)q * HW + r, cnt[i]);
        atomicAdd(sums + ((size_t)q * HW + r) * 2, (unsigned long long)sy[i] + (unsigned long long)cnt[i] * (unsigned long long)y0);
        atomicAdd(sums + ((size_t)q * HW + r) * 2 + 1, (unsigned long long)sx[i] + (unsigned long long)cnt[i] * (unsigned long long)x0);
    }
}

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
