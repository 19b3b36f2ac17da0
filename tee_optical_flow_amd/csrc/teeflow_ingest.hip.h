// teeflow_ingest.hip.h -- k_ingest: a study's frames as the file stores them (RGB, grey, YBR_FULL) -> uint8 RGB [N][H][W][3], columns
// mirrored on request (tf_hold_frames, teeflow_frames_host.hip.h).  The pixel arithmetic and the lane's loads and stores are
// teeflow_ingest_core.h's, the same text the host checker compiles.  Memory-bound: 1 or 3 bytes in, 3 bytes out per pixel.
#pragma once
#define TFG_FN __device__ __forceinline__
#define TFG_FMA(a, b, c) __fmaf_rn((a), (b), (c))
#include "teeflow_ingest_core.h"

namespace tfg {
// grid ceil(ceil(npx / 4) / 256): a lane takes 4 consecutive pixels of the npx = N * H * W (ingest_lane)
template <int FORM, bool FLIP>
__global__ __launch_bounds__(256) void k_ingest(const uint8_t* __restrict__ src, size_t npx, int W, uint8_t* __restrict__ out)
{
    ingest_lane<FORM, FLIP>(src, npx, W, (size_t)blockIdx.x * 256 + threadIdx.x, out);
}

// the same from sample planes [N][3][hw], hw = H * W (k_rle_decode's scratch): the interleave is this kernel's, not the decoder's
template <int FORM, bool FLIP>
__global__ __launch_bounds__(256) void k_ingest_planar(const uint8_t* __restrict__ src, size_t npx, int W, size_t hw, uint8_t* __restrict__ out)
{
    ingest_lane<FORM, FLIP, true>(src, npx, W, (size_t)blockIdx.x * 256 + threadIdx.x, out, hw);
}
}  // namespace tfg
