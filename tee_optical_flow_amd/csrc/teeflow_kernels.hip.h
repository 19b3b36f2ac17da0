// teeflow_kernels.hip.h -- gfx950 (MI355X) kernels of the DualTVL1 engine: what more than one solver uses (geometry and state
// types, small helpers, level-0 conversion, the pyramid, the float16 output helpers), then DualTVL1's stages, one header each:
// teeflow_tvl1_warp / _iter / _median / _out, and the study tail's conditioning kernels (teeflow_cond), included at the end.
//
// What they compute is OpenCV's CPU DualTVL1 as the reference reaches it through
// /root/reference/optical_flow/calculate_optical_flow.py:577-578, 642.
// Arithmetic contract: every float expression is evaluated in the written order with IEEE
// single/double operations and NO fused multiply-add (build flag -ffp-contract=off), so results
// are bit-identical to the CPU oracle in oracle/tvl1_oracle.c (which tests/ compare against).
//
// Data layout in HBM: every image-like quantity is a stack of fp32 planes [pair|frame][h][pitch],
// pitch = round_up(w, 32) floats (128-B rows, float4-aligned), plane = pitch*h.  Per level the
// engine keeps: the frame pyramid (I0/I1 share frames in sequence mode), three per-warp constants
// (I1wx, I1wy, rho_c -- |grad|^2 is recomputed, I1x/I1y are never materialised) and the
// ping-pong state u1,u2 (x2) and p11,p12,p21,p22 (x2).
//
// All kernels are HBM-bandwidth-bound stencils (no MFMA).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>

#define TF_HD __host__ __device__

typedef unsigned long long u64;

struct Geom {
    int w, h, pitch;
    long long plane;   // floats per frame plane of the pyramid (pitch*h of THIS level)
    long long splane;  // floats between consecutive pairs in the state/constant buffers (level-0 plane at
                       // every level, so pairs whose ping-pong parity differs never overlap across levels)
};

struct PairCtl {
    int ubase;  // which of the two u buffers holds this pair's current flow at stage start
    int pbase;  // same for the dual variable
};

struct StateBufs {
    float* u1[2]; float* u2[2];
    float* p11[2]; float* p12[2]; float* p21[2]; float* p22[2];
};

#define ERR_SCALE_F 1073741824.0f  // 2^30: per-pixel convergence term -> exact integer (oracle D1)
#define ERR_CAP_F 4096.0f

#define UNPACK4(dst, v) { dst[0] = (v).x; dst[1] = (v).y; dst[2] = (v).z; dst[3] = (v).w; }
#define PACK4(a) make_float4((a)[0], (a)[1], (a)[2], (a)[3])

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int cv_floor_f(float v) { int i = (int)v; return i - (i > v); }

// ---------------------------------------------------------------------------------------------
// u8 -> f32 (cv::Mat::convertTo(CV_32F, 1.0)): dense [F][H][W] bytes -> pitched fp32 planes
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_u8_to_f32(const uint8_t* __restrict__ src, float* __restrict__ dst, Geom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= g.w) return;
    dst[(size_t)f * g.plane + (size_t)y * g.pitch + x] = (float)src[((size_t)f * g.h + y) * g.w + x];
}

// CV_32FC1 frames.  cv2's DualTVL1 brings them to the 0..255 range, convertTo(CV_32F, 255.0) = one fp32 multiply per pixel (scale255);
// cv2's DeepFlow takes them as they are, convertTo(CV_32F) without a factor = a copy.
__global__ __launch_bounds__(256) void k_f32_to_level0(const float* __restrict__ src, float* __restrict__ dst, Geom g, int scale255)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= g.w) return;
    const float v = src[((size_t)f * g.h + y) * g.w + x];
    dst[(size_t)f * g.plane + (size_t)y * g.pitch + x] = scale255 ? v * 255.0f : v;
}

// ---------------------------------------------------------------------------------------------
// cv::resize INTER_LINEAR on CV_32FC1 (see oracle orc_resize_linear for the border rules)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float resize_px(const float* __restrict__ S, int sw, int sh, int spitch,
                                           int dx, int dy, double scale_x, double scale_y)
{
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = cv_floor_f(fx);
    fx -= (float)sx;
    bool tail = false;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx + 1 >= sw) { tail = true; if (sx >= sw - 1) { fx = 0.f; sx = sw - 1; } }
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int sy = cv_floor_f(fy);
    fy -= (float)sy;
    const float b0 = 1.f - fy, b1 = fy;
    const int r0 = sy >= 0 ? (sy < sh ? sy : sh - 1) : 0;
    const int r1 = sy + 1 >= 0 ? (sy + 1 < sh ? sy + 1 : sh - 1) : 0;
    const float* S0 = S + (size_t)r0 * spitch;
    const float* S1 = S + (size_t)r1 * spitch;
    float t0, t1;
    if (tail) { t0 = S0[sx]; t1 = S1[sx]; }
    else {
        const float a1 = fx, a0 = 1.f - fx;
        t0 = S0[sx] * a0 + S0[sx + 1] * a1;
        t1 = S1[sx] * a0 + S1[sx + 1] * a1;
    }
    return t0 * b0 + t1 * b1;
}

// cv::cuda::resize INTER_LINEAR as its resize_linear kernel samples (TF_VARIANT_CUDA only; oracle orc_resize_cuda, [UPSTREAM-FROM-MEMORY]):
// no half-pixel shift, replicate at the far edges, four weighted taps accumulated in float in upstream's order
__device__ __forceinline__ float resize_px_cuda(const float* __restrict__ S, int sw, int sh, int spitch, int dx, int dy, float scale_x, float scale_y)
{
    const float src_x = (float)dx * scale_x, src_y = (float)dy * scale_y;
    int x1 = cv_floor_f(src_x), y1 = cv_floor_f(src_y);
    x1 = x1 > sw - 1 ? sw - 1 : x1; y1 = y1 > sh - 1 ? sh - 1 : y1;
    const int x2 = x1 + 1, y2 = y1 + 1, x2r = x2 < sw - 1 ? x2 : sw - 1, y2r = y2 < sh - 1 ? y2 : sh - 1;
    const float* S1 = S + (size_t)y1 * spitch;
    const float* S2 = S + (size_t)y2r * spitch;
    float out = 0.f;
    out = out + S1[x1] * (((float)x2 - src_x) * ((float)y2 - src_y));
    out = out + S1[x2r] * ((src_x - (float)x1) * ((float)y2 - src_y));
    out = out + S2[x1] * (((float)x2 - src_x) * (src_y - (float)y1));
    out = out + S2[x2r] * ((src_x - (float)x1) * (src_y - (float)y1));
    return out;
}

// pyramid: one level down for every frame (cuda_sampling: the CUDA class's cuda::resize rule, scale = (float)(1/fx))
__global__ __launch_bounds__(256) void k_pyr_down(const float* __restrict__ src, Geom gs, float* __restrict__ dst, Geom gd,
                                                  double scale_x, double scale_y, int cuda_sampling = 0)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6), f = blockIdx.z;
    if (dx >= gd.w || dy >= gd.h) return;
    dst[(size_t)f * gd.plane + (size_t)dy * gd.pitch + dx] = cuda_sampling
        ? resize_px_cuda(src + (size_t)f * gs.plane, gs.w, gs.h, gs.pitch, dx, dy, (float)scale_x, (float)scale_y)
        : resize_px(src + (size_t)f * gs.plane, gs.w, gs.h, gs.pitch, dx, dy, scale_x, scale_y);
}

// ---- float16 forms of a study's payload (reference :400-404: the file stores `flow` and `echo` as float16) -----------------------
// One value of the flow output: the float32 product, rounded to float32 as numpy rounds `flows * np.float32(scale)`, then -- for a
// float16 destination -- that float32 rounded to half, nearest-even, subnormal halves kept (v_cvt_f16_f32; the library is built with
// -ffp-contract=off and there is no half arithmetic here): two roundings, numpy's `(flows * np.float32(scale)).astype(np.float16)`.
// The empty asm keeps the product in a register as a float32 of its own: without it the compiler folds multiply and conversion into one
// v_fma_mixlo_f16.  The guard is tests/test_gpu_payload.py::test_rounding_multiplies_in_float32_then_converts (scale 0.1 on 10^5 values,
// where one rounding and two differ): should a compiler fold the two again in spite of the asm, that test fails.
__device__ __forceinline__ uint32_t scaled_half_bits(float v, float scale)
{
    float prod = v * scale;
    asm volatile("" : "+v"(prod));
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)prod);
}

// A row of the float16 flow output, [w][2] halves from `row` on: thread t of the row takes the two pixels x0 = 2t - par and x0 + 1,
// par = the row's first pixel sitting on an odd 4-byte word -- so that a pair's four halves are one aligned 8-byte store whatever the
// width and the row (an odd width shifts every other row by one pixel); the pixel left over at either end of a row is a 4-byte store.
// w / 2 + 1 threads cover a row.  load(x) gives pixel x's (u, v).
template <typename Load>
__device__ __forceinline__ void store_flow_row_f16(uint16_t* __restrict__ row, int w, int t, float scale, Load load)
{
    const int par = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 1);
    const int x0 = 2 * t - par;
    if (x0 >= w) return;
    const bool has0 = x0 >= 0, has1 = x0 + 1 < w;
    uint32_t p0 = 0, p1 = 0;
    if (has0) { const float2 a = load(x0); p0 = scaled_half_bits(a.x, scale) | (scaled_half_bits(a.y, scale) << 16); }
    if (has1) { const float2 b = load(x0 + 1); p1 = scaled_half_bits(b.x, scale) | (scaled_half_bits(b.y, scale) << 16); }
    uint32_t* dst = reinterpret_cast<uint32_t*>(row) + x0;
    if (has0 && has1) *reinterpret_cast<uint2*>(dst) = make_uint2(p0, p1);
    else if (has0) dst[0] = p0;
    else if (has1) dst[1] = p1;
}
// grid of the output kernels for element type T: float32 one pixel per thread, float16 two
template <typename T> inline dim3 out_grid(const Geom& g, int z)
{
    const int tx = sizeof(T) == 2 ? g.w / 2 + 1 : g.w;
    return dim3((tx + 63) / 64, (g.h + 3) / 4, z);
}

// merge(u1,u2) -> interleaved [B][H][W][2], times the caller's unit scale (reference :600); T = float, or uint16_t for float16 bits
template <typename T>
__global__ __launch_bounds__(256) void k_output(StateBufs sb, const PairCtl* __restrict__ ctl, Geom g, float scale,
                                                T* __restrict__ out)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if constexpr (sizeof(T) == 4) {
        if (x >= g.w || y >= g.h) return;
        const int uc = ctl[b].ubase & 1;
        const size_t i = (size_t)b * g.splane + (size_t)y * g.pitch + x;
        float2 v = make_float2(sb.u1[uc][i] * scale, sb.u2[uc][i] * scale);
        reinterpret_cast<float2*>(out)[((size_t)b * g.h + y) * g.w + x] = v;
    } else {
        if (y >= g.h) return;
        const int uc = ctl[b].ubase & 1;
        const float* u1 = sb.u1[uc] + (size_t)b * g.splane + (size_t)y * g.pitch;
        const float* u2 = sb.u2[uc] + (size_t)b * g.splane + (size_t)y * g.pitch;
        store_flow_row_f16(out + ((size_t)b * g.h + y) * g.w * 2, g.w, x, scale, [&](int px) { return make_float2(u1[px], u2[px]); });
    }
}

// tf_dbg_f16_round: the output kernels' value function on caller-chosen values
__global__ __launch_bounds__(256) void k_dbg_f16_round(const float* __restrict__ in, size_t n, float scale, uint16_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (uint16_t)scaled_half_bits(in[i], scale);
}

// DualTVL1's stages (the median's skip test reads the stop rules of the iteration header), then the tail's conditioning
#include "teeflow_tvl1_warp.hip.h"
#include "teeflow_tvl1_iter.hip.h"
#include "teeflow_tvl1_median.hip.h"
#include "teeflow_cond.hip.h"
