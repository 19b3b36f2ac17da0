// teeflow_cond.hip.h -- frame conditioning and the float16 `echo` of the study tail (k_cond_minmax / k_cond_norm, also Otsu's
// input; k_echo_f16); included by teeflow_kernels.hip.h
#pragma once

// ---------------------------------------------------------------------------------------------
// Frame conditioning on the device: img2uint8(rgb2gray(frame)) of the reference
// (/root/reference/optical_flow/calculate_optical_flow.py:588, optical_flow_utils.py:30-31), per frame:
//   g = (R/255)*0.2125 + (G/255)*0.7154 + (B/255)*0.0721   (float64, skimage.color.rgb2gray)
//   u8 = rint(((g - min g) / max g) * 255)                  (the reference divides by max, NOT max - min)
// Pass 1 reduces per-frame min / max of g (non-negative doubles order like their bit patterns, so integer atomics do);
// pass 2 recomputes g and writes the byte.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double luma_f64(const uint8_t* p)
{
    return ((double)p[0] / 255.0) * 0.2125 + ((double)p[1] / 255.0) * 0.7154 + ((double)p[2] / 255.0) * 0.0721;
}

__global__ __launch_bounds__(256) void k_cond_minmax(const uint8_t* __restrict__ rgb, size_t npx, u64* __restrict__ mm /* [F][2] */)
{
    __shared__ u64 smin[4], smax[4];
    const int f = blockIdx.y;
    const uint8_t* src = rgb + (size_t)f * npx * 3;
    u64 lo = ~0ull, hi = 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const u64 b = (u64)__double_as_longlong(luma_f64(src + i * 3));
        lo = b < lo ? b : lo; hi = b > hi ? b : hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { lo = smin[w] < lo ? smin[w] : lo; hi = smax[w] > hi ? smax[w] : hi; }
        lo = smin[0] < lo ? smin[0] : lo; hi = smax[0] > hi ? smax[0] : hi;
        atomicMin(&mm[2 * f], lo);
        atomicMax(&mm[2 * f + 1], hi);
    }
}

__global__ __launch_bounds__(256) void k_cond_norm(const uint8_t* __restrict__ rgb, size_t npx, const u64* __restrict__ mm, uint8_t* __restrict__ out)
{
    const int f = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    const double mn = __longlong_as_double((long long)mm[2 * f]), mx = __longlong_as_double((long long)mm[2 * f + 1]);
    const double g = luma_f64(rgb + ((size_t)f * npx + i) * 3);
    double v = rint(((g - mn) / mx) * 255.0);
    v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);          // NaN (all-black frame: 0/0) falls through to 0 below
    out[(size_t)f * npx + i] = (uint8_t)(v == v ? (int)v : 0);
}

// ---- `echo` of the study file (reference :400-402): rgb2gray(frame).astype(np.float16), per pixel half(luma_f64(rgb)) ----------------
// float64 -> float16 in ONE rounding (nearest-even, subnormal halves kept, overflow to inf), with integer operations: a conversion
// through float32 rounds twice and differs from numpy's at 1057 of the 2^24 RGB triples.
__host__ __device__ inline uint16_t f64_to_f16_bits(double d)
{
    const u64 b = (u64)__builtin_bit_cast(unsigned long long, d);
    const uint32_t sign = (uint32_t)(b >> 48) & 0x8000u;
    const u64 a = b & 0x7fffffffffffffffull;
    const int e = (int)(a >> 52);                                       // biased by 1023
    if (e == 0x7ff) return (uint16_t)(sign | 0x7c00u | ((a & 0xfffffffffffffull) ? 0x200u : 0u));
    if (e > 1023 + 15) return (uint16_t)(sign | 0x7c00u);               // >= 2^16
    if (e < 1023 - 25) return (uint16_t)sign;                           // < 2^-25: below half of the smallest subnormal half
    const u64 m = (a & 0xfffffffffffffull) | (1ull << 52);              // 53-bit significand (e >= 998: a normal double)
    const bool normal = e >= 1023 - 14;
    const int shift = normal ? 42 : 1051 - e;                           // subnormal half: units of 2^-24, shift in [43, 53]
    const u64 r = m >> shift, rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    uint32_t hb = normal ? ((uint32_t)(e - 1008) << 10) + (uint32_t)(r & 0x3ff) : (uint32_t)r;
    if (rem > half || (rem == half && (r & 1))) ++hb;                   // a carry runs into the exponent, up to 0x7c00 = inf
    return (uint16_t)(sign | hb);
}

// n pixels of RGB (frames back to back) -> n halves; a thread takes 4 pixels: 12 bytes in, one 8-byte store
__global__ __launch_bounds__(256) void k_echo_f16(const uint8_t* __restrict__ rgb, size_t n, uint16_t* __restrict__ out)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n && (reinterpret_cast<uintptr_t>(out + i) & 7) == 0) {
        uint32_t hb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) hb[k] = f64_to_f16_bits(luma_f64(rgb + (i + k) * 3));
        *reinterpret_cast<uint2*>(out + i) = make_uint2(hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16));
    } else
        for (size_t k = i; k < n && k < i + 4; ++k) out[k] = f64_to_f16_bits(luma_f64(rgb + k * 3));
}
