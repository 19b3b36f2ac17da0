// teeflow_overlay.hip.h -- the per-pixel part of the reference's visualize_radlong on the device
// (/root/reference/optical_flow/analyze_optical_flow.py:488-560, visualization.py:241-297, 1045-1051; host restatement
// tee_optical_flow_amd/analysis.py::radlong_overlay).  From the rad / long planes the projection left resident (float64 [n][H][W])
// and the echo frames (float16 or uint8 [n][H][W]):
//   half = max |rad[0]|                                  one CenteredNorm, frozen by its first call: frame 0 of the radial plane
//   t    = (a + half) / (2 * half), 0 if half == 0       float64, not clipped
//   idx  = clip(floor(t * 256), 0, 255)                  matplotlib's lookup with under = lut[0], over = lut[255]
//   m2   = the largest channel of the LUT entries either component used        (host, from the 2 x 256 flags of k_ov_index)
//   out  = uint8(((0.5 * (echo / echo max)) + (0.5 * (lut[idx][c] / m2))) * 255) truncating; [n][H][2W][3], radial left, long right
// The echo term is float16 arithmetic for a float16 echo, as numpy runs it: the quotient in float32 rounded to half, its half
// rounded to half again (both RNE, subnormals kept), then widened.  A uint8 echo divides in float64.
//   k_ov_half    max |v| over frame 0 of the radial plane, as the bits of a non-negative double (atomicMax)
//   k_ov_echo    max of the echo over the frames of a chunk + a flag for a negative or non-finite value
//   k_ov_index   both indices of a pixel into a 2-byte scratch; the entries used, as an LDS bitset OR-ed into global once per block
//   k_ov_compose the output seen as a flat array of 3-byte slots ([n * H] rows of 2W slots): a lane takes 4 consecutive slots = 12 bytes =
//                3 whole dwords at a dword-aligned offset, whatever W is, so a wave stores 768 contiguous bytes
// Everything is float64 in the reference's operation order (-ffp-contract=off); integer flags: atomic order cannot change a bit.
#pragma once
#include "teeflow_analysis.hip.h"

namespace ovl {

constexpr int ECHO_F16 = 0, ECHO_U8 = 1;

// the echo value as the double the reference's sum sees: 0.5 * (e / max)
template <int KIND> struct Echo;
template <> struct Echo<ECHO_F16> {
    using T = _Float16;
    static __device__ __forceinline__ double term(T e, double mx)
    {
        const _Float16 q = (_Float16)((float)e / (float)mx);         // mx holds a float16 value exactly
        return (double)(_Float16)((float)q * 0.5f);
    }
    static __device__ __forceinline__ bool bad(T e) { const float v = (float)e; return !(v >= 0.f) || v > 65504.f; }   // NaN, < 0, inf
    static __device__ __forceinline__ unsigned key(T e) { const float v = (float)e; return v > 0.f ? __float_as_uint(v) : 0u; }
};
template <> struct Echo<ECHO_U8> {
    using T = uint8_t;
    static __device__ __forceinline__ double term(T e, double mx) { return 0.5 * ((double)e / mx); }
    static __device__ __forceinline__ bool bad(T) { return false; }
    static __device__ __forceinline__ unsigned key(T e) { return __float_as_uint((float)e); }
};

// grid (<= 256): *half_bits = max over frame 0 of the bits of |v| (zeroed before; the planes are finite: the caller has checked)
__global__ __launch_bounds__(256) void k_ov_half(const double* __restrict__ rad, size_t npx, u64* __restrict__ half_bits)
{
    __shared__ u64 part[4];
    u64 m = 0ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const u64 b = (u64)__double_as_longlong(rad[i]) & 0x7FFFFFFFFFFFFFFFull;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_down(m, off, 64); m = o > m ? o : m; }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) m = part[w] > m ? part[w] : m;
    atomicMax(half_bits, m);
}

// grid (<= 1024): emax[0] = max over tot echo values of the float32 bits of the value (non-negative: ordered as unsigned),
// emax[1] |= 1 for a negative or non-finite value (both zeroed before)
template <int KIND>
__global__ __launch_bounds__(256) void k_ov_echo(const typename Echo<KIND>::T* __restrict__ echo, size_t tot, unsigned* __restrict__ emax)
{
    __shared__ unsigned part[4], pbad[4];
    unsigned m = 0u, bad = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (size_t)gridDim.x * 256) {
        const typename Echo<KIND>::T e = echo[i];
        if (Echo<KIND>::bad(e)) bad = 1u;
        else { const unsigned k = Echo<KIND>::key(e); m = k > m ? k : m; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned o = __shfl_down(m, off, 64); m = o > m ? o : m; bad |= __shfl_down(bad, off, 64); }
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = m; pbad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) { m = part[w] > m ? part[w] : m; bad |= pbad[w]; }
    atomicMax(emax, m);
    if (bad) atomicOr(emax + 1, 1u);
}

__device__ __forceinline__ unsigned lut_index(double a, double half, double two_half)
{
    if (half == 0.0) return 0u;                                      // Normalize: vmin == vmax gives 0 everywhere
    const double x = ((a + half) / two_half) * 256.0;
    return x < 0.0 ? 0u : (x >= 256.0 ? 255u : (unsigned)(int)x);  // under -> 0; == 256 -> 255; over -> 255; else truncation
}

// grid (<= 2048): idx[i] = radial index | long index << 8 for the tot pixels of all frames; used[0..8) / used[8..16) = the bitsets of
// the entries the radial / longitudinal plane used (zeroed before)
__global__ __launch_bounds__(256) void k_ov_index(const double* __restrict__ rad, const double* __restrict__ lon, size_t tot,
                                                  const u64* __restrict__ half_bits, uint16_t* __restrict__ idx, unsigned* __restrict__ used)
{
    __shared__ unsigned bits[16];
    if (threadIdx.x < 16) bits[threadIdx.x] = 0u;
    __syncthreads();
    const double half = __longlong_as_double((long long)*half_bits), two_half = half - (-half);   // vmax - vmin
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (size_t)gridDim.x * 256) {
        const unsigned ir = lut_index(rad[i], half, two_half), il = lut_index(lon[i], half, two_half);
        idx[i] = (uint16_t)(ir | (il << 8));
        // a set bit is never cleared: a stale read only costs a redundant atomic
        if (!((bits[ir >> 5] >> (ir & 31)) & 1u)) atomicOr(&bits[ir >> 5], 1u << (ir & 31));
        if (!((bits[8 + (il >> 5)] >> (il & 31)) & 1u)) atomicOr(&bits[8 + (il >> 5)], 1u << (il & 31));
    }
    __syncthreads();
    if (threadIdx.x < 16 && bits[threadIdx.x]) atomicOr(used + threadIdx.x, bits[threadIdx.x]);
}

// one block per 1024 slots.  rows = frames of the chunk * H; idx and echo point at the chunk's first frame; col[0] / col[1] =
// 0.5 * (lut / m2) of the radial / longitudinal colormap, [256][3]; out: the chunk's bytes rounded up to whole runs, ceil(slots / 4) * 3
// dwords: a lane that passes `s0 < slots` owns all three dwords of its run.
template <int KIND>
__global__ __launch_bounds__(256) void k_ov_compose(const uint16_t* __restrict__ idx, const typename Echo<KIND>::T* __restrict__ echo, double emax,
                                                    const double* __restrict__ col /* [2][256][3] */, size_t rows, int W,
                                                    unsigned* __restrict__ out)
{
    const size_t W2 = 2 * (size_t)W, slots = rows * W2;
    const size_t s0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= slots) return;
    size_t R = s0 / W2;
    unsigned o = (unsigned)(s0 - R * W2);
    uint8_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (s0 + k < slots) {
            const unsigned comp = o >= (unsigned)W ? 1u : 0u;
            const size_t p = R * (size_t)W + (o - comp * (unsigned)W);
            const unsigned j = (idx[p] >> (8 * comp)) & 255u;
            const double e = Echo<KIND>::term(echo[p], emax);
            const double* c = col + ((size_t)comp * 256 + j) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) b[3 * k + ch] = (uint8_t)(int)((e + c[ch]) * 255.0);   // in [0, 255]: truncation
        } else {
            b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = 0;              // (the last run's padding)
        }
        if (++o == (unsigned)W2) { o = 0; ++R; }
    }
    unsigned* dst = out + (s0 / 4) * 3;                                // byte 3 * s0 = dword 3 * (s0 / 4): s0 is a multiple of 4
#pragma unroll
    for (int d = 0; d < 3; ++d)
        dst[d] = (unsigned)b[4 * d] | ((unsigned)b[4 * d + 1] << 8) | ((unsigned)b[4 * d + 2] << 16) | ((unsigned)b[4 * d + 3] << 24);
}

}  // namespace ovl
