// teeflow_magoverlay.hip.h -- the per-pixel part of the reference's "single component" video on the device: the magnitude of
// get_masked_arr(param, label) through a colormap, blended half and half with the echo (the reference's example_peak_plots.py:459-513,
// optical_flow_dataset.py:57-58, 100-101, 189-228; host restatement tee_optical_flow_amd/analysis.py::magnitude_overlay_host).  From the
// flow (float16 or float32 [N][H][W][2]), the mask (uint8 [N][H][W][C]) and the echo (float16 or uint8 [n][H][W]), n <= N frames rendered:
//   mag   = sqrt(x*x + y*y) of the param field, float32: two rounded products, a rounded sum, a rounded root; nothing fused (this is
//           not cart_to_polar's sqrt(fma(x, x, y*y)))
//   vmin, vmax = min, max of mag over ALL N frames (zeros outside the mask included): one Normalize for the study
//   t     = (mag - vmin) / (vmax - vmin), float32; the divisor is the float64 difference (norm_f64: the quotient is formed in float64
//           and rounded to float32 once, numpy >= 2) or that difference rounded to float32 first (numpy 1.x); 0 if vmin == vmax
//   idx   = min(trunc(t * 256), 255)                                   the colormap's lookup for t in [0, 1]
//   per frame: emax = max echo, cmax = the largest channel of the table rows this frame used
//   v     = ((0.5 * (echo / emax)) + (0.5 * (lut[idx][c] / cmax))) * 255     float64; echo / emax is echo when emax == 0, lut / cmax is
//           lut when cmax == 0; the echo term is float16 arithmetic for a float16 echo (Echo<ECHO_F16>), float64 for uint8
//   out   = uint8 [n][H][W][3]: a float16 echo stores v into a float16 array first (rounded to half, nearest-even) and truncates
//           that; a uint8 echo truncates v itself
// Kernels:
//   k_mo_range    mag of every pixel of all N frames: min / max as the bits of non-negative floats (atomicMin / atomicMax on unsigned
//                 words: the order of the atomics cannot change a bit; a block whose extrema cannot move them skips them), and a flag
//                 for NaN or inf
//   k_mo_index    mag of frames [0, n) again, its index byte, and per frame the 256-bit set of rows used (an LDS bitset OR-ed out once
//                 per block)
//   k_mo_echo     per frame of a chunk: max of the echo as float32 bits + a flag for a negative or non-finite value
//   k_mo_scale    one block per frame: cmax from the frame's 256 flags and the table, then the frame's 256 x 3 colour terms
//                 0.5 * (lut / cmax), on the device so that the host need not wait between the index pass and the compose pass
//   k_mo_compose  the chunk's output seen as a flat array of 3-byte slots: a lane takes 4 consecutive slots = 12 bytes = 3 whole dwords
//                 at a dword-aligned offset, whatever W is (k_ov_compose's store shape); a slot's frame selects its emax and colour terms
// The index pass recomputes the magnitude from the flow rather than reading a stored float32 plane.  Per pixel and frame, float16 flow,
// C mask bytes: recomputing reads 4 B (velocity) or up to 12 B (acceleration, PWR: two neighbour frames, which the frames before and
// after have just read through the same L2) + C twice; a stored plane would add 4 B written over all N frames and 4 B read over n, and
// N * H * W * 4 B of scratch (68 MB for a 65-frame 512 x 512 study) against none.  The index itself is 1 B per pixel of the n frames.
// Everything is in the reference's operation order (-ffp-contract=off); flags and extrema are integers.
#pragma once
#include "teeflow_overlay.hip.h"

namespace mov {

// per frame: the rows used, the echo's maximum (float32 bits) and bad-value flag, the colour maximum
struct FrameMeta { unsigned used[8]; unsigned emax, ebad; double cmax; unsigned pad[4]; };
static_assert(sizeof(FrameMeta) == 64, "layout of the magnitude overlay's per-frame words");

// the study's words: min / max bits of the magnitude, its non-finite flag
struct Range { unsigned lo, hi, bad, pad; };

template <int PARAM, typename FT, typename T>
__device__ __forceinline__ float mag_px(const FT* __restrict__ flow, const uint8_t* __restrict__ mask, int C, size_t npx, int n,
                                        const ParamFrame<T>& pf, size_t i)
{
    const float2 f = param_px<PARAM, FT, T>(flow, mask, C, npx, n, pf, i);
    const float xx = f.x * f.x, yy = f.y * f.y;                       // np.sqrt(x**2 + y**2): each step rounded to float32
    return sqrtf(xx + yy);
}

// rounds a float64 in [0, 65504] to the nearest float16 value (ties to even, subnormals kept), returned as a float64: what a store
// into a float16 array does
__host__ __device__ inline double round_to_half(double v)
{
    union { double d; unsigned long long u; } c; c.d = v;
    int e = (int)((c.u >> 52) & 0x7FF) - 1023;                        // floor(log2 v) for a normal v; zero and subnormals: below -14
    if (e < -14) e = -14;                                             // float16's subnormal spacing, 2^-24
    c.u = (unsigned long long)(1023 + 10 - e) << 52;                  // 2^(10 - e)
    const double up = c.d;
    c.u = (unsigned long long)(1023 - 10 + e) << 52;                  // 2^(e - 10): the spacing of float16 values at v
    return __builtin_rint(v * up) * c.d;                              // both products are exact: scalings by powers of two
}

// grid (<= 256, N): rng->lo / hi = min / max of the bits of mag over all N frames (seeded ~0 / 0), rng->bad |= 1 for NaN or inf
template <int PARAM, typename FT, typename T>
__global__ __launch_bounds__(256) void k_mo_range(const FT* __restrict__ flow /* [N][H][W][2] */, int N,
                                                  const uint8_t* __restrict__ mask /* [N][H][W][C] */, int C, double h, size_t npx,
                                                  Range* __restrict__ rng)
{
    __shared__ unsigned plo[4], phi[4], pbad[4];
    const int n = blockIdx.y;
    const ParamFrame<T> pf = param_frame<T>(n, N, h);
    unsigned lo = ~0u, hi = 0u, bad = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const unsigned b = __float_as_uint(mag_px<PARAM, FT, T>(flow, mask, C, npx, n, pf, i));
        if (b >= 0x7F800000u) bad = 1u;                               // inf, NaN of either sign (a finite mag is >= +0)
        else { lo = b < lo ? b : lo; hi = b > hi ? b : hi; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned ol = __shfl_down(lo, off, 64), oh = __shfl_down(hi, off, 64);
        lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi; bad |= __shfl_down(bad, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { plo[threadIdx.x >> 6] = lo; phi[threadIdx.x >> 6] = hi; pbad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) { lo = plo[w] < lo ? plo[w] : lo; hi = phi[w] > hi ? phi[w] : hi; bad |= pbad[w]; }
    // Every block of every frame meets at these three words, and atomics on one address go through L2 one at a time (measured: 16640
    // blocks, 380 us whatever the frame size, ten times the kernel's loads).  The extrema only ever move outwards, so a block that
    // cannot move them says nothing; it learns that from a load that is coherent across the device, where a stale value only costs a
    // redundant atomic.
    if (lo < __hip_atomic_load(&rng->lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&rng->lo, lo);
    if (hi > __hip_atomic_load(&rng->hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&rng->hi, hi);
    if (bad) atomicOr(&rng->bad, 1u);
}

// grid (<= 128, n): idx[n][i] = the table row of pixel i of frame n; fm[n].used = the bitset of the rows frame n used (zeroed before)
template <int PARAM, typename FT, typename T>
__global__ __launch_bounds__(256) void k_mo_index(const FT* __restrict__ flow, int N, const uint8_t* __restrict__ mask, int C, double h,
                                                  size_t npx, const Range* __restrict__ rng, int norm_f64, uint8_t* __restrict__ idx,
                                                  FrameMeta* __restrict__ fm)
{
    __shared__ unsigned bits[8];
    if (threadIdx.x < 8) bits[threadIdx.x] = 0u;
    __syncthreads();
    const int n = blockIdx.y;
    const ParamFrame<T> pf = param_frame<T>(n, N, h);
    const float vmin = __uint_as_float(rng->lo), vmax = __uint_as_float(rng->hi);
    const double d64 = (double)vmax - (double)vmin;                   // vmin and vmax reach the norm as float64 scalars
    const float d32 = (float)d64;
    const bool flat = !(vmin < vmax);                                 // Normalize: vmin == vmax gives 0 everywhere
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const float s = mag_px<PARAM, FT, T>(flow, mask, C, npx, n, pf, i) - vmin;
        const float t = flat ? 0.f : (norm_f64 ? (float)((double)s / d64) : s / d32);
        const float x = t * 256.f;
        const unsigned j = x >= 256.f ? 255u : (x > 0.f ? (unsigned)(int)x : 0u);   // == 256 -> 255, else truncation (NaN -> 0: refused later)
        idx[(size_t)n * npx + i] = (uint8_t)j;
        // a set bit is never cleared: a stale read only costs a redundant atomic
        if (!((bits[j >> 5] >> (j & 31)) & 1u)) atomicOr(&bits[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    if (threadIdx.x < 8 && bits[threadIdx.x]) atomicOr(&fm[n].used[threadIdx.x], bits[threadIdx.x]);
}

// grid (<= 64, frames of the chunk): fm[f].emax = max over frame f of the float32 bits of the echo (non-negative: ordered as unsigned),
// fm[f].ebad |= 1 for a negative or non-finite value (both zeroed before); echo and fm point at the chunk's first frame
template <int KIND>
__global__ __launch_bounds__(256) void k_mo_echo(const typename ovl::Echo<KIND>::T* __restrict__ echo, size_t npx, FrameMeta* __restrict__ fm)
{
    using E = ovl::Echo<KIND>;
    __shared__ unsigned part[4], pbad[4];
    const int f = blockIdx.y;
    unsigned m = 0u, bad = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const typename E::T e = echo[(size_t)f * npx + i];
        if (E::bad(e)) bad = 1u;
        else { const unsigned k = E::key(e); m = k > m ? k : m; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned o = __shfl_down(m, off, 64); m = o > m ? o : m; bad |= __shfl_down(bad, off, 64); }
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = m; pbad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) { m = part[w] > m ? part[w] : m; bad |= pbad[w]; }
    atomicMax(&fm[f].emax, m);
    if (bad) atomicOr(&fm[f].ebad, 1u);
}

// grid (n), 256 threads, thread j = table row j: fm[f].cmax = the largest channel of the rows frame f used; col[f][j][c] =
// 0.5 * (lut[j][c] / cmax), or 0.5 * lut[j][c] when cmax == 0.  The table's entries are finite and >= 0 (the caller has checked), so
// their bits order as unsigned integers and the maximum is exact in any order.
__global__ __launch_bounds__(256) void k_mo_scale(const double* __restrict__ lut /* [256][3] */, FrameMeta* __restrict__ fm,
                                                  double* __restrict__ col /* [n][256][3] */)
{
    __shared__ u64 part[4];
    const int f = blockIdx.x, j = threadIdx.x;
    const double c0 = lut[3 * j], c1 = lut[3 * j + 1], c2 = lut[3 * j + 2];
    u64 m = 0ull;
    if ((fm[f].used[j >> 5] >> (j & 31)) & 1u) {
        const double v = c0 > c1 ? (c0 > c2 ? c0 : c2) : (c1 > c2 ? c1 : c2);
        m = (u64)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull;     // (-0.0 counts as 0)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_down(m, off, 64); m = o > m ? o : m; }
    if ((j & 63) == 0) part[j >> 6] = m;
    __syncthreads();
    m = part[0];
    for (int w = 1; w < 4; ++w) m = part[w] > m ? part[w] : m;
    const double cmax = __longlong_as_double((long long)m);
    if (j == 0) fm[f].cmax = cmax;
    double* c = col + ((size_t)f * 256 + j) * 3;
    c[0] = 0.5 * (cmax > 0.0 ? c0 / cmax : c0);
    c[1] = 0.5 * (cmax > 0.0 ? c1 / cmax : c1);
    c[2] = 0.5 * (cmax > 0.0 ? c2 / cmax : c2);
}

// one block per 1024 slots of the chunk.  idx, echo, fm and col point at the chunk's first frame; slots = frames of the chunk * npx;
// out: the chunk's bytes rounded up to whole runs, ceil(slots / 4) * 3 dwords: a lane that passes `s0 < slots` owns all three dwords
// of its run.
template <int KIND>
__global__ __launch_bounds__(256) void k_mo_compose(const uint8_t* __restrict__ idx, const typename ovl::Echo<KIND>::T* __restrict__ echo,
                                                    const FrameMeta* __restrict__ fm, const double* __restrict__ col /* [frames][256][3] */,
                                                    size_t npx, size_t slots, unsigned* __restrict__ out)
{
    using E = ovl::Echo<KIND>;
    const size_t s0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= slots) return;
    size_t f = s0 / npx, o = s0 - f * npx;
    double emax = (double)__uint_as_float(fm[f].emax);
    uint8_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (s0 + k < slots) {
            const size_t p = s0 + k;
            const double e = emax > 0.0 ? E::term(echo[p], emax) : 0.0;   // an all-zero frame: e / max is e itself, 0
            const double* c = col + (f * 256 + idx[p]) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double v = (e + c[ch]) * 255.0;                      // in [0, 255]
                b[3 * k + ch] = (uint8_t)(int)(KIND == ovl::ECHO_F16 ? round_to_half(v) : v);   // truncation
            }
        } else {
            b[3 * k] = b[3 * k + 1] = b[3 * k + 2] = 0;                  // (the last run's padding)
        }
        if (++o == npx && s0 + k + 1 < slots) { o = 0; ++f; emax = (double)__uint_as_float(fm[f].emax); }
    }
    unsigned* dst = out + (s0 / 4) * 3;                                    // byte 3 * s0 = dword 3 * (s0 / 4): s0 is a multiple of 4
#pragma unroll
    for (int d = 0; d < 3; ++d)
        dst[d] = (unsigned)b[4 * d] | ((unsigned)b[4 * d + 1] << 8) | ((unsigned)b[4 * d + 2] << 16) | ((unsigned)b[4 * d + 3] << 24);
}

}  // namespace mov
