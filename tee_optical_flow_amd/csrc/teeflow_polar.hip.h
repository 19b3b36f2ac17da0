// teeflow_polar.hip.h -- the polar steps of the consumer's per-pixel study analysis, on the device:
//   calculate_3dhist(ds, param, label) (the reference's optical_flow/analyze_optical_flow.py:909-966): cv2.cartToPolar of every
//     frame of ds.get_masked_arr(param, label), then per-frame histograms of the non-zero magnitudes and angles and the 99th
//     percentile of the non-zero magnitudes;
//   AngleDetector.detect (cardiac_cycle_detection.py:100-120): np.round(ang, 2) of the same angles, zeros dropped, and
//     scipy.stats.mode of each frame.
// One fused pass per frame block: OpticalFlowDataset's param field (param_px, shared with k_radlong_project_param), the polar
// transform as OpenCV 4.x computes it, the resident float64 planes that tf_radlong_hist / tf_radlong_select serve, the float32
// min/max and non-zero counts, and a per-frame histogram of the rounded angle.  A second small kernel picks each frame's mode.
#pragma once
#include "teeflow_analysis.hip.h"

// cv::cartToPolar for CV_32F in radians, restated from OpenCV 4.x's SIMD body (modules/core/src/mathfuncs_core.simd.hpp:
// magnitude32f, fastAtan32f / v_atan_f32), the path every element of a row of >= 16 takes on an AVX2 (FMA3) or NEON build.  The
// library builds with -ffp-contract=off, so the fused steps are written as __builtin_fmaf and nothing else fuses; division and
// sqrt are IEEE, denormals kept.  analysis.cart_to_polar is the same formula in numpy.  Parity with cv2 is unpinned.
#define PO_PI 3.1415926535897932384626433832795                      // CV_PI
#define PO_DEG (180.0 / PO_PI)
__device__ __forceinline__ float2 cart_to_polar(float x, float y)
{
    const float P1 = 0.9997878412794807f * (float)PO_DEG, P3 = -0.3258083974640975f * (float)PO_DEG;
    const float P5 = 0.1555786518463281f * (float)PO_DEG, P7 = -0.04432655554792128f * (float)PO_DEG;
    const float mag = sqrtf(__builtin_fmaf(x, x, y * y));             // v_muladd(x, x, y*y): y*y rounded first
    const float ax = fabsf(x), ay = fabsf(y);
    const float c = fminf(ax, ay) / (fmaxf(ax, ay) + (float)2.2204460492503131e-16);   // (float)DBL_EPSILON
    const float cc = c * c;
    float a = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(cc, P7, P5), cc, P3), cc, P1) * c;
    a = ax >= ay ? a : 90.f - a;
    a = x < 0.f ? 180.f - a : a;                                      // -0.0 is not < 0
    a = y < 0.f ? 360.f - a : a;
    return make_float2(mag, a * (float)(PO_PI / 180.0));
}

// np.round(ang, 2) is rint(ang * 100.f) / 100.f in float32; ang is in [0, 2*pi], so its integer k is in [0, 628].  k = 0 is what
// `flat != 0` drops; bins 1..628 are counted.
#define PO_NBINS 629

// mag / ang planes [n_used][H][W] as float64 (exact), optional float32 copies, min/max keys [4] (mag min, max, ang min, max, zeros
// included as np.min / np.max see them), non-zero counts [n_used][2], and the rounded-angle histogram [n_used][PO_NBINS]
template <int PARAM, typename FT, typename T>
__global__ __launch_bounds__(256) void k_polar_project_param(const FT* __restrict__ flow /* [>= n_used (+1)][H][W][2] */, int N,
                                                             const uint8_t* __restrict__ mask /* [n_used][H][W][C] */, int C, double h,
                                                             int H, int W, double* __restrict__ magp, double* __restrict__ angp,
                                                             float* __restrict__ mag32, float* __restrict__ ang32 /* both or neither */,
                                                             u64* __restrict__ mm, unsigned long long* __restrict__ cnt,
                                                             unsigned* __restrict__ bins)
{
    __shared__ unsigned sb[PO_NBINS];
    for (int b = threadIdx.x; b < PO_NBINS; b += 256) sb[b] = 0u;
    __syncthreads();
    const int n = blockIdx.y;
    const size_t npx = (size_t)H * W;
    u64 k[4] = {~0ull, 0ull, ~0ull, 0ull};
    unsigned c0 = 0, c1 = 0;
    const ParamFrame<T> pf = param_frame<T>(n, N, h);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const float2 f = param_px<PARAM, FT, T>(flow, mask, C, npx, n, pf, i);
        const float2 p = cart_to_polar(f.x, f.y);
        const size_t o = (size_t)n * npx + i;
        magp[o] = (double)p.x;
        angp[o] = (double)p.y;
        if (mag32) { mag32[o] = p.x; ang32[o] = p.y; }
        const u64 km = f64_key((double)p.x), ka = f64_key((double)p.y);
        k[0] = km < k[0] ? km : k[0]; k[1] = km > k[1] ? km : k[1];
        k[2] = ka < k[2] ? ka : k[2]; k[3] = ka > k[3] ? ka : k[3];
        c0 += p.x != 0.f; c1 += p.y != 0.f;
        const float r = rintf(p.y * 100.f);                            // round half to even, as np.round
        if (r >= 1.f && r <= (float)(PO_NBINS - 1)) atomicAdd(&sb[(int)r], 1u);   // (a NaN angle fails both tests)
    }
    radlong_reduce(k, c0, c1, n, mm, cnt);
    __syncthreads();
    for (int b = threadIdx.x; b < PO_NBINS; b += 256)
        if (sb[b]) atomicAdd(&bins[(size_t)n * PO_NBINS + b], sb[b]);
}

// scipy.stats.mode of frame n's rounded non-zero angles: the most frequent k, the smallest on a tie (scipy returns the smallest of
// the most frequent values, and k / 100.f grows with k); 0 for a frame without any
__global__ __launch_bounds__(256) void k_polar_mode(const unsigned* __restrict__ bins, int* __restrict__ mode_k /* [n_used] */)
{
    __shared__ u64 s[4];
    const int n = blockIdx.x;
    u64 best = 0;
    for (int b = 1 + threadIdx.x; b < PO_NBINS; b += 256) {
        const u64 key = ((u64)bins[(size_t)n * PO_NBINS + b] << 32) | (u64)(PO_NBINS - b);   // larger count, then smaller k
        best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = s[w] > best ? s[w] : best;
        mode_k[n] = (best >> 32) ? PO_NBINS - (int)(best & 0xFFFFFFFFull) : 0;
    }
}
