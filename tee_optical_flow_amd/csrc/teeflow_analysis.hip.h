// teeflow_analysis.hip.h -- SURVEY.md row f1: radial / longitudinal projection of the flow and the per-frame statistics
// the reference derives from it (/root/reference/optical_flow/analysis.py:89-212: radial_vecgrid, calc_proj_mag,
// calculate_comp_magnitude, calc_bidirectional_hist).  The reference builds [N,H,W,2] float64 unit-vector grids in Python
// loops and calls np.percentile / np.histogram per frame; here the projection is one pass over the flow, the histogram a
// second, and the percentiles' order statistics an exact 4-pass radix select -- all in float64 with the reference's
// operation order (bit-identical to tests/golden/reference_analysis.npz, which the reference's own code produced).
#pragma once
#include "teeflow_kernels.hip.h"

// order-preserving map double -> u64 (total order of finite values; -0.0 < +0.0 is irrelevant: zeros are excluded)
__device__ __forceinline__ u64 f64_key(double v)
{
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double f64_unkey(u64 k)
{
    const u64 b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    union { u64 u; double d; } c; c.u = b;
    return c.d;
}

// one pixel of the projection: rad/long of the float32 field (fx, fy) at pixel i of frame n around the centroid (cH, cW), folded into
// the thread's min/max keys and non-zero counts
__device__ __forceinline__ void radlong_px(float fx, float fy, double cH, double cW, int W, int n, size_t npx, size_t i, double* __restrict__ rad,
                                           double* __restrict__ lon, u64 (&k)[4], unsigned& c0, unsigned& c1)
{
    const int hh = (int)(i / W), ww = (int)(i - (size_t)hh * W);
    const double dh = cH - (double)hh, dw = cW - (double)ww;
    const double nrm = sqrt(dh * dh + dw * dw);
    double u0 = dh / nrm, u1 = dw / nrm;
    u0 = u0 == u0 ? u0 : 0.0; u1 = u1 == u1 ? u1 : 0.0;         // nan_to_num(nan=0): the centroid pixel itself
    const double r = (double)fx * u0 + (double)fy * u1;           // sum(OF * unitvec): note OF[...,0] (x) meets the ROW component
    const double l = (double)fx * u1 + (double)fy * (-1.0 * u0);
    rad[(size_t)n * npx + i] = r;
    lon[(size_t)n * npx + i] = l;
    const u64 kr = f64_key(r), kl = f64_key(l);
    k[0] = kr < k[0] ? kr : k[0]; k[1] = kr > k[1] ? kr : k[1];
    k[2] = kl < k[2] ? kl : k[2]; k[3] = kl > k[3] ? kl : k[3];
    c0 += r != 0.0; c1 += l != 0.0;
}

// the block's min/max keys and non-zero counts into the global ones (256 threads)
__device__ __forceinline__ void radlong_reduce(u64 (&k)[4], unsigned c0, unsigned c1, int n, u64* __restrict__ mm, unsigned long long* __restrict__ cnt)
{
    __shared__ u64 s[4][4];
    __shared__ unsigned sc[4][2];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u64 o = __shfl_down(k[j], off, 64);
            k[j] = (j & 1) ? (o > k[j] ? o : k[j]) : (o < k[j] ? o : k[j]);
        }
        c0 += __shfl_down(c0, off, 64); c1 += __shfl_down(c1, off, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { for (int j = 0; j < 4; ++j) s[wv][j] = k[j]; sc[wv][0] = c0; sc[wv][1] = c1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w2 = 1; w2 < 4; ++w2) {
            for (int j = 0; j < 4; ++j) k[j] = (j & 1) ? (s[w2][j] > k[j] ? s[w2][j] : k[j]) : (s[w2][j] < k[j] ? s[w2][j] : k[j]);
            c0 += sc[w2][0]; c1 += sc[w2][1];
        }
        atomicMin(&mm[0], k[0]); atomicMax(&mm[1], k[1]); atomicMin(&mm[2], k[2]); atomicMax(&mm[3], k[3]);
        atomicAdd(&cnt[2 * n], (unsigned long long)c0); atomicAdd(&cnt[2 * n + 1], (unsigned long long)c1);
    }
}

// rad/long planes [N][H][W] (f64), global min/max keys of both, per-frame non-zero counts
__global__ __launch_bounds__(256) void k_radlong_project(const float* __restrict__ flow, const double* __restrict__ cent, int H, int W,
                                                         double* __restrict__ rad, double* __restrict__ lon, u64* __restrict__ mm /* [4]: rad min,max, long min,max */,
                                                         unsigned long long* __restrict__ cnt /* [N][2] */)
{
    const int n = blockIdx.y;
    const size_t npx = (size_t)H * W;
    const double cH = cent[2 * n], cW = cent[2 * n + 1];
    u64 k[4] = {~0ull, 0ull, ~0ull, 0ull};
    unsigned c0 = 0, c1 = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const float2 f = reinterpret_cast<const float2*>(flow)[(size_t)n * npx + i];
        radlong_px(f.x, f.y, cH, cW, W, n, npx, i, rad, lon, k, c0, c1);
    }
    radlong_reduce(k, c0, c1, n, mm, cnt);
}

// The parameter field of OpticalFlowDataset (/root/reference/optical_flow/optical_flow_dataset.py:57, 100-101, 182-228) fused into the
// projection: vel = flow.astype(float32); accel = np.gradient(vel, h, axis=0); pwr = vel * accel; field = param * mask.
// np.gradient's output has vel's dtype (float32); T is the type its division runs in (numpy's promotion of float32 by the caller's
// spacing h: float, or double for a np.float64 h under NEP 50): interior (v[n+1] - v[n-1]) / (2.0 * h), frames 0 and N-1 the one-sided
// difference / h (edge_order 1), each difference in float32 and each quotient rounded to float32.  pwr and the mask product are float32
// (a bool mask multiplies by 0 or 1).  Frames [0, n_used) are projected; the gradient sees all N.
enum { RL_PARAM_VELOCITY = 0, RL_PARAM_ACCELERATION = 1, RL_PARAM_PWR = 2 };

template <typename FT>
__device__ __forceinline__ float2 rl_ld(const FT* __restrict__ f, size_t j) { return make_float2((float)f[2 * j], (float)f[2 * j + 1]); }

// frame n's gradient neighbours lo / hi and divisor den (np.gradient, edge_order 1)
template <typename T>
struct ParamFrame { int lo, hi; T den; };

template <typename T>
__device__ __forceinline__ ParamFrame<T> param_frame(int n, int N, double h)
{
    const bool edge = n == 0 || n == N - 1;
    const int lo = edge ? (n == 0 ? 0 : N - 2) : n - 1;
    return {lo, edge ? lo + 1 : n + 1, edge ? (T)h : (T)(2.0 * h)};
}

// the param field times the mask at pixel i of frame n (float32, as numpy keeps it); shared by every kernel that reads the field
template <int PARAM, typename FT, typename T>
__device__ __forceinline__ float2 param_px(const FT* __restrict__ flow, const uint8_t* __restrict__ mask, int C, size_t npx, int n,
                                           const ParamFrame<T>& pf, size_t i)
{
    const float2 v = rl_ld(flow, (size_t)n * npx + i);
    float fx = v.x, fy = v.y;
    if (PARAM != RL_PARAM_VELOCITY) {
        const float2 a = rl_ld(flow, (size_t)pf.lo * npx + i), b = rl_ld(flow, (size_t)pf.hi * npx + i);
        const float gx = (float)((T)(b.x - a.x) / pf.den), gy = (float)((T)(b.y - a.y) / pf.den);
        fx = PARAM == RL_PARAM_PWR ? v.x * gx : gx;
        fy = PARAM == RL_PARAM_PWR ? v.y * gy : gy;
    }
    const uint8_t* mp = mask + ((size_t)n * npx + i) * C;
    fx = fx * (float)mp[0];
    fy = fy * (float)mp[C - 1];                                    // C == 1: channel 0 for both components (numpy broadcasting)
    return make_float2(fx, fy);
}

template <int PARAM, typename FT, typename T>
__global__ __launch_bounds__(256) void k_radlong_project_param(const FT* __restrict__ flow /* [>= n_used (+1)][H][W][2] */, int N,
                                                               const uint8_t* __restrict__ mask /* [n_used][H][W][C] */, int C, double h,
                                                               const double* __restrict__ cent, int H, int W, double* __restrict__ rad,
                                                               double* __restrict__ lon, u64* __restrict__ mm, unsigned long long* __restrict__ cnt)
{
    const int n = blockIdx.y;
    const size_t npx = (size_t)H * W;
    const double cH = cent[2 * n], cW = cent[2 * n + 1];
    u64 k[4] = {~0ull, 0ull, ~0ull, 0ull};
    unsigned c0 = 0, c1 = 0;
    const ParamFrame<T> pf = param_frame<T>(n, N, h);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const float2 f = param_px<PARAM, FT, T>(flow, mask, C, npx, n, pf, i);
        radlong_px(f.x, f.y, cH, cW, W, n, npx, i, rad, lon, k, c0, c1);
    }
    radlong_reduce(k, c0, c1, n, mm, cnt);
}

// np.histogram(frame[frame != 0], bins=nbins, range=(first, last)) per frame: estimate, then numpy's edge fix-ups
__global__ __launch_bounds__(256) void k_radlong_hist(const double* __restrict__ v, size_t npx, const double* __restrict__ edges, int nbins,
                                                      unsigned long long* __restrict__ freq /* [N][nbins] */)
{
    const int n = blockIdx.y;
    const double first = edges[0], last = edges[nbins];
    const double denom = last - first;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const double x = v[(size_t)n * npx + i];
        if (x == 0.0 || !(x >= first && x <= last)) continue;
        int idx = (int)(((x - first) / denom) * (double)nbins);
        if (idx >= nbins) idx = nbins - 1;
        if (idx < 0) idx = 0;
        if (x < edges[idx]) --idx;
        else if (idx != nbins - 1 && x >= edges[idx + 1]) ++idx;
        atomicAdd(&freq[(size_t)n * nbins + idx], 1ull);
    }
}

// one 16-bit digit pass of the radix select: histogram of the digit among the non-zero values whose higher digits equal the
// slot's prefix (up to NSLOT order statistics per frame are selected at once)
#define RL_NSLOT 4
__global__ __launch_bounds__(256) void k_radlong_sel_hist(const double* __restrict__ v, size_t npx, int shift, const u64* __restrict__ prefix /* [N][NSLOT] */,
                                                          const int* __restrict__ active /* [N][NSLOT] */, unsigned* __restrict__ hist /* [N][NSLOT][65536] */)
{
    const int n = blockIdx.y;
    u64 pf[RL_NSLOT]; int ac[RL_NSLOT];
#pragma unroll
    for (int j = 0; j < RL_NSLOT; ++j) { pf[j] = prefix[n * RL_NSLOT + j]; ac[j] = active[n * RL_NSLOT + j]; }
    const u64 himask = shift == 48 ? 0ull : (~0ull << (shift + 16));
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const double x = v[(size_t)n * npx + i];
        if (x == 0.0) continue;
        const u64 key = f64_key(x);
        const unsigned digit = (unsigned)((key >> shift) & 0xFFFFull);
#pragma unroll
        for (int j = 0; j < RL_NSLOT; ++j)
            if (ac[j] && (key & himask) == (pf[j] & himask)) atomicAdd(&hist[((size_t)n * RL_NSLOT + j) * 65536 + digit], 1u);
    }
}

// find the digit bucket that contains the slot's remaining rank; extend the prefix, reduce the rank
__global__ __launch_bounds__(256) void k_radlong_sel_scan(const unsigned* __restrict__ hist, int shift, u64* __restrict__ prefix, long long* __restrict__ rank,
                                                          const int* __restrict__ active)
{
    __shared__ unsigned long long part[256];
    const int slot = blockIdx.x;                       // n * NSLOT + j
    if (!active[slot]) return;
    const unsigned* hrow = hist + (size_t)slot * 65536;
    unsigned long long loc = 0;
    for (int b = 0; b < 256; ++b) loc += hrow[threadIdx.x * 256 + b];
    part[threadIdx.x] = loc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long r = rank[slot];
        int t = 0;
        while (t < 255 && (long long)part[t] <= r) { r -= (long long)part[t]; ++t; }
        int b = 0;
        while (b < 255 && (long long)hrow[t * 256 + b] <= r) { r -= (long long)hrow[t * 256 + b]; ++b; }
        const u64 digit = (u64)(t * 256 + b);
        prefix[slot] |= digit << shift;
        rank[slot] = r;
    }
}
