// teeflow_otsu.hip.h -- predict_movie_thres of the reference on the device (/root/reference/optical_flow/calculate_optical_flow.py:184-213;
// host restatement tee_optical_flow_amd/masks.py).  For every uint8 RGB frame of a study:
//   g      = rgb2gray(frame)                      float64 luma, luma_f64 of teeflow_cond.hip.h (never stored: recomputed from the bytes)
//   thr    = skimage.filters.threshold_otsu(g)    256-bin np.histogram over [min g, max g], bin centres, first maximum of var12
//   m      = g > thr
//   clean  = remove_small_objects(binary_fill_holes(m), min_size)     the two labellings of clean_mask, the first set from LumaNotAbove
// and over the stack of cleaned planes, last, moving_avg_mask with its defaults; the store duplicates the channel (0x0101 per pixel).
//   k_cond_minmax   (teeflow_cond.hip.h)    per-frame min / max of g
//   k_otsu_hist     np.histogram's index rule, counts privatised in LDS per wave, one global atomic add per non-empty bin and block
//   k_otsu_thr      one block per frame: the four cumulative sums in np.cumsum's sequential order, var12, first argmax
//   k_otsu_keep     after the two labellings of a chunk of frames: one byte per pixel of the cleaned plane, kept for the whole study
//   k_otsu_window   the temporal window over the cleaned planes (it crosses chunk boundaries, so it runs last) and the store
// Counts and booleans only leave the atomics: their order cannot change a bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "teeflow_masks.hip.h"

namespace otsu {

constexpr int NBINS = 256;

// the first labelling's set (k_ccl_local): the background of m = g > thr[frame]; plane q of the chunk is frame f0 + q
struct LumaNotAbove {
    const uint8_t* __restrict__ rgb; const double* __restrict__ thr;
    int f0; size_t HW;
    __device__ __forceinline__ bool operator()(int q, size_t p) const
    {
        const size_t f = (size_t)(f0 + q);
        return !(luma_f64(rgb + (f * HW + p) * 3) > thr[f]);
    }
};

// edge i of np.linspace(mn, mx, NBINS + 1): i * step + mn, the last one set to mx
__device__ __forceinline__ double edge(int i, double mn, double mx, double step) { return i == NBINS ? mx : (double)i * step + mn; }

// np.histogram(a, bins=256, range=(mn, mx)) for mn < mx: the bin of a (mn <= a <= mx)
__device__ __forceinline__ int hist_bin(double a, double mn, double mx, double step)
{
    int i = (int)(((a - mn) / (mx - mn)) * (double)NBINS);      // astype(intp) truncates; the value is in [0, 256]
    i = i < 0 ? 0 : i;
    if (i >= NBINS) i = NBINS - 1;
    if (a < edge(i, mn, mx, step) && i > 0) --i;                // (a >= mn = edge 0: bin 0 never steps down)
    if (i != NBINS - 1 && a >= edge(i + 1, mn, mx, step)) ++i;
    return i;
}

// grid (blocks, frames), grid-stride over the frame's pixels.  hist: [frames][256], zeroed before.  A frame of one luma value (mn == mx)
// has no histogram: k_otsu_thr gives it that value.  Each wave counts into its own 256 words of LDS, and a thread adds a run of equal
// bins at once: a sector's zero background is one address for every lane, which would otherwise serialise the LDS atomics.
__global__ __launch_bounds__(256) void k_otsu_hist(const uint8_t* __restrict__ rgb, size_t npx, const u64* __restrict__ mm, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t cnt[4][NBINS];
    const int f = blockIdx.y;
    const double mn = __longlong_as_double((long long)mm[2 * f]), mx = __longlong_as_double((long long)mm[2 * f + 1]);
    if (!(mn < mx)) return;                                     // (uniform over the block)
#pragma unroll
    for (int w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0u;
    __syncthreads();
    const double step = (mx - mn) / (double)NBINS;
    const uint8_t* src = rgb + (size_t)f * npx * 3;
    uint32_t* mine = cnt[threadIdx.x >> 6];
    int run_bin = -1; uint32_t run = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const int b = hist_bin(luma_f64(src + i * 3), mn, mx, step);
        if (b == run_bin) { ++run; continue; }
        if (run) atomicAdd(mine + run_bin, run);
        run_bin = b; run = 1u;
    }
    if (run) atomicAdd(mine + run_bin, run);
    __syncthreads();
    const uint32_t c = cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
    if (c) atomicAdd(hist + (size_t)f * NBINS + threadIdx.x, c);
}

// grid (frames), 256 threads.  skimage 0.18.3 threshold_otsu on the histogram: thr[f] = centre of the first bin that maximises
//   var12[i] = w1[i] * w2[i+1] * (m1[i] - m2[i+1])^2,   i < 255
// with w1 / w2 the forward / backward cumulative counts and m1 / m2 the cumulative means, every sum in np.cumsum's sequential order.
// Bin 0 holds the minimum and bin 255 the maximum, so no w is zero.  A one-valued frame: thr = that value (skimage's early return).
__global__ __launch_bounds__(256) void k_otsu_thr(const u64* __restrict__ mm, const uint32_t* __restrict__ hist, double* __restrict__ thr)
{
    __shared__ double ctr[NBINS], hc[NBINS], w1[NBINS], w2[NBINS], m1[NBINS], m2[NBINS], var[NBINS];
    const int f = blockIdx.x, t = threadIdx.x;
    const double mn = __longlong_as_double((long long)mm[2 * f]), mx = __longlong_as_double((long long)mm[2 * f + 1]);
    if (!(mn < mx)) {
        if (t == 0) thr[f] = mn;
        return;
    }
    const double step = (mx - mn) / (double)NBINS;
    const double h = (double)hist[(size_t)f * NBINS + t];
    ctr[t] = (edge(t, mn, mx, step) + edge(t + 1, mn, mx, step)) / 2.0;
    hc[t] = h * ctr[t];
    w1[t] = h;                                                  // (the counts, until the scans below replace them)
    w2[t] = h;
    __syncthreads();
    if (t == 0) {                                               // forward sums: cumsum(hist), cumsum(hist * centres) / w1
        double w = 0.0, s = 0.0;
        for (int i = 0; i < NBINS; ++i) {
            w = i ? w + w1[i] : w1[i];
            s = i ? s + hc[i] : hc[i];
            w1[i] = w; m1[i] = s / w;
        }
    } else if (t == 64) {                                       // backward sums, on another wave
        double w = 0.0, s = 0.0;
        for (int i = NBINS - 1; i >= 0; --i) {
            w = i != NBINS - 1 ? w + w2[i] : w2[i];
            s = i != NBINS - 1 ? s + hc[i] : hc[i];
            w2[i] = w; m2[i] = s / w;
        }
    }
    __syncthreads();
    if (t < NBINS - 1) {
        const double d = m1[t] - m2[t + 1];
        var[t] = (w1[t] * w2[t + 1]) * (d * d);
    }
    __syncthreads();
    if (t == 0) {
        int best = 0;
        for (int i = 1; i < NBINS - 1; ++i)
            if (var[i] > var[best]) best = i;                   // np.argmax: the first of equal maxima
        thr[f] = ctr[best];
    }
}

// grid (ceil(H*W / 256), frames of the chunk): clean[f0 + fi][p] = 1 where p's component of the filled mask has at least min_size pixels
__global__ __launch_bounds__(256) void k_otsu_keep(const uint32_t* __restrict__ par, const uint32_t* __restrict__ aux, size_t HW, long long min_size,
                                                  uint8_t* __restrict__ clean /* at frame f0 */)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t q = blockIdx.y;
    const uint32_t r = par[q * HW + p];
    clean[q * HW + p] = r != msk::NONE && (long long)aux[q * HW + r] >= min_size;
}

// grid (ceil(H*W / 256), N): moving_avg_mask's defaults over the cleaned planes, both channels at once
__global__ __launch_bounds__(256) void k_otsu_window(const uint8_t* __restrict__ clean, int N, size_t HW, uint16_t* __restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int f = blockIdx.y;
    const int fa = f > 0 ? f - 1 : 0, fc = f + 1 < N ? f + 1 : N - 1, fd = f + 2 < N ? f + 2 : N - 1;
    const int count = clean[(size_t)fa * HW + p] + clean[(size_t)f * HW + p] + clean[(size_t)fc * HW + p] + clean[(size_t)fd * HW + p];
    out[(size_t)f * HW + p] = (double)count / 4.0 > 0.49 ? 0x0101 : 0;
}

}  // namespace otsu
