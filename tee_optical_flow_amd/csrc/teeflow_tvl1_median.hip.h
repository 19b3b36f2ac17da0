// teeflow_tvl1_median.hip.h -- DualTVL1's median stage (k_median<3|5>); included by teeflow_kernels.hip.h after the iteration
// header, whose stop rules decide which pairs a launch skips
#pragma once
#include "median_net.h"

// ---------------------------------------------------------------------------------------------
// cv::medianBlur(u, u, KS) on both flow planes, BORDER_REPLICATE, for pairs still iterating: with one iteration per launch
// (step 1) a pair that is active at `it`, with two (step 2) a pair in NORMAL mode at `it`.
// Tile 64x16 outputs per 256-thread block, staged through LDS with its halo; grid.z = 2*B.
// ---------------------------------------------------------------------------------------------
struct MedArgs {
    StateBufs sb;
    const PairCtl* ctl;
    const u64* err; int errstride; int it; double thr_q; int utog;
    int total, step;    // inner*outer; iterations per tvl1_iter launch (1 or 2)
    Geom g;
};

// Stage one 64 x 16 output tile of a plane with its halo (replicate border) in LDS.  Every load of a thread is issued
// before its first LDS write: one memory round trip per block instead of one per 256 staged values (the staging loop used
// to be ten dependent load -> wait -> write trips, several times the 1.5 k cycles the selection network takes).  Tiles
// whose 64 columns lie inside the image take float4 loads for the body and scalar loads for the 2R halo columns.
template <int KS>
__device__ __forceinline__ void median_stage(float (*t)[64 + 2 * (KS / 2)], const float* __restrict__ src, int x0, int y0, int W, int H, int pitch)
{
    constexpr int R = KS / 2, LW = 64 + 2 * R, LH = 16 + 2 * R;
    const int tid = threadIdx.x;
    if (x0 + 64 <= W) {
        constexpr int NV = (LH * 16 + 255) / 256;
        float4 v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = tid + 256 * k, ly = i >> 4, q = i & 15;
            if (i < LH * 16) v[k] = *reinterpret_cast<const float4*>(src + (size_t)clampi(y0 - R + ly, 0, H - 1) * pitch + x0 + 4 * q);
        }
        const bool halo = tid < LH * 2 * R;
        const int hly = tid / (2 * R), hc = tid % (2 * R), hlx = hc < R ? hc : 64 + hc;
        float hv = 0.f;
        if (halo) hv = src[(size_t)clampi(y0 - R + hly, 0, H - 1) * pitch + clampi(x0 - R + hlx, 0, W - 1)];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = tid + 256 * k, ly = i >> 4, q = i & 15;
            if (i < LH * 16) {
                float* d = &t[ly][R + 4 * q];
                if constexpr (R % 2 == 0) {            // 8-byte aligned: two ds_write_b64
                    *reinterpret_cast<float2*>(d) = make_float2(v[k].x, v[k].y);
                    *reinterpret_cast<float2*>(d + 2) = make_float2(v[k].z, v[k].w);
                } else { d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w; }
            }
        }
        if (halo) t[hly][hlx] = hv;
    } else {
        constexpr int NS = (LH * LW + 255) / 256;
        float sv[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int i = tid + 256 * k, ly = i / LW, lx = i % LW;
            if (i < LH * LW) sv[k] = src[(size_t)clampi(y0 - R + ly, 0, H - 1) * pitch + clampi(x0 - R + lx, 0, W - 1)];
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int i = tid + 256 * k;
            if (i < LH * LW) (&t[0][0])[i] = sv[k];
        }
    }
    __syncthreads();
}

// median of a staged (TH+2R) x (TW+2R) tile: 5x5 -> each thread produces FOUR horizontally adjacent outputs from one 5x8
// window (tf_median25_row4: shared column sorts and merges, 76 min/max/med3 per output instead of 198); 3x3 -> one
// output per thread and row as before.
template <int KS, int LW>
__device__ __forceinline__ void median_tile(const float (*t)[LW], float* __restrict__ dst, int x0, int y0, int W, int H, int pitch)
{
    if constexpr (KS == 5) {
        const int qx = threadIdx.x & 15, ly = threadIdx.x >> 4;        // 16 quads x 16 rows = the 64 x 16 tile
        const int x = x0 + 4 * qx, y = y0 + ly;
        if (x < W && y < H) {
            float col[8][5], out[4];
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const float4 lo = *reinterpret_cast<const float4*>(&t[ly + r][4 * qx]);
                const float4 hi = *reinterpret_cast<const float4*>(&t[ly + r][4 * qx + 4]);
                col[0][r] = lo.x; col[1][r] = lo.y; col[2][r] = lo.z; col[3][r] = lo.w;
                col[4][r] = hi.x; col[5][r] = hi.y; col[6][r] = hi.z; col[7][r] = hi.w;
            }
            tf_median25_row4(col, out);
            float* o = dst + (size_t)y * pitch + x;
            if (x + 3 < W) *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
            else
#pragma unroll
                for (int i = 0; i < 4; ++i) if (x + i < W) o[i] = out[i];
        }
    } else {
        const int lx = threadIdx.x & 63, x = x0 + lx;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ly = (threadIdx.x >> 6) + 4 * r, y = y0 + ly;
            if (x < W && y < H) {
                float p[KS * KS];
#pragma unroll
                for (int j = 0; j < KS; ++j)
#pragma unroll
                    for (int i = 0; i < KS; ++i) p[j * KS + i] = t[ly + j][lx + i];
                dst[(size_t)y * pitch + x] = tf_median9(p);
            }
        }
    }
}

template <int KS>
__global__ __launch_bounds__(256) void k_median(MedArgs a)
{
    constexpr int R = KS / 2, TWm = 64, THm = 16, LW = TWm + 2 * R, LH = THm + 2 * R;
    __shared__ __attribute__((aligned(16))) float t[LH][LW];
    const int b = blockIdx.z >> 1, plane = blockIdx.z & 1;
    const u64* e = a.err + (size_t)b * a.errstride;
    if (a.step == 2 ? pair_mode2(e, a.it, a.total, a.thr_q) != M_NORMAL : !pair_active(e, a.it, a.thr_q)) return;   // block-uniform
    const int uc = (a.ctl[b].ubase ^ a.utog) & 1;
    const size_t po = (size_t)b * a.g.splane;
    const float* __restrict__ src = (plane ? a.sb.u2[uc] : a.sb.u1[uc]) + po;
    float* __restrict__ dst = (plane ? a.sb.u2[uc ^ 1] : a.sb.u1[uc ^ 1]) + po;
    const int x0 = blockIdx.x * TWm, y0 = blockIdx.y * THm, W = a.g.w, H = a.g.h, pitch = a.g.pitch;
    median_stage<KS>(t, src, x0, y0, W, H, pitch);
    median_tile<KS, LW>(t, dst, x0, y0, W, H, pitch);
}
