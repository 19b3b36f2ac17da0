// teeflow_tvl1_warp.hip.h -- DualTVL1's flow upsample, the initial flow's way down the pyramid, and the warp stage (k_flow_up; k_init_split,
// k_init_down, k_chain_seed, k_chain_gather; k_warp, k_warp_lds; k_grad and k_warp_cuda for TF_VARIANT_CUDA); included by teeflow_kernels.hip.h, which holds the types, helpers and arithmetic contract
#pragma once

// flow: coarse level -> next finer level, times 1/scaleStep (resize + multiply of DualTVL1::calc)
__global__ __launch_bounds__(256) void k_flow_up(StateBufs sb, const PairCtl* __restrict__ ctl, Geom gs, Geom gd,
                                                 double scale_x, double scale_y, float mul, int cuda_sampling = 0)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (dx >= gd.w || dy >= gd.h) return;
    const int uc = ctl[b].ubase & 1;
    const size_t di = (size_t)b * gd.splane + (size_t)dy * gd.pitch + dx;
    if (cuda_sampling) {
        sb.u1[uc ^ 1][di] = resize_px_cuda(sb.u1[uc] + (size_t)b * gs.splane, gs.w, gs.h, gs.pitch, dx, dy, (float)scale_x, (float)scale_y) * mul;
        sb.u2[uc ^ 1][di] = resize_px_cuda(sb.u2[uc] + (size_t)b * gs.splane, gs.w, gs.h, gs.pitch, dx, dy, (float)scale_x, (float)scale_y) * mul;
        return;
    }
    sb.u1[uc ^ 1][di] = resize_px(sb.u1[uc] + (size_t)b * gs.splane, gs.w, gs.h, gs.pitch, dx, dy, scale_x, scale_y) * mul;
    sb.u2[uc ^ 1][di] = resize_px(sb.u2[uc] + (size_t)b * gs.splane, gs.w, gs.h, gs.pitch, dx, dy, scale_x, scale_y) * mul;
}

// ---- useInitialFlow: the caller's flow down the pyramid to the coarsest level, where the solve starts from it ---------------------
// split(flow, u1s[0], u2s[0]): interleaved [B][H][W][2] (any 4-byte alignment) -> level-0 planes of u buffer `k`
__global__ __launch_bounds__(256) void k_init_split(const float* __restrict__ init, StateBufs sb, int k, Geom g)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= g.w || y >= g.h) return;
    const size_t si = (((size_t)b * g.h + y) * g.w + x) * 2;
    const size_t di = (size_t)b * g.splane + (size_t)y * g.pitch + x;
    sb.u1[k][di] = init[si];
    sb.u2[k][di] = init[si + 1];
}

// k_flow_up's mirror: level s-1 (u buffer `k`) -> level s (the other buffer) by the pyramid's rule, resize(src, Size(), scaleStep,
// scaleStep) = resize_px with scale 1/scaleStep, times (float)scaleStep.  Reads and writes x < w only.
__global__ __launch_bounds__(256) void k_init_down(StateBufs sb, int k, Geom gs, Geom gd, double scale, float mul)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (dx >= gd.w || dy >= gd.h) return;
    const size_t di = (size_t)b * gd.splane + (size_t)dy * gd.pitch + dx;
    sb.u1[k ^ 1][di] = resize_px(sb.u1[k] + (size_t)b * gs.splane, gs.w, gs.h, gs.pitch, dx, dy, scale, scale) * mul;
    sb.u2[k ^ 1][di] = resize_px(sb.u2[k] + (size_t)b * gs.splane, gs.w, gs.h, gs.pitch, dx, dy, scale, scale) * mul;
}

// A chained sequence: the finished level-0 flow of the pair solved last in state slot b (u buffer ctl[b].ubase -- which one depends on
// the iterations that pair executed, so only the device knows, and it differs from slot to slot) becomes the initial flow of the slot's
// next pair, level 0 of the chain above, which k_init_down expects in u buffer `k`: kept where it is, or moved, each slot in its own
// plane.  `pad` (a one-level solve, where this level is the one the first stage reads and the host's memsets, which would clear it, are
// left out): the row padding x in [w, pitch) of buffer `k` is cleared, as those memsets leave it.  Reads ctl[b] and never writes it:
// k_ctl_set follows.  One thread per (x < pitch, y < h) and slot blockIdx.z: one slot for a single chain, the step's active slots
// [0, B) for chains in lock-step; slots beyond the grid are not touched.
__global__ __launch_bounds__(256) void k_chain_seed(StateBufs sb, const PairCtl* __restrict__ ctl, int k, Geom g, int pad)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= g.pitch || y >= g.h) return;
    const size_t i = (size_t)b * g.splane + (size_t)y * g.pitch + x;
    if (x >= g.w) {
        if (pad) { sb.u1[k][i] = 0.f; sb.u2[k][i] = 0.f; }
        return;
    }
    const int uc = ctl[b].ubase & 1;
    if (uc == k) return;
    sb.u1[k][i] = sb.u1[uc][i];
    sb.u2[k][i] = sb.u2[uc][i];
}

// Chains in lock-step: level 0 of the pyramid, time-major.  Frame slot f = t * S + s holds frame t of chain s, so that a step's pairs
// are consecutive slots (WarpArgs' off0 + b, off1 + b).  src[f] is that frame, dense [H][W] in device memory -- uint8
// (k_u8_to_f32's conversion), or float32 in [0,1] when f32 (k_f32_to_level0's, times 255) -- or null where chain s has no frame t:
// that slot is cleared, so that the pyramid kernels, which sweep every slot, read finite values there.
__global__ __launch_bounds__(256) void k_chain_gather(const void* const* __restrict__ src, int f32, float* __restrict__ dst, Geom g)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= g.w) return;
    const void* p = src[f];
    const size_t si = (size_t)y * g.w + x;
    float v = 0.f;
    if (p) v = f32 ? static_cast<const float*>(p)[si] * 255.0f : (float)static_cast<const uint8_t*>(p)[si];
    dst[(size_t)f * g.plane + (size_t)y * g.pitch + x] = v;
}

// ---------------------------------------------------------------------------------------------
// Warp stage (tvl1flow.cpp: buildFlowMap + 3x cv::remap INTER_CUBIC/BORDER_CONSTANT + calcGradRho).
// The centred gradient of I1 is evaluated on the fly from a clamped 6x6 patch (bit-identical to
// gradient-then-remap: each tap's gradient is the same 0.5f*(next-prev) of the same two pixels),
// so I1x/I1y never exist in HBM.  Output: I1wx, I1wy, rho_c.
// ---------------------------------------------------------------------------------------------
struct WarpArgs {
    const float* pyr;       // this level's frame planes
    int off0, off1;         // pair b uses frames off0+b (I0) and off1+b (I1)
    StateBufs sb;
    const PairCtl* ctl;
    const float* tab;       // [32][4] bicubic coefficients (A = -0.75)
    float *wx, *wy, *rho;
    Geom g;
};

// one output pixel of the warp stage; every pointer is already offset to the pair's plane (I0 / I1: to its frames)
__device__ __forceinline__ void warp_px(const float* stab, const float* __restrict__ I0, const float* __restrict__ I1,
                                        const float* __restrict__ gu1, const float* __restrict__ gu2,
                                        float* __restrict__ owx, float* __restrict__ owy, float* __restrict__ orho,
                                        int W, int H, int pitch, int x, int y)
{
    const size_t idx = (size_t)y * pitch + x;
    const float u1 = gu1[idx], u2 = gu2[idx];
    const float mx = (float)x + u1, my = (float)y + u2;
    const int sx = __float2int_rn(mx * 32.f), sy = __float2int_rn(my * 32.f);
    const float* wxp = stab + (sx & 31) * 4;
    const float* wyp = stab + (sy & 31) * 4;
    int ixs = sx >> 5, iys = sy >> 5;
    ixs = clampi(ixs, -32768, 32767); iys = clampi(iys, -32768, 32767);   // saturate_cast<short>
    const int ix = ixs - 1, iy = iys - 1;
    float vI = 0.f, vX = 0.f, vY = 0.f;
    if (!(ix >= W || ix + 4 <= 0 || iy >= H || iy + 4 <= 0)) {
        float P[6][6];
        unsigned xo[6], yo[6];                             // unsigned 32-bit BYTE offsets from the frame base (a plane is < 2^24 px):
                                                           // the loads take the scalar-base + 32-bit-offset form, no 64-bit address math
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            xo[i] = (unsigned)clampi(ix - 1 + i, 0, W - 1) * 4u;
            yo[i] = (unsigned)clampi(iy - 1 + i, 0, H - 1) * (unsigned)pitch * 4u;
        }
        const char* base1 = reinterpret_cast<const char*>(I1);
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int i = 0; i < 6; ++i) P[j][i] = *reinterpret_cast<const float*>(base1 + (yo[j] + xo[i]));
        float wgt[16];
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) wgt[k1 * 4 + k2] = wyp[k1] * wxp[k2];
        const unsigned width1 = (unsigned)(W - 3 > 0 ? W - 3 : 0), height1 = (unsigned)(H - 3 > 0 ? H - 3 : 0);
        if ((unsigned)ix < width1 && (unsigned)iy < height1) {
            // interior: each source row summed left to right, rows accumulated in order
#pragma unroll
            for (int k1 = 0; k1 < 4; ++k1) {
                float rI = P[k1 + 1][1] * wgt[k1 * 4];
                float rX = (0.5f * (P[k1 + 1][2] - P[k1 + 1][0])) * wgt[k1 * 4];
                float rY = (0.5f * (P[k1 + 2][1] - P[k1][1])) * wgt[k1 * 4];
#pragma unroll
                for (int k2 = 1; k2 < 4; ++k2) {
                    rI = rI + P[k1 + 1][k2 + 1] * wgt[k1 * 4 + k2];
                    rX = rX + (0.5f * (P[k1 + 1][k2 + 2] - P[k1 + 1][k2])) * wgt[k1 * 4 + k2];
                    rY = rY + (0.5f * (P[k1 + 2][k2 + 1] - P[k1][k2 + 1])) * wgt[k1 * 4 + k2];
                }
                if (k1 == 0) { vI = rI; vX = rX; vY = rY; }
                else { vI += rI; vX += rX; vY += rY; }
            }
        } else {
            // partially outside: constant border 0, valid taps accumulated one by one
#pragma unroll
            for (int k1 = 0; k1 < 4; ++k1) {
                const int yi = iy + k1;
                if (yi < 0 || yi >= H) continue;
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2) {
                    const int xj = ix + k2;
                    if (xj < 0 || xj >= W) continue;
                    vI += P[k1 + 1][k2 + 1] * wgt[k1 * 4 + k2];
                    vX += (0.5f * (P[k1 + 1][k2 + 2] - P[k1 + 1][k2])) * wgt[k1 * 4 + k2];
                    vY += (0.5f * (P[k1 + 2][k2 + 1] - P[k1][k2 + 1])) * wgt[k1 * 4 + k2];
                }
            }
        }
    }
    owx[idx] = vX;
    owy[idx] = vY;
    orho[idx] = ((vI - vX * u1) - vY * u2) - I0[idx];
}

__global__ __launch_bounds__(256) void k_warp(WarpArgs a)
{
    __shared__ float stab[128];
    if (threadIdx.x < 128) stab[threadIdx.x] = a.tab[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int W = a.g.w, H = a.g.h, pitch = a.g.pitch;
    if (x >= W || y >= H) return;
    const int uc = a.ctl[b].ubase & 1;
    const size_t po = (size_t)b * a.g.splane;
    warp_px(stab, a.pyr + (size_t)(a.off0 + b) * a.g.plane, a.pyr + (size_t)(a.off1 + b) * a.g.plane, a.sb.u1[uc] + po, a.sb.u2[uc] + po,
            a.wx + po, a.wy + po, a.rho + po, W, H, pitch, x, y);
}

// ---- cv2.cuda.OpticalFlowDual_TVL1 variant (oracle variant 1) -----------------------------------
// centeredGradientKernel: 0.5 * (next - prev) with replicate at the border, for every frame of a level
__global__ __launch_bounds__(256) void k_grad(const float* __restrict__ src, float* __restrict__ gx, float* __restrict__ gy, Geom g)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.w || y >= g.h) return;
    const size_t fo = (size_t)blockIdx.z * g.plane;
    const float* S = src + fo;
    const size_t i = (size_t)y * g.pitch + x;
    const int xp = x + 1 < g.w ? x + 1 : g.w - 1, xm = x > 0 ? x - 1 : 0, yp = y + 1 < g.h ? y + 1 : g.h - 1, ym = y > 0 ? y - 1 : 0;
    gx[fo + i] = 0.5f * (S[(size_t)y * g.pitch + xp] - S[(size_t)y * g.pitch + xm]);
    gy[fo + i] = 0.5f * (S[(size_t)yp * g.pitch + x] - S[(size_t)ym * g.pitch + x]);
}

__device__ __forceinline__ float cuda_bicubic_coeff(float x_)
{
    const float x = fabsf(x_);
    if (x <= 1.0f) return x * x * (1.5f * x - 2.5f) + 1.0f;
    else if (x < 2.0f) return x * (x * (-0.5f * x + 2.5f) - 4.0f) + 2.0f;
    return 0.0f;
}

struct WarpCudaArgs {
    WarpArgs w;
    const float *gx, *gy;      // centred gradient of this level's frames (same layout as w.pyr)
};

// warpBackwardKernel: weight-normalised Catmull-Rom taps over ceil(w-2)..floor(w+2) with clamp addressing, on I1, I1x, I1y
__global__ __launch_bounds__(256) void k_warp_cuda(WarpCudaArgs A)
{
    const WarpArgs& a = A.w;
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int W = a.g.w, H = a.g.h, pitch = a.g.pitch;
    if (x >= W || y >= H) return;
    const int uc = a.ctl[b].ubase & 1;
    const size_t po = (size_t)b * a.g.splane, idx = (size_t)y * pitch + x;
    const size_t f1 = (size_t)(a.off1 + b) * a.g.plane;
    const float* __restrict__ I0 = a.pyr + (size_t)(a.off0 + b) * a.g.plane;
    const float* __restrict__ I1 = a.pyr + f1;
    const float* __restrict__ I1x = A.gx + f1;
    const float* __restrict__ I1y = A.gy + f1;
    const float u1v = a.sb.u1[uc][po + idx], u2v = a.sb.u2[uc][po + idx];
    const float wx = (float)x + u1v, wy = (float)y + u2v;
    const int xmin = (int)ceilf(wx - 2.0f), xmax = (int)floorf(wx + 2.0f);
    const int ymin = (int)ceilf(wy - 2.0f), ymax = (int)floorf(wy + 2.0f);
    float sum = 0.0f, sumx = 0.0f, sumy = 0.0f, wsum = 0.0f;
    for (int cy = ymin; cy <= ymax; ++cy) {
        const float wyc = cuda_bicubic_coeff(wy - (float)cy);
        const size_t row = (size_t)clampi(cy, 0, H - 1) * pitch;
        for (int cx = xmin; cx <= xmax; ++cx) {
            const float wt = cuda_bicubic_coeff(wx - (float)cx) * wyc;
            const size_t j = row + clampi(cx, 0, W - 1);
            sum += wt * I1[j];
            sumx += wt * I1x[j];
            sumy += wt * I1y[j];
            wsum += wt;
        }
    }
    const float coeff = 1.0f / wsum;
    const float I1w = sum * coeff, gxv = sumx * coeff, gyv = sumy * coeff;
    a.wx[po + idx] = gxv;
    a.wy[po + idx] = gyv;
    a.rho[po + idx] = ((I1w - gxv * u1v) - gyv * u2v) - I0[idx];
}

// ---------------------------------------------------------------------------------------------
// k_warp_lds: same arithmetic as k_warp, but the 36 taps of a pixel come from an LDS copy of the I1 tile plus a margin
// of M pixels (k_warp is L1/TA-bound on its 36 scalar gathers per pixel; ds_read_b32 from a staged tile is ~7x cheaper).
// A pixel whose 6x6 footprint leaves the staged region (|flow| > ~M) falls back to clamped global loads, so the result
// never depends on M.  The staged array holds I1 at UNclamped coordinates with replicate content, which is exactly what
// the clamped patch loads of k_warp read.  All global loads of a thread are in flight together (see median_stage).
// ---------------------------------------------------------------------------------------------
#define WL_TW 64
#define WL_TH 16

__device__ __forceinline__ void warp_accumulate(const float (&P)[6][6], const float* wxp, const float* wyp, int ix, int iy, int W, int H,
                                                float& vI, float& vX, float& vY)
{
    float wgt[16];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) wgt[k1 * 4 + k2] = wyp[k1] * wxp[k2];
    const unsigned width1 = (unsigned)(W - 3 > 0 ? W - 3 : 0), height1 = (unsigned)(H - 3 > 0 ? H - 3 : 0);
    vI = vX = vY = 0.f;
    if ((unsigned)ix < width1 && (unsigned)iy < height1) {
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            float rI = P[k1 + 1][1] * wgt[k1 * 4];
            float rX = (0.5f * (P[k1 + 1][2] - P[k1 + 1][0])) * wgt[k1 * 4];
            float rY = (0.5f * (P[k1 + 2][1] - P[k1][1])) * wgt[k1 * 4];
#pragma unroll
            for (int k2 = 1; k2 < 4; ++k2) {
                rI = rI + P[k1 + 1][k2 + 1] * wgt[k1 * 4 + k2];
                rX = rX + (0.5f * (P[k1 + 1][k2 + 2] - P[k1 + 1][k2])) * wgt[k1 * 4 + k2];
                rY = rY + (0.5f * (P[k1 + 2][k2 + 1] - P[k1][k2 + 1])) * wgt[k1 * 4 + k2];
            }
            if (k1 == 0) { vI = rI; vX = rX; vY = rY; }
            else { vI += rI; vX += rX; vY += rY; }
        }
    } else {
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            const int yi = iy + k1;
            if (yi < 0 || yi >= H) continue;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                const int xj = ix + k2;
                if (xj < 0 || xj >= W) continue;
                vI += P[k1 + 1][k2 + 1] * wgt[k1 * 4 + k2];
                vX += (0.5f * (P[k1 + 1][k2 + 2] - P[k1 + 1][k2])) * wgt[k1 * 4 + k2];
                vY += (0.5f * (P[k1 + 2][k2 + 1] - P[k1][k2 + 1])) * wgt[k1 * 4 + k2];
            }
        }
    }
}

template <int M>
__global__ __launch_bounds__(256) void k_warp_lds(WarpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* stab = smem;                  // [128] bicubic table
    float* S = smem + 128;               // [SH][SW] staged I1 (16-byte aligned rows)
    // horizontal margin M + 4 on both sides (the region then starts on a float4 boundary), vertical M + 3 above / M + 4 below
    constexpr int MX = M + 4, SW = WL_TW + 2 * MX, SH = WL_TH + 2 * M + 7, QW = SW / 4, NQ = QW * SH, NV = (NQ + 255) / 256;
    static_assert(M % 4 == 0, "margin classes are multiples of 4");
    const int b = blockIdx.z;
    const int W = a.g.w, H = a.g.h, pitch = a.g.pitch;
    const int x0 = blockIdx.x * WL_TW, y0 = blockIdx.y * WL_TH;
    const int rx0 = x0 - MX, ry0 = y0 - M - 3;
    const float* __restrict__ I0 = a.pyr + (size_t)(a.off0 + b) * a.g.plane;
    const float* __restrict__ I1 = a.pyr + (size_t)(a.off1 + b) * a.g.plane;
    const int uc = a.ctl[b].ubase & 1;
    const size_t po = (size_t)b * a.g.splane;
    const int lx = threadIdx.x & 63, x = x0 + lx, ty = threadIdx.x >> 6;
    // everything this thread reads from global memory is requested before the first wait: the flow and I0 of its four
    // pixels, then its share of the staged region (float4 where the quad lies inside the image, clamped scalars at the border)
    float u1r[4], u2r[4], i0r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = y0 + ty + 4 * r;
        u1r[r] = u2r[r] = i0r[r] = 0.f;
        if (x < W && y < H) {
            const size_t idx = (size_t)y * pitch + x;
            u1r[r] = a.sb.u1[uc][po + idx]; u2r[r] = a.sb.u2[uc][po + idx]; i0r[r] = I0[idx];
        }
    }
    float4 v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (i < NQ) {
            const int ly = i / QW, gx = rx0 + 4 * (i - ly * QW);
            const float* row = I1 + (size_t)clampi(ry0 + ly, 0, H - 1) * pitch;
            if (gx >= 0 && gx + 3 < W) v[k] = *reinterpret_cast<const float4*>(row + gx);
            else v[k] = make_float4(row[clampi(gx, 0, W - 1)], row[clampi(gx + 1, 0, W - 1)], row[clampi(gx + 2, 0, W - 1)], row[clampi(gx + 3, 0, W - 1)]);
        }
    }
    if (threadIdx.x < 128) stab[threadIdx.x] = a.tab[threadIdx.x];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + 256 * k;
        if (i < NQ) *reinterpret_cast<float4*>(S + 4 * i) = v[k];
    }
    __syncthreads();
    if (x >= W) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = y0 + ty + 4 * r;
        if (y >= H) break;
        const size_t idx = (size_t)y * pitch + x;
        const float u1 = u1r[r], u2 = u2r[r];
        const float mx = (float)x + u1, my = (float)y + u2;
        const int sx = __float2int_rn(mx * 32.f), sy = __float2int_rn(my * 32.f);
        const float* wxp = stab + (sx & 31) * 4;
        const float* wyp = stab + (sy & 31) * 4;
        const int ix = clampi(sx >> 5, -32768, 32767) - 1, iy = clampi(sy >> 5, -32768, 32767) - 1;   // saturate_cast<short>
        float vI = 0.f, vX = 0.f, vY = 0.f;
        if (!(ix >= W || ix + 4 <= 0 || iy >= H || iy + 4 <= 0)) {
            float P[6][6];
            const int px = ix - 1 - rx0, py = iy - 1 - ry0;
            if (px >= 0 && py >= 0 && px + 6 <= SW && py + 6 <= SH) {
                const float* Sp = S + py * SW + px;
#pragma unroll
                for (int j = 0; j < 6; ++j)
#pragma unroll
                    for (int i = 0; i < 6; ++i) P[j][i] = Sp[j * SW + i];
            } else {
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const float* row = I1 + (size_t)clampi(iy - 1 + j, 0, H - 1) * pitch;
#pragma unroll
                    for (int i = 0; i < 6; ++i) P[j][i] = row[clampi(ix - 1 + i, 0, W - 1)];
                }
            }
            warp_accumulate(P, wxp, wyp, ix, iy, W, H, vI, vX, vY);
        }
        a.wx[po + idx] = vX;
        a.wy[po + idx] = vY;
        a.rho[po + idx] = ((vI - vX * u1) - vY * u2) - i0r[r];
    }
}
