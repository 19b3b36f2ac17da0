// teeflow_tvl1_iter.hip.h -- DualTVL1's inner iteration: the stop rules, the exact-arithmetic helpers, the four
// tvl1_iter kernels (tiles / strips, one / two iterations per launch) and the control kernels; included by teeflow_kernels.hip.h
#pragma once

// active(pair, it): did iteration it-1 leave error > threshold?  Slots are zeroed per stage, so a pair
// that stopped earlier reads 0 and stays stopped.
__device__ __forceinline__ bool pair_active(const u64* errb, int it, double thr_q)
{
    if (it == 0) return true;
    return (double)errb[it - 1] > thr_q;
}

// ---------------------------------------------------------------------------------------------
// tvl1_iter: ONE fused inner iteration of procOneScale for a tile:
//   estimateV (threshold TH) -> divergence(p) -> estimateU (+ convergence term) ->
//   forwardGradient(u') -> estimateDualVariables
// 256 threads = 16 quads x 16 rows compute u' on a 64x16 px region (float4 per thread); the block
// OUTPUTS the 60x15 sub-tile whose forward differences it can form from that region (u' goes
// through LDS for the x+1 / y+1 neighbours).  u and p are ping-ponged so neighbouring tiles always
// read the previous iterate.  Algorithmic traffic: 9 plane reads + 6 plane writes = 60 B/px.
// The convergence sum is accumulated exactly (uint64 of rint(t*2^30)), one atomic per block.
// ---------------------------------------------------------------------------------------------
#define IT_TW 64
#define IT_TH 16
#define IT_OW 60
#define IT_OH 15

struct IterArgs {
    const float *wx, *wy, *rho;
    StateBufs sb;
    const PairCtl* ctl;
    u64* err; int errstride; int it; double thr_q;
    int utog, ptog, pzero;
    Geom g;
    float l_t, theta, taut;
    int* host_slot;   // host-mapped word: block 0 publishes how many pairs are still iterating at this launch
    int B;
    int variant;      // 0 = cv2.optflow CPU DualTVL1; 1 = cv2.cuda.OpticalFlowDual_TVL1 stop rule
    double thr_d;     // epsilon^2 * area in double: the CUDA class keeps scaledEpsilon, error and prevError in double (variant 1)
};

// Block 0 / wave 0 tells the host how many of the B pairs enter iteration `it` active, through fine-grained
// host memory.  The host reads it a few launches later (never blocking the stream) to stop enqueuing a stage.
__device__ __forceinline__ void publish_active_count(const IterArgs& a)
{
    if (a.host_slot && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < 64) {
        int c = 0;
        for (int b2 = threadIdx.x; b2 < a.B; b2 += 64)
            c += pair_active(a.err + (size_t)b2 * a.errstride, a.it, a.thr_q) ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (threadIdx.x == 0) __hip_atomic_store(a.host_slot, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- exact arithmetic helpers shared by the four tvl1_iter forms ----------------------------------------
// All of them return the SAME bits as the plain C expressions in the oracle; they only drop work that the
// generic lowering does for operand ranges that cannot occur here.  tests/test_gpu_kernels.py compares the
// results with the oracle bit for bit.
// The iteration kernels are VALU-bound (non-packed fp32 issues one wave64 instruction per 4 cycles), so the pointwise part
// of the quad helpers is written on float2 values spanning two NEIGHBOURING PIXELS: they sit in adjacent registers of the
// dwordx4 loads, so v_pk_mul/add/fma_f32 apply without shuffles.  Each lane does the oracle's operations in the oracle's
// order, hence the same bits.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 mk2(float a, float b) { f2 r; r.x = a; r.y = b; return r; }
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// IEEE a/b as hipcc lowers it (v_rcp_f32, one Newton step on the reciprocal, two on the quotient, v_div_fixup_f32), with
// two changes that keep the bits: (1) the refined reciprocal is shared by the quotients that have the same denominator;
// (2) instead of v_div_scale's case analysis, numerator AND denominator are always scaled by 2^64 -- what v_div_scale does
// for a tiny numerator.  The quotient is unchanged, a power of two commutes with every rounding in the chain, and the
// remainders fma(-b, q, a) cannot underflow.  A quotient in the denormal range is rounded once, by the last fma, like
// v_div_fmas does.  Valid for 2^-24 < |b| < 2^60 and |a| < 2^60 -- here b is 1 + taut*|grad u| >= 1 or |grad I|^2 in
// (2^-23, 2^24) and |a| stays far below 2^60.  `rcp2s` returns 1/(b*2^64).
__device__ __forceinline__ f2 rcp2s(f2 bs)
{
    const f2 r = mk2(__builtin_amdgcn_rcpf(bs.x), __builtin_amdgcn_rcpf(bs.y));
    const f2 e = fma2(-bs, r, mk2(1.0f, 1.0f));
    return fma2(e, r, r);
}
__device__ __forceinline__ f2 div2s(f2 a, f2 b, f2 bs, f2 rs)
{
    const f2 as = a * 0x1p64f;
    f2 q = as * rs;
    f2 e = fma2(-bs, q, as);
    q = fma2(e, rs, q);
    e = fma2(-bs, q, as);
    q = fma2(e, rs, q);
    return mk2(__builtin_amdgcn_div_fixupf(q.x, b.x, a.x), __builtin_amdgcn_div_fixupf(q.y, b.y, a.y));
}

// oracle D2: (float)sqrt((double)a*a + (double)b*b).  a*a, b*b are exact in double, so fma(a,a,b*b) is the same
// single rounding as the sum of the two products.  The square root is the Goldschmidt sequence hipcc emits for
// sqrt(double) (correctly rounded), without its ldexp rescaling for x < 2^-767 (x is 0 or >= 2^-298 here), without its
// x == inf test (a, b are floats: x <= 2^257) and with the x == 0 case folded into a clamp (sqrt(2^-400) converts to
// 0.0f like sqrt(0)).
__device__ __forceinline__ float hypot_exact(float a, float b)
{
    const double ad = (double)a, bd = (double)b;
    const double x = __builtin_fmax(__builtin_fma(ad, ad, bd * bd), 0x1p-400);
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    return (float)g;
}

// estimateV + divergence + estimateU for the 4 pixels of one quad.  `ytop` is uniform per row; only the first pixel of
// the first quad (x == 0) has no left neighbour.
struct QuadU {
    float u1k[4], u2k[4], wx[4], wy[4], r[4];       // current flow and warp constants
    float p11[4], p12[4], p21[4], p22[4];           // dual variable at the pixel
    float p12u[4], p22u[4];                         // ... one row up
    float l11, l21;                                 // ... p11/p21 of the pixel left of the quad
};

// estimateV + divergence + estimateU for two neighbouring pixels; `first` = this is the pair that holds pixel x == 0 of
// the row when x0 is set (only that pixel uses the first-column form of the divergence)
__device__ __forceinline__ void tv_u_pair(float l_t, float theta, f2 u1k, f2 u2k, f2 wx, f2 wy, f2 rc, f2 p11, f2 p12, f2 p21,
                                          f2 p22, f2 p12u, f2 p22u, float l11, float l21, bool ytop, bool x0, f2& u1n, f2& u2n)
{
    // estimateV, branch-free: the three cases of the thresholding step become selects (the quotient is computed in
    // every lane and discarded where it does not apply; straight-line code lets the pixels interleave)
    const f2 Ix2 = wx * wx, Iy2 = wy * wy;
    const f2 grad = Ix2 + Iy2;
    const f2 rho = rc + (wx * u1k + wy * u2k);
    const f2 lg = l_t * grad;
    const f2 grads = grad * 0x1p64f;
    const f2 fi = div2s(-rho, grad, grads, rcp2s(grads));
    const bool c1x = rho.x < -lg.x, c2x = rho.x > lg.x, c3x = grad.x > FLT_EPSILON;
    const bool c1y = rho.y < -lg.y, c2y = rho.y > lg.y, c3y = grad.y > FLT_EPSILON;
    const f2 k = mk2(c1x ? l_t : (c2x ? -l_t : fi.x), c1y ? l_t : (c2y ? -l_t : fi.y));
    const f2 kd1 = k * wx, kd2 = k * wy;
    const bool anyx = c1x || c2x || c3x, anyy = c1y || c2y || c3y;
    const f2 d1 = mk2(anyx ? kd1.x : 0.f, anyy ? kd1.y : 0.f), d2 = mk2(anyx ? kd2.x : 0.f, anyy ? kd2.y : 0.f);
    const f2 v1 = u1k + d1, v2 = u2k + d2;
    // divergence: backward differences with upstream's first-row / first-column forms
    const f2 dx1 = mk2(p11.x - l11, p11.y - p11.x), dx2 = mk2(p21.x - l21, p21.y - p21.x);
    f2 div1, div2_;
    if (!ytop) {
        div1 = dx1 + (p12 - p12u); div2_ = dx2 + (p22 - p22u);
        const float b1 = (p11.x + p12.x) - p12u.x, b2 = (p21.x + p22.x) - p22u.x;
        div1.x = x0 ? b1 : div1.x; div2_.x = x0 ? b2 : div2_.x;
    } else {
        div1 = dx1 + p12; div2_ = dx2 + p22;
        const float b1 = p11.x + p12.x, b2 = p21.x + p22.x;
        div1.x = x0 ? b1 : div1.x; div2_.x = x0 ? b2 : div2_.x;
    }
    u1n = v1 + theta * div1;
    u2n = v2 + theta * div2_;
}

__device__ __forceinline__ void tv_u_quad(float l_t, float theta, const QuadU& q, bool ytop, bool x0, float* u1n, float* u2n)
{
    f2 a1, a2, b1, b2;
    tv_u_pair(l_t, theta, mk2(q.u1k[0], q.u1k[1]), mk2(q.u2k[0], q.u2k[1]), mk2(q.wx[0], q.wx[1]), mk2(q.wy[0], q.wy[1]),
              mk2(q.r[0], q.r[1]), mk2(q.p11[0], q.p11[1]), mk2(q.p12[0], q.p12[1]), mk2(q.p21[0], q.p21[1]),
              mk2(q.p22[0], q.p22[1]), mk2(q.p12u[0], q.p12u[1]), mk2(q.p22u[0], q.p22u[1]), q.l11, q.l21, ytop, x0, a1, a2);
    tv_u_pair(l_t, theta, mk2(q.u1k[2], q.u1k[3]), mk2(q.u2k[2], q.u2k[3]), mk2(q.wx[2], q.wx[3]), mk2(q.wy[2], q.wy[3]),
              mk2(q.r[2], q.r[3]), mk2(q.p11[2], q.p11[3]), mk2(q.p12[2], q.p12[3]), mk2(q.p21[2], q.p21[3]),
              mk2(q.p22[2], q.p22[3]), mk2(q.p12u[2], q.p12u[3]), mk2(q.p22u[2], q.p22u[3]), q.p11[1], q.p21[1], ytop, false, b1, b2);
    u1n[0] = a1.x; u1n[1] = a1.y; u1n[2] = b1.x; u1n[3] = b1.y;
    u2n[0] = a2.x; u2n[1] = a2.y; u2n[2] = b2.x; u2n[3] = b2.y;
}

// convergence terms of a quad, added to a double accumulator: every term is an integer below 2^43, so the sum is exact
// while it stays below 2^53 (the row march folds its accumulator into a u64 every 256 steps, the other kernels per quad).
// `keep[i]` is all-ones for a pixel that counts and 0 for one that does not (halo rows, columns >= W).  Masks, not
// selects: a v_cndmask whose VCC was produced by the scalar unit (row predicate AND column predicate) costs ~23 cycles on
// gfx950 against 2.5 for a v_and.
__device__ __forceinline__ unsigned opaque_u(unsigned m) { asm volatile("" : "+v"(m)); return m; }
__device__ __forceinline__ float mask_f(float v, unsigned m) { return __uint_as_float(__float_as_uint(v) & m); }

__device__ __forceinline__ double tv_err_quad(const float* u1n, const float* u1k, const float* u2n, const float* u2k,
                                              const unsigned* keep)
{
    const f2 e1a = mk2(u1n[0], u1n[1]) - mk2(u1k[0], u1k[1]), e2a = mk2(u2n[0], u2n[1]) - mk2(u2k[0], u2k[1]);
    const f2 e1b = mk2(u1n[2], u1n[3]) - mk2(u1k[2], u1k[3]), e2b = mk2(u2n[2], u2n[3]) - mk2(u2k[2], u2k[3]);
    const f2 ta = e1a * e1a + e2a * e2a, tb = e1b * e1b + e2b * e2b;
    const float t[4] = {ta.x, ta.y, tb.x, tb.y};
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v = __builtin_rintf(fminf(t[i], ERR_CAP_F) * ERR_SCALE_F);
        acc += (double)mask_f(v, keep[i]);
    }
    return acc;
}

// estimateDualVariables for two neighbouring pixels, both flow components.  The two quotients by the same
// 1 + taut*|grad u| share one reciprocal; div2s scales unconditionally so that this needs no guard.  (A shared-reciprocal
// division that kept v_div_scale's operand range with a wave vote was bit-exact but 15 % SLOWER than the compiler's IEEE
// `/`: the vote splits the basic block and stops the 16 divisions of a quad from interleaving.)
__device__ __forceinline__ void tv_p_pair(float taut, f2 u1x, f2 u1y, f2 u2x, f2 u2y, f2 p11, f2 p12, f2 p21, f2 p22,
                                          f2& o11, f2& o12, f2& o21, f2& o22)
{
    const f2 g1 = mk2(hypot_exact(u1x.x, u1y.x), hypot_exact(u1x.y, u1y.y));
    const f2 g2 = mk2(hypot_exact(u2x.x, u2y.x), hypot_exact(u2x.y, u2y.y));
    const f2 ng1 = 1.0f + taut * g1, ng2 = 1.0f + taut * g2;
    const f2 ns1 = ng1 * 0x1p64f, ns2 = ng2 * 0x1p64f;
    const f2 r1 = rcp2s(ns1), r2 = rcp2s(ns2);
    o11 = div2s(p11 + taut * u1x, ng1, ns1, r1); o12 = div2s(p12 + taut * u1y, ng1, ns1, r1);
    o21 = div2s(p21 + taut * u2x, ng2, ns2, r2); o22 = div2s(p22 + taut * u2y, ng2, ns2, r2);
}

__device__ __forceinline__ void tv_p_quad(float taut, const float* u1x, const float* u1y, const float* u2x, const float* u2y,
                                          const float* p11, const float* p12, const float* p21, const float* p22,
                                          float* o11, float* o12, float* o21, float* o22)
{
#pragma unroll
    for (int h = 0; h < 4; h += 2) {
        f2 a, b, c, d;
        tv_p_pair(taut, mk2(u1x[h], u1x[h + 1]), mk2(u1y[h], u1y[h + 1]), mk2(u2x[h], u2x[h + 1]), mk2(u2y[h], u2y[h + 1]),
                  mk2(p11[h], p11[h + 1]), mk2(p12[h], p12[h + 1]), mk2(p21[h], p21[h + 1]), mk2(p22[h], p22[h + 1]), a, b, c, d);
        o11[h] = a.x; o11[h + 1] = a.y; o12[h] = b.x; o12[h + 1] = b.y;
        o21[h] = c.x; o21[h + 1] = c.y; o22[h] = d.x; o22[h + 1] = d.y;
    }
}

// exact convergence sum of a block of `nwaves` waves: shuffle reduction -> one partial per wave in LDS -> one atomic per block
__device__ __forceinline__ void block_err_add(u64 q, u64* sred, int nwaves, u64* slot)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_down(q, off, 64);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 tot = 0;
        for (int w = 0; w < nwaves; ++w) tot += sred[w];
        atomicAdd(slot, tot);
    }
}

__global__ __launch_bounds__(256) void k_iter(IterArgs a)
{
    __shared__ __attribute__((aligned(16))) float su1[IT_TH][IT_TW + 4];
    __shared__ __attribute__((aligned(16))) float su2[IT_TH][IT_TW + 4];
    __shared__ u64 sred[4];
    publish_active_count(a);
    const int b = blockIdx.z;
    u64* errb = a.err + (size_t)b * a.errstride;
    if (!pair_active(errb, a.it, a.thr_q)) return;   // block-uniform
    const PairCtl c = a.ctl[b];
    const int uc = (c.ubase ^ a.utog) & 1, pc = (c.pbase ^ a.ptog) & 1;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int W = a.g.w, H = a.g.h, pitch = a.g.pitch;
    const int x = blockIdx.x * IT_OW + tx * 4, y = blockIdx.y * IT_OH + ty;
    const bool inr = x < W && y < H;
    const size_t po = (size_t)b * a.g.splane;
    const size_t row = po + (size_t)y * pitch + x;

    float u1n[4], u2n[4], p11c[4], p12c[4], p21c[4], p22c[4];
    u64 q = 0;
    const bool outr = inr && tx < 15 && ty < 15;
    if (inr) {
        const float4 u1q = ld4(a.sb.u1[uc] + row), u2q = ld4(a.sb.u2[uc] + row);
        const float4 wxq = ld4(a.wx + row), wyq = ld4(a.wy + row), rq = ld4(a.rho + row);
        float4 a11 = make_float4(0, 0, 0, 0), a12 = a11, a21 = a11, a22 = a11, up12 = a11, up22 = a11;
        float l11 = 0.f, l21 = 0.f;
        if (!a.pzero) {
            a11 = ld4(a.sb.p11[pc] + row); a12 = ld4(a.sb.p12[pc] + row);
            a21 = ld4(a.sb.p21[pc] + row); a22 = ld4(a.sb.p22[pc] + row);
            if (y > 0) { up12 = ld4(a.sb.p12[pc] + row - pitch); up22 = ld4(a.sb.p22[pc] + row - pitch); }
            if (x > 0) { l11 = a.sb.p11[pc][row - 1]; l21 = a.sb.p21[pc][row - 1]; }
        }
        QuadU qu;
        UNPACK4(qu.u1k, u1q) UNPACK4(qu.u2k, u2q) UNPACK4(qu.wx, wxq) UNPACK4(qu.wy, wyq) UNPACK4(qu.r, rq)
        UNPACK4(qu.p11, a11) UNPACK4(qu.p12, a12) UNPACK4(qu.p21, a21) UNPACK4(qu.p22, a22)
        UNPACK4(qu.p12u, up12) UNPACK4(qu.p22u, up22)
        qu.l11 = l11; qu.l21 = l21;
        UNPACK4(p11c, a11) UNPACK4(p12c, a12) UNPACK4(p21c, a21) UNPACK4(p22c, a22)
        tv_u_quad(a.l_t, a.theta, qu, y == 0, x == 0, u1n, u2n);
        unsigned keep[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[i] = outr && x + i < W ? ~0u : 0u;
        q += (u64)tv_err_quad(u1n, qu.u1k, u2n, qu.u2k, keep);
        st4(&su1[ty][tx * 4], make_float4(u1n[0], u1n[1], u1n[2], u1n[3]));
        st4(&su2[ty][tx * 4], make_float4(u2n[0], u2n[1], u2n[2], u2n[3]));
    }
    __syncthreads();
    if (outr) {
        float o11[4], o12[4], o21[4], o22[4], u1x[4], u1y[4], u2x[4], u2y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xi = x + i;
            // forwardGradient of u' (0 in the last column / row)
            const float r1 = i < 3 ? u1n[i + 1] : su1[ty][tx * 4 + 4];
            const float r2 = i < 3 ? u2n[i + 1] : su2[ty][tx * 4 + 4];
            u1x[i] = xi < W - 1 ? r1 - u1n[i] : 0.f;
            u2x[i] = xi < W - 1 ? r2 - u2n[i] : 0.f;
            u1y[i] = y < H - 1 ? su1[ty + 1][tx * 4 + i] - u1n[i] : 0.f;
            u2y[i] = y < H - 1 ? su2[ty + 1][tx * 4 + i] - u2n[i] : 0.f;
        }
        tv_p_quad(a.taut, u1x, u1y, u2x, u2y, p11c, p12c, p21c, p22c, o11, o12, o21, o22);
        st4(a.sb.u1[uc ^ 1] + row, make_float4(u1n[0], u1n[1], u1n[2], u1n[3]));
        st4(a.sb.u2[uc ^ 1] + row, make_float4(u2n[0], u2n[1], u2n[2], u2n[3]));
        st4(a.sb.p11[pc ^ 1] + row, make_float4(o11[0], o11[1], o11[2], o11[3]));
        st4(a.sb.p12[pc ^ 1] + row, make_float4(o12[0], o12[1], o12[2], o12[3]));
        st4(a.sb.p21[pc ^ 1] + row, make_float4(o21[0], o21[1], o21[2], o21[3]));
        st4(a.sb.p22[pc ^ 1] + row, make_float4(o22[0], o22[1], o22[2], o22[3]));
    }
    block_err_add(q, sred, 4, &errb[a.it]);
}

// ---------------------------------------------------------------------------------------------
// tvl1_iter, row-strip form (single-iteration variant; W <= 2048): same arithmetic as k_iter,
// different traffic shape.  A block owns R full-width rows of one pair and marches down them RY rows
// per step (thread = one float4 quad of one row).  Full-width rows mean every 128-B line of every plane
// is fetched exactly once per launch (no x halo; the 64x16 tiles of k_iter start at 240-B offsets and
// fetch ~1.8x the algorithmic bytes at the fabric), and the only re-computation is one halo row per
// strip for the forward difference in y.  Neighbour exchange (p12/p22 of the row above, p11/p21 of the
// quad to the left, u' of the quad to the right and of the row below) goes through LDS; the dual
// update of a row is deferred by one step until the u' row below it exists.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void k_iter_rows(IterArgs a, int R, int QX, int RY)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int LW = QX * 4 + 4;
    u64* sred = reinterpret_cast<u64*>(smem);      // 8 x u64 (one per wave, blocks have up to 512 threads)
    float* su1 = smem + 32;                        // [2][RY][LW]   u1' rows of this / the previous step
    float* su2 = su1 + 2 * RY * LW;
    float* sp12 = su2 + 2 * RY * LW;               // [2][RY][LW]   old p12 rows (the row below reads them)
    float* sp22 = sp12 + 2 * RY * LW;
    float* sp11w = sp22 + 2 * RY * LW;             // [RY][QX]      last element of each quad of old p11
    float* sp21w = sp11w + RY * QX;

    publish_active_count(a);
    const int b = blockIdx.z;
    u64* errb = a.err + (size_t)b * a.errstride;
    if (!pair_active(errb, a.it, a.thr_q)) return;   // block-uniform
    const PairCtl c = a.ctl[b];
    const int uc = (c.ubase ^ a.utog) & 1, pc = (c.pbase ^ a.ptog) & 1;
    const int tid = threadIdx.x;
    const int ty = tid / QX, tx = tid - ty * QX;
    const bool lane_on = ty < RY;
    const int W = a.g.w, H = a.g.h, pitch = a.g.pitch;
    const int x = tx * 4;
    const int y0 = blockIdx.x * R;
    const int nsteps = R / RY;
    const size_t po = (size_t)b * a.g.splane;

    const float* __restrict__ gu1 = a.sb.u1[uc] + po;
    const float* __restrict__ gu2 = a.sb.u2[uc] + po;
    const float* __restrict__ g11 = a.sb.p11[pc] + po;
    const float* __restrict__ g12 = a.sb.p12[pc] + po;
    const float* __restrict__ g21 = a.sb.p21[pc] + po;
    const float* __restrict__ g22 = a.sb.p22[pc] + po;
    const float* __restrict__ gwx = a.wx + po;
    const float* __restrict__ gwy = a.wy + po;
    const float* __restrict__ grh = a.rho + po;

    // state of the previous step's row, waiting for the u' row below it
    float pu1[4] = {0, 0, 0, 0}, pu2[4] = {0, 0, 0, 0}, q11[4], q12[4], q21[4], q22[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q11[i] = q12[i] = q21[i] = q22[i] = 0.f;
    bool prev_out = false;
    int prev_y = 0;
    u64 q = 0;

    for (int s = 0; s <= nsteps; ++s) {
        const int cur = s & 1;
        const int y = y0 + s * RY + ty;
        const bool valid = lane_on && y < H && (s < nsteps || ty == 0);   // step nsteps = the halo row (u' only)
        const bool is_out = lane_on && s < nsteps && y < H;
        const size_t row = (size_t)y * pitch + x;
        float4 u1q, u2q, wxq, wyq, rq, a11, a12, a21, a22;
        u1q = u2q = wxq = wyq = rq = a11 = a12 = a21 = a22 = make_float4(0, 0, 0, 0);
        if (valid) {
            u1q = ld4(gu1 + row); u2q = ld4(gu2 + row);
            wxq = ld4(gwx + row); wyq = ld4(gwy + row); rq = ld4(grh + row);
            if (!a.pzero) { a11 = ld4(g11 + row); a12 = ld4(g12 + row); a21 = ld4(g21 + row); a22 = ld4(g22 + row); }
            st4(sp12 + (cur * RY + ty) * LW + x, a12);
            st4(sp22 + (cur * RY + ty) * LW + x, a22);
            sp11w[ty * QX + tx] = a11.w;
            sp21w[ty * QX + tx] = a21.w;
        }
        __syncthreads();
        float u1n[4] = {0, 0, 0, 0}, u2n[4] = {0, 0, 0, 0};
        if (valid) {
            float4 up12 = make_float4(0, 0, 0, 0), up22 = up12;
            if (y > 0) {
                if (ty > 0) { up12 = ld4(sp12 + (cur * RY + ty - 1) * LW + x); up22 = ld4(sp22 + (cur * RY + ty - 1) * LW + x); }
                else if (s > 0) { up12 = ld4(sp12 + ((cur ^ 1) * RY + RY - 1) * LW + x); up22 = ld4(sp22 + ((cur ^ 1) * RY + RY - 1) * LW + x); }
                else if (!a.pzero) { up12 = ld4(g12 + row - pitch); up22 = ld4(g22 + row - pitch); }
            }
            float l11 = 0.f, l21 = 0.f;
            if (tx > 0) { l11 = sp11w[ty * QX + tx - 1]; l21 = sp21w[ty * QX + tx - 1]; }
            QuadU qu;
            UNPACK4(qu.u1k, u1q) UNPACK4(qu.u2k, u2q) UNPACK4(qu.wx, wxq) UNPACK4(qu.wy, wyq) UNPACK4(qu.r, rq)
            UNPACK4(qu.p11, a11) UNPACK4(qu.p12, a12) UNPACK4(qu.p21, a21) UNPACK4(qu.p22, a22)
            UNPACK4(qu.p12u, up12) UNPACK4(qu.p22u, up22)
            qu.l11 = l11; qu.l21 = l21;
            tv_u_quad(a.l_t, a.theta, qu, y == 0, x == 0, u1n, u2n);
            unsigned keep[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) keep[i] = is_out && x + i < W ? ~0u : 0u;
            q += (u64)tv_err_quad(u1n, qu.u1k, u2n, qu.u2k, keep);
            st4(su1 + (cur * RY + ty) * LW + x, make_float4(u1n[0], u1n[1], u1n[2], u1n[3]));
            st4(su2 + (cur * RY + ty) * LW + x, make_float4(u2n[0], u2n[1], u2n[2], u2n[3]));
            // keep this row's old p for its deferred dual update (after the previous row's update below)
        }
        __syncthreads();
        if (prev_out) {
            // dual update of the previous step's row: forward differences of u' (0 in the last column / row)
            const float* d1 = ty < RY - 1 ? su1 + ((cur ^ 1) * RY + ty + 1) * LW + x : su1 + (cur * RY) * LW + x;
            const float* d2 = ty < RY - 1 ? su2 + ((cur ^ 1) * RY + ty + 1) * LW + x : su2 + (cur * RY) * LW + x;
            const bool lastrow = prev_y >= H - 1;
            float4 dn1 = make_float4(0, 0, 0, 0), dn2 = dn1;
            if (!lastrow) { dn1 = ld4(d1); dn2 = ld4(d2); }
            float r1 = 0.f, r2 = 0.f;
            if (x + 4 < W) { r1 = su1[((cur ^ 1) * RY + ty) * LW + x + 4]; r2 = su2[((cur ^ 1) * RY + ty) * LW + x + 4]; }
            const float dv1[4] = {dn1.x, dn1.y, dn1.z, dn1.w}, dv2[4] = {dn2.x, dn2.y, dn2.z, dn2.w};
            float o11[4], o12[4], o21[4], o22[4], u1x[4], u1y[4], u2x[4], u2y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xi = x + i;
                const float n1 = i < 3 ? pu1[i + 1] : r1, n2 = i < 3 ? pu2[i + 1] : r2;
                u1x[i] = xi < W - 1 ? n1 - pu1[i] : 0.f;
                u2x[i] = xi < W - 1 ? n2 - pu2[i] : 0.f;
                u1y[i] = !lastrow ? dv1[i] - pu1[i] : 0.f;
                u2y[i] = !lastrow ? dv2[i] - pu2[i] : 0.f;
            }
            tv_p_quad(a.taut, u1x, u1y, u2x, u2y, q11, q12, q21, q22, o11, o12, o21, o22);
            const size_t prow = po + (size_t)prev_y * pitch + x;
            st4(a.sb.u1[uc ^ 1] + prow, make_float4(pu1[0], pu1[1], pu1[2], pu1[3]));
            st4(a.sb.u2[uc ^ 1] + prow, make_float4(pu2[0], pu2[1], pu2[2], pu2[3]));
            st4(a.sb.p11[pc ^ 1] + prow, make_float4(o11[0], o11[1], o11[2], o11[3]));
            st4(a.sb.p12[pc ^ 1] + prow, make_float4(o12[0], o12[1], o12[2], o12[3]));
            st4(a.sb.p21[pc ^ 1] + prow, make_float4(o21[0], o21[1], o21[2], o21[3]));
            st4(a.sb.p22[pc ^ 1] + prow, make_float4(o22[0], o22[1], o22[2], o22[3]));
        }
        // rotate: this step's row becomes the pending one
        prev_out = is_out;
        prev_y = y;
#pragma unroll
        for (int i = 0; i < 4; ++i) { pu1[i] = u1n[i]; pu2[i] = u2n[i]; }
        q11[0] = a11.x; q11[1] = a11.y; q11[2] = a11.z; q11[3] = a11.w;
        q12[0] = a12.x; q12[1] = a12.y; q12[2] = a12.z; q12[3] = a12.w;
        q21[0] = a21.x; q21[1] = a21.y; q21[2] = a21.z; q21[3] = a21.w;
        q22[0] = a22.x; q22[1] = a22.y; q22[2] = a22.z; q22[3] = a22.w;
    }
    block_err_add(q, sred, (int)(blockDim.x >> 6), &errb[a.it]);
}

// ---------------------------------------------------------------------------------------------
// tvl1_iter x2: TWO inner iterations per launch inside the row march (time skewing).  The strip's rows flow
// through a 3-stage pipeline, one row group per step:
//     stage 1 (group s)   : load row, u1 = U(u0, p0)                         [iteration `it`]
//     stage 2 (group s-1) : p1 = P(p0, u1) ; u2 = U(u1, p1)                   [`it` dual, `it+1` primal]
//     stage 3 (group s-2) : p2 = P(p1, u2) ; store u2, p2                     [`it+1` dual]
// so the 9 input planes are read once and the 6 state planes written once per TWO iterations (30 B/px per
// iteration instead of 60).  Extra work: one halo row above and two below each strip.
//
// Stopping stays exact.  A launch covers iterations (it, it+1); both error sums are accumulated.  If a pair
// met the threshold already at `it`, the launch overshot by one iteration; the state it read is still
// intact in the other ping-pong half, so the NEXT launch re-runs that pair in REPLAY mode: iteration `it`
// alone, from the previous launch's source buffers into its destination buffers (no error accumulation).
//   active_at(j)  = j == 0 || (err[j-2] > thr && err[j-1] > thr)           (j even; slots are zeroed per stage)
//   NORMAL  at it : it < total && active_at(it)
//   REPLAY  at it : it >= 2 && active_at(it-2) && !(err[it-2] > thr)
// ---------------------------------------------------------------------------------------------
#define M_EXIT 0
#define M_NORMAL 1
#define M_REPLAY 2

__device__ __forceinline__ int pair_mode2(const u64* e, int it, int total, double thr)
{
    const bool a1 = it >= 1 ? (double)e[it - 1] > thr : true;
    const bool a2 = it >= 2 ? (double)e[it - 2] > thr : true;
    if (it < total && (it == 0 || (a2 && a1))) return M_NORMAL;
    if (it >= 2 && !a2) {
        const int j = it - 2;
        const bool act = j == 0 || ((double)e[j - 2] > thr && (double)e[j - 1] > thr);
        if (act) return M_REPLAY;
    }
    return M_EXIT;
}

// Stop rule of cv2.cuda.OpticalFlowDual_TVL1 (cudaoptflow tvl1flow.cpp procOneScale, restated in oracle/tvl1_oracle.c
// variant 1): one loop of `total` iterations; the error sum is looked at only on odd iterations n, and only once the
// running prevError (last seen error, minus the threshold for every iteration without a look) has dropped below the
// threshold.  A stop can therefore only follow an odd iteration = the second one of a launch: no REPLAY in this variant.
// Replays the recurrence over iterations [0, it): M_NORMAL if the pair still iterates at launch `it`, else M_EXIT with
// *n_it = iterations executed.
__device__ __forceinline__ int pair_mode_cuda(const u64* e, int it, int total, double thr, int* n_it)
{
    // cudaoptflow procOneScale keeps scaledEpsilon / error / prevError in double ([UPSTREAM-FROM-MEMORY]; a float
    // `prevError -= scaledEpsilon` could flip the iteration at which the sum is next consulted)
    double prev = 0.0;
    for (int n = 0; n < it; ++n) {
        const bool calc = thr > 0.0 && (n & 1) && prev < thr;
        if (calc) {
            const double err = (double)e[n] * 0x1p-30;
            prev = err;
            if (!(err > thr)) { if (n_it) *n_it = n + 1; return M_EXIT; }
        } else prev -= thr;
    }
    if (n_it) *n_it = total;
    return it < total ? M_NORMAL : M_EXIT;
}

__device__ __forceinline__ int pair_mode(const u64* e, int it, int total, double thr_q, int variant, double thr_d)
{
    return variant ? pair_mode_cuda(e, it, total, thr_d, nullptr) : pair_mode2(e, it, total, thr_q);
}

// Work items of a tvl1_iter launch when the strips are sized ON THE DEVICE from the number of pairs that still
// iterate (`n`): one round of at most `slots` resident blocks (slots = CUs x blocks per CU), each marching a strip that is
// as long as that allows -- a lock-step batch loses a third of its time otherwise (a launch with 1024 blocks on 768 slots
// takes two rounds, one with 300 takes as long as one with 768).  Returns rows per strip and the strip count.
TF_HD inline void strip_rule_min(int n, int H, int minrows, int slots, int* R, int* S)
{
    if (n < 1) n = 1;
    if (minrows < 1) minrows = 1;
    const int k = (n + slots - 1) / slots;                 // rounds
    int s = (int)(((long long)k * slots) / n);
    const int smax = H / minrows > 0 ? H / minrows : 1;    // no strip shorter than `minrows` rows (each pays ~3 halo rows)
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    int r = (H + s - 1) / s;
    *R = r;
    *S = (H + r - 1) / r;
}
TF_HD inline void strip_rule(int n, int H, int RY, int slots, int* R, int* S)
{
    strip_rule_min(n, H, 4 * RY, slots, R, S);            // at least 4 steps per strip
}

struct Iter2Args {
    IterArgs a;                           // a.it = first iteration of the launch (even), a.utog/ptog/pzero for it
    int utog_prev, ptog_prev, pzero_prev; // the same three for the previous launch (used by REPLAY blocks)
    int total;                            // inner*outer
};

__device__ __forceinline__ void publish_active_count2(const Iter2Args& A)
{
    const IterArgs& a = A.a;
    if (a.host_slot && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x < 64) {
        int c = 0;
        for (int b2 = threadIdx.x; b2 < a.B; b2 += 64)
            c += pair_mode(a.err + (size_t)b2 * a.errstride, a.it, A.total, a.thr_q, a.variant, a.thr_d) != M_EXIT ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if (threadIdx.x == 0) __hip_atomic_store(a.host_slot, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}


// What one block of the two-iteration row march needs to know: which pair and strip, the strip length, the block shape
// and the pair's mode.  k_iter2_rows derives it from launch-uniform arguments + the pair's error slots and hands it to
// iter2_rows_body.  (Two functions on purpose: written as one, the kernel compiles to another instruction stream, and the stored
// profiles and instruction counts of k_iter2_rows are of this one.)
struct Iter2Blk {
    int b, strip, R, QX, RY;
    bool replay, pzero;
    int uc, pc;          // ping-pong halves the block READS u / p from (it writes the other ones)
    int it;              // first of the two iterations (error slots it, it+1)
    u64* errb;           // the pair's error slots
    int W, H, pitch;     // geometry of the pair's level
    long long splane;    // floats between consecutive pairs in the state / constant buffers
};

__device__ __forceinline__ void iter2_rows_body(const IterArgs& a, const Iter2Blk& k, float* smem);

// `slots` > 0: grid = (max work items, 1, 1) and every block finds its (pair, strip) among the pairs that still iterate;
// `slots` == 0: grid = (strips, 1, pairs) with the fixed strip length R.
__global__ __launch_bounds__(512) void k_iter2_rows(Iter2Args A, int R, int QX, int RY, int slots)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const IterArgs& a = A.a;
    u64* sred = reinterpret_cast<u64*>(smem);      // 2 x 8 x u64 = 128 B (one per wave and error sum)

    publish_active_count2(A);
    int b = blockIdx.z, strip = blockIdx.x;
    if (slots > 0) {
        // 64-pair masks of the pairs that are not in EXIT mode (sred is free until the end of the kernel; B <= 1024)
        const int nchunk = (a.B + 63) >> 6, nw = (int)(blockDim.x >> 6), wv = (int)(threadIdx.x >> 6), ln = (int)(threadIdx.x & 63);
        for (int c = wv; c < nchunk; c += nw) {
            const int pb = c * 64 + ln;
            const bool on = pb < a.B && pair_mode(a.err + (size_t)pb * a.errstride, a.it, A.total, a.thr_q, a.variant, a.thr_d) != M_EXIT;
            const u64 m = __ballot(on);
            if (ln == 0) sred[c] = m;
        }
        __syncthreads();
        int nact = 0;
        for (int c = 0; c < nchunk; ++c) nact += __popcll(sred[c]);
        int S;
        strip_rule(nact, a.g.h, RY, slots, &R, &S);
        const int item = blockIdx.x;
        if (item >= nact * S) return;                      // block-uniform
        int k = item / S;
        strip = item - k * S;
        int c = 0;
        u64 m = sred[0];
        while (k >= __popcll(m)) { k -= __popcll(m); m = sred[++c]; }
        for (; k > 0; --k) m &= m - 1;                      // drop the k lowest set bits
        b = c * 64 + (__ffsll((long long)m) - 1);
        __syncthreads();                                    // sred is reused for the error sums below
    }
    u64* errb = a.err + (size_t)b * a.errstride;
    const int mode = pair_mode(errb, a.it, A.total, a.thr_q, a.variant, a.thr_d);   // block-uniform
    if (mode == M_EXIT) return;
    const bool replay = mode == M_REPLAY;
    const PairCtl c = a.ctl[b];
    const int utog = replay ? A.utog_prev : a.utog, ptog = replay ? A.ptog_prev : a.ptog;
    Iter2Blk blk;
    blk.b = b; blk.strip = strip; blk.R = R; blk.QX = QX; blk.RY = RY; blk.replay = replay;
    blk.pzero = (replay ? A.pzero_prev : a.pzero) != 0;
    blk.uc = (c.ubase ^ utog) & 1; blk.pc = (c.pbase ^ ptog) & 1;
    blk.it = a.it; blk.errb = errb;
    blk.W = a.g.w; blk.H = a.g.h; blk.pitch = a.g.pitch; blk.splane = a.g.splane;
    iter2_rows_body(a, blk, smem);
}

__device__ __forceinline__ void iter2_rows_body(const IterArgs& a, const Iter2Blk& k, float* smem)
{
    const int b = k.b, strip = k.strip, R = k.R, QX = k.QX, RY = k.RY, uc = k.uc, pc = k.pc;
    const bool replay = k.replay, pzero = k.pzero;
    u64* errb = k.errb;
    const int LW = QX * 4 + 4;
    u64* sred = reinterpret_cast<u64*>(smem);      // 2 x 8 x u64 = 128 B (one per wave and error sum)
    float* U1a = smem + 32;                        // [2][RY][LW]  u1 (first iterate) plane 1 / 2
    float* U1b = U1a + 2 * RY * LW;
    float* U2a = U1b + 2 * RY * LW;                // [2][RY][LW]  u2 (second iterate)
    float* U2b = U2a + 2 * RY * LW;
    float* B12 = U2b + 2 * RY * LW;                // [RY+1][LW]   rolling rows of p1_12 / p1_22 (p0's row above is
                                                   //              re-read from global/L2: keeps LDS at 3 blocks per CU)
    float* B22 = B12 + (RY + 1) * LW;
    float* B11w = B22 + (RY + 1) * LW;             // [RY][QX]     last element of each quad of p1_11 / p1_21
    float* B21w = B11w + RY * QX;
    const int tid = threadIdx.x;
    const int ty = tid / QX, tx = tid - ty * QX;
    const bool lane_on = ty < RY;
    const int W = k.W, H = k.H, pitch = k.pitch;
    const int x = tx * 4;
    const int y0 = strip * R;
    // the first primal update covers rows y0-1 .. y0+R+1; groups of RY rows start at y0-1 (R need not be a multiple of RY)
    const int ngroups = (R + 3 + RY - 1) / RY;
    const size_t po = (size_t)b * (size_t)k.splane;
    const int RB = RY + 1;

    const float* __restrict__ gu1 = a.sb.u1[uc] + po;
    const float* __restrict__ gu2 = a.sb.u2[uc] + po;
    const float* __restrict__ g11 = a.sb.p11[pc] + po;
    const float* __restrict__ g12 = a.sb.p12[pc] + po;
    const float* __restrict__ g21 = a.sb.p21[pc] + po;
    const float* __restrict__ g22 = a.sb.p22[pc] + po;
    const float* __restrict__ gwx = a.wx + po;
    const float* __restrict__ gwy = a.wy + po;
    const float* __restrict__ grh = a.rho + po;
    float* __restrict__ ou1 = a.sb.u1[uc ^ 1] + po;
    float* __restrict__ ou2 = a.sb.u2[uc ^ 1] + po;
    float* __restrict__ o11 = a.sb.p11[pc ^ 1] + po;
    float* __restrict__ o12 = a.sb.p12[pc ^ 1] + po;
    float* __restrict__ o21 = a.sb.p21[pc ^ 1] + po;
    float* __restrict__ o22 = a.sb.p22[pc ^ 1] + po;

    // row predicates (absolute row index)
    const int yu1_lo = y0 - 1, yu1_hi = y0 + R + 1, yp1_hi = y0 + R, yout_hi = y0 + R - 1;

    // pipeline registers.  Written only under the predicate (s1_valid / s2_valid) they are later read under, so they
    // need no initial value and the predicated-off lanes need no zero fill.
    float s1_u1[4], s1_u2[4], s1_wx[4], s1_wy[4], s1_r[4], s1_11[4], s1_12[4], s1_21[4], s1_22[4];   // stage1 -> stage2
    float s2_u1[4], s2_u2[4], s2_11[4], s2_12[4], s2_21[4], s2_22[4];                                  // stage2 -> stage3
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s1_u1[i] = s1_u2[i] = s1_wx[i] = s1_wy[i] = s1_r[i] = s1_11[i] = s1_12[i] = s1_21[i] = s1_22[i] = 0.f;
        s2_u1[i] = s2_u2[i] = s2_11[i] = s2_12[i] = s2_21[i] = s2_22[i] = 0.f;
    }
    bool s1_valid = false, s2_valid = false;
    // column masks: inw[j] = all-ones iff column x + j lies inside the image (j = 0..4; x itself always does)
    unsigned inw[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) inw[j] = opaque_u(x + j < W ? ~0u : 0u);
    int ring = ty + 1;                                    // (r2 mod RB) for r2 = (s-1)*RY + ty, kept incrementally
    u64 qA = 0, qB = 0;
    double accA = 0.0, accB = 0.0;

    for (int s = 0; s < ngroups + 2; ++s) {
        // ================= stage 1: group s, iteration `it` primal =================
        const int r1 = s * RY + ty;                       // linear row counter inside the strip's pipeline
        const int y = y0 - 1 + r1;
        const bool v1 = lane_on && s < ngroups && y >= 0 && y < H && y >= yu1_lo && y <= yu1_hi;
        const size_t row = (size_t)y * pitch + x;
        float4 u1q, u2q, wxq, wyq, rq, a11, a12, a21, a22;
        u1q = u2q = wxq = wyq = rq = a11 = a12 = a21 = a22 = make_float4(0, 0, 0, 0);
        if (v1) {
            u1q = ld4(gu1 + row); u2q = ld4(gu2 + row);
            wxq = ld4(gwx + row); wyq = ld4(gwy + row); rq = ld4(grh + row);
            if (!pzero) { a11 = ld4(g11 + row); a12 = ld4(g12 + row); a21 = ld4(g21 + row); a22 = ld4(g22 + row); }
        }
        float n_u1[4] = {0, 0, 0, 0}, n_u2[4] = {0, 0, 0, 0};
        float c11[4], c12[4], c21[4], c22[4], wxv[4], wyv[4], rv[4];
        UNPACK4(c11, a11) UNPACK4(c12, a12) UNPACK4(c21, a21) UNPACK4(c22, a22) UNPACK4(wxv, wxq) UNPACK4(wyv, wyq) UNPACK4(rv, rq)
        if (v1) {
            float4 up12 = make_float4(0, 0, 0, 0), up22 = up12;
            if (y > 0 && !pzero) { up12 = ld4(g12 + row - pitch); up22 = ld4(g22 + row - pitch); }
            // dual variable of the pixel left of the quad: one dword each straight from global memory (the line is in
            // L1/L2, the neighbouring lane loads it as part of its float4) -- no LDS exchange, no barrier
            float l11 = 0.f, l21 = 0.f;
            if (tx > 0 && !pzero) { l11 = g11[row - 1]; l21 = g21[row - 1]; }
            QuadU qu;
            UNPACK4(qu.u1k, u1q) UNPACK4(qu.u2k, u2q) UNPACK4(qu.wx, wxq) UNPACK4(qu.wy, wyq) UNPACK4(qu.r, rq)
            UNPACK4(qu.p11, a11) UNPACK4(qu.p12, a12) UNPACK4(qu.p21, a21) UNPACK4(qu.p22, a22)
            UNPACK4(qu.p12u, up12) UNPACK4(qu.p22u, up22)
            qu.l11 = l11; qu.l21 = l21;
            const bool isout = y >= y0 && y <= yout_hi;
            tv_u_quad(a.l_t, a.theta, qu, y == 0, x == 0, n_u1, n_u2);
            const unsigned mrow = opaque_u(!replay && isout ? ~0u : 0u);
            const unsigned keep[4] = {inw[0] & mrow, inw[1] & mrow, inw[2] & mrow, inw[3] & mrow};
            accA += tv_err_quad(n_u1, qu.u1k, n_u2, qu.u2k, keep);
            st4(U1a + ((s & 1) * RY + ty) * LW + x, PACK4(n_u1));
            st4(U1b + ((s & 1) * RY + ty) * LW + x, PACK4(n_u2));
        }
        __syncthreads();
        // ================= stage 2: group s-1: iteration `it` dual, then `it+1` primal =================
        const int yb = y - RY;
        const bool v2 = s1_valid && yb <= yp1_hi;           // s1_valid already implies in-image and >= yu1_lo
        float p1_11[4] = {0, 0, 0, 0}, p1_12[4] = {0, 0, 0, 0}, p1_21[4] = {0, 0, 0, 0}, p1_22[4] = {0, 0, 0, 0};
        if (v2) {
            const int bp = (s - 1) & 1;
            const bool lastrow = yb >= H - 1;
            float4 dn1 = make_float4(0, 0, 0, 0), dn2 = dn1;
            if (!lastrow) {
                const float* d1 = ty < RY - 1 ? U1a + (bp * RY + ty + 1) * LW + x : U1a + ((s & 1) * RY) * LW + x;
                const float* d2 = ty < RY - 1 ? U1b + (bp * RY + ty + 1) * LW + x : U1b + ((s & 1) * RY) * LW + x;
                dn1 = ld4(d1); dn2 = ld4(d2);
            }
            float rr1 = 0.f, rr2 = 0.f;
            if (x + 4 < W) { rr1 = U1a[(bp * RY + ty) * LW + x + 4]; rr2 = U1b[(bp * RY + ty) * LW + x + 4]; }
            const unsigned mnl = opaque_u(lastrow ? 0u : ~0u);
            float dv1[4], dv2[4], u1x[4], u1y[4], u2x[4], u2y[4];
            UNPACK4(dv1, dn1) UNPACK4(dv2, dn2)
            {   // the thread's own quad of the first iterate lives in LDS since stage 1 of the previous step
                const float4 o1 = ld4(U1a + (bp * RY + ty) * LW + x), o2 = ld4(U1b + (bp * RY + ty) * LW + x);
                UNPACK4(s1_u1, o1) UNPACK4(s1_u2, o2)
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e1 = i < 3 ? s1_u1[i + 1] : rr1, e2 = i < 3 ? s1_u2[i + 1] : rr2;
                u1x[i] = mask_f(e1 - s1_u1[i], inw[i + 1]);       // 0 in the last column (x + i == W - 1) and beyond
                u2x[i] = mask_f(e2 - s1_u2[i], inw[i + 1]);
                u1y[i] = mask_f(dv1[i] - s1_u1[i], mnl);          // 0 in the last row
                u2y[i] = mask_f(dv2[i] - s1_u2[i], mnl);
            }
            tv_p_quad(a.taut, u1x, u1y, u2x, u2y, s1_11, s1_12, s1_21, s1_22, p1_11, p1_12, p1_21, p1_22);
            if (replay) {
                if (yb >= y0 && yb <= yout_hi) {
                    const size_t prow = (size_t)yb * pitch + x;
                    st4(ou1 + prow, PACK4(s1_u1)); st4(ou2 + prow, PACK4(s1_u2));
                    st4(o11 + prow, PACK4(p1_11)); st4(o12 + prow, PACK4(p1_12));
                    st4(o21 + prow, PACK4(p1_21)); st4(o22 + prow, PACK4(p1_22));
                }
            } else {
                st4(B12 + ring * LW + x, PACK4(p1_12));
                st4(B22 + ring * LW + x, PACK4(p1_22));
                B11w[ty * QX + tx] = p1_11[3];
                B21w[ty * QX + tx] = p1_21[3];
            }
        }
        bool v2u = false;
        float m_u1[4] = {0, 0, 0, 0}, m_u2[4] = {0, 0, 0, 0};
        if (!replay) {
            __syncthreads();
            v2u = v2 && yb >= y0;                           // rows y0 .. y0+R get the second primal update
            if (v2u) {
                float4 up12 = make_float4(0, 0, 0, 0), up22 = up12;
                if (yb > 0) {
                    const int ri = ring > 0 ? ring - 1 : RB - 1;        // (r2 - 1) mod RB
                    up12 = ld4(B12 + ri * LW + x); up22 = ld4(B22 + ri * LW + x);
                }
                float l11 = 0.f, l21 = 0.f;
                if (tx > 0) { l11 = B11w[ty * QX + tx - 1]; l21 = B21w[ty * QX + tx - 1]; }
                QuadU qu;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    qu.u1k[i] = s1_u1[i]; qu.u2k[i] = s1_u2[i]; qu.wx[i] = s1_wx[i]; qu.wy[i] = s1_wy[i]; qu.r[i] = s1_r[i];
                    qu.p11[i] = p1_11[i]; qu.p12[i] = p1_12[i]; qu.p21[i] = p1_21[i]; qu.p22[i] = p1_22[i];
                }
                UNPACK4(qu.p12u, up12) UNPACK4(qu.p22u, up22)
                qu.l11 = l11; qu.l21 = l21;
                const bool isout = yb <= yout_hi;
                tv_u_quad(a.l_t, a.theta, qu, yb == 0, x == 0, m_u1, m_u2);
                const unsigned mrow = opaque_u(isout ? ~0u : 0u);
                const unsigned keep[4] = {inw[0] & mrow, inw[1] & mrow, inw[2] & mrow, inw[3] & mrow};
                accB += tv_err_quad(m_u1, s1_u1, m_u2, s1_u2, keep);
                st4(U2a + (((s - 1) & 1) * RY + ty) * LW + x, PACK4(m_u1));
                st4(U2b + (((s - 1) & 1) * RY + ty) * LW + x, PACK4(m_u2));
            }
            __syncthreads();
            // ================= stage 3: group s-2: iteration `it+1` dual, store =================
            const int yc = y - 2 * RY;
            if (s2_valid && yc <= yout_hi) {
                const int bq = s & 1;                       // (s-2)&1
                const bool lastrow = yc >= H - 1;
                float4 dn1 = make_float4(0, 0, 0, 0), dn2 = dn1;
                if (!lastrow) {
                    const float* d1 = ty < RY - 1 ? U2a + (bq * RY + ty + 1) * LW + x : U2a + ((bq ^ 1) * RY) * LW + x;
                    const float* d2 = ty < RY - 1 ? U2b + (bq * RY + ty + 1) * LW + x : U2b + ((bq ^ 1) * RY) * LW + x;
                    dn1 = ld4(d1); dn2 = ld4(d2);
                }
                float rr1 = 0.f, rr2 = 0.f;
                if (x + 4 < W) { rr1 = U2a[(bq * RY + ty) * LW + x + 4]; rr2 = U2b[(bq * RY + ty) * LW + x + 4]; }
                const unsigned mnl = opaque_u(lastrow ? 0u : ~0u);
                float dv1[4], dv2[4], r11[4], r12[4], r21[4], r22[4], u1x[4], u1y[4], u2x[4], u2y[4];
                UNPACK4(dv1, dn1) UNPACK4(dv2, dn2)
                {   // own quad of the second iterate: in LDS since stage 2 of the previous step
                    const float4 o1 = ld4(U2a + (bq * RY + ty) * LW + x), o2 = ld4(U2b + (bq * RY + ty) * LW + x);
                    UNPACK4(s2_u1, o1) UNPACK4(s2_u2, o2)
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e1 = i < 3 ? s2_u1[i + 1] : rr1, e2 = i < 3 ? s2_u2[i + 1] : rr2;
                    u1x[i] = mask_f(e1 - s2_u1[i], inw[i + 1]);
                    u2x[i] = mask_f(e2 - s2_u2[i], inw[i + 1]);
                    u1y[i] = mask_f(dv1[i] - s2_u1[i], mnl);
                    u2y[i] = mask_f(dv2[i] - s2_u2[i], mnl);
                }
                tv_p_quad(a.taut, u1x, u1y, u2x, u2y, s2_11, s2_12, s2_21, s2_22, r11, r12, r21, r22);
                const size_t prow = (size_t)yc * pitch + x;
                st4(ou1 + prow, PACK4(s2_u1)); st4(ou2 + prow, PACK4(s2_u2));
                st4(o11 + prow, PACK4(r11)); st4(o12 + prow, PACK4(r12));
                st4(o21 + prow, PACK4(r21)); st4(o22 + prow, PACK4(r22));
            }
        }
        else __syncthreads();       // REPLAY blocks: keep the next step's stage-1 LDS writes behind this step's stage-2 reads
        // ================= rotate the pipeline registers =================
        s2_valid = v2u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            s2_11[i] = p1_11[i]; s2_12[i] = p1_12[i]; s2_21[i] = p1_21[i]; s2_22[i] = p1_22[i];
            s1_wx[i] = wxv[i]; s1_wy[i] = wyv[i]; s1_r[i] = rv[i];
            s1_11[i] = c11[i]; s1_12[i] = c12[i]; s1_21[i] = c21[i]; s1_22[i] = c22[i];
        }
        s1_valid = v1;
        ring += RY; ring = ring >= RB ? ring - RB : ring;
        if ((s & 255) == 255) { qA += (u64)accA; qB += (u64)accB; accA = accB = 0.0; }   // keep the double sums exact
    }
    if (!replay) {
        qA += (u64)accA; qB += (u64)accB;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { qA += __shfl_down(qA, off, 64); qB += __shfl_down(qB, off, 64); }
        __syncthreads();
        if ((tid & 63) == 0) { sred[tid >> 6] = qA; sred[8 + (tid >> 6)] = qB; }
        __syncthreads();
        if (tid == 0) {
            u64 ta = 0, tb = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { ta += sred[w]; tb += sred[8 + w]; }
            atomicAdd(&errb[k.it], ta);
            atomicAdd(&errb[k.it + 1], tb);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// tvl1_iter, two iterations per launch on TILES: the form for launches too small for the row strips (a single pair, a
// handful of pairs) and for levels wider than 2048 px.  Same schedule, modes (NORMAL / REPLAY / EXIT) and arithmetic as
// k_iter2_rows; a block stages a 64 x 16 region (16 quads x 16 rows, region origin 4 px left of and 1 row above its
// outputs) and produces the 52 x 13 outputs whose dependency cone (1 px left / 1 row up for the primal updates, 1 px
// right / 1 row down for the dual updates, twice) stays inside the region:
//     U1 on quads 0..15, rows 0..15 | P1 on quads 0..14, rows 0..14 | U2 on quads 1..14, rows 1..14 | P2, store: quads 1..13, rows 1..13
// Halving the number of dependent launches is what matters here: a single 512 x 512 pair spends its 4 ms in ~390 launches.
// ---------------------------------------------------------------------------------------------
#define T2_OW 52
#define T2_OH 13

__global__ __launch_bounds__(256) void k_iter2_tile(Iter2Args A)
{
    constexpr int LW = 68;
    __shared__ __attribute__((aligned(16))) float sA[16][LW], sB[16][LW];      // u1 / u2 of the first, then of the second iterate
    __shared__ __attribute__((aligned(16))) float s12[16][LW], s22[16][LW];    // p1_12 / p1_22
    __shared__ float s11w[16][16], s21w[16][16];                               // last element of each quad of p1_11 / p1_21
    __shared__ u64 sred[8];
    const IterArgs& a = A.a;
    publish_active_count2(A);
    const int b = blockIdx.z;
    u64* errb = a.err + (size_t)b * a.errstride;
    const int mode = pair_mode(errb, a.it, A.total, a.thr_q, a.variant, a.thr_d);   // block-uniform
    if (mode == M_EXIT) return;
    const bool replay = mode == M_REPLAY;
    const PairCtl c = a.ctl[b];
    const int utog = replay ? A.utog_prev : a.utog, ptog = replay ? A.ptog_prev : a.ptog;
    const bool pzero = (replay ? A.pzero_prev : a.pzero) != 0;
    const int uc = (c.ubase ^ utog) & 1, pc = (c.pbase ^ ptog) & 1;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int W = a.g.w, H = a.g.h, pitch = a.g.pitch;
    const int x = (int)blockIdx.x * T2_OW - 4 + tx * 4, y = (int)blockIdx.y * T2_OH - 1 + ty;
    const bool inr = x >= 0 && x < W && y >= 0 && y < H;
    const bool outq = inr && tx >= 1 && tx <= 13 && ty >= 1 && ty <= 13;        // this thread's quad is an output of the block
    const size_t po = (size_t)b * a.g.splane;
    const size_t row = po + (size_t)(inr ? y : 0) * pitch + (inr ? x : 0);

    unsigned inw[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) inw[j] = opaque_u(x + j < W ? ~0u : 0u);
    const unsigned mnl = opaque_u(y >= H - 1 ? 0u : ~0u);
    const unsigned mout = opaque_u(outq ? ~0u : 0u);
    const unsigned keep[4] = {inw[0] & mout, inw[1] & mout, inw[2] & mout, inw[3] & mout};

    float u0_1[4], u0_2[4], wx[4], wy[4], rc[4], p0_11[4], p0_12[4], p0_21[4], p0_22[4];
    float u1_1[4], u1_2[4];
    double accA = 0.0, accB = 0.0;
    // ---- first primal update on the whole region ----
    if (inr) {
        const float4 u1q = ld4(a.sb.u1[uc] + row), u2q = ld4(a.sb.u2[uc] + row);
        const float4 wxq = ld4(a.wx + row), wyq = ld4(a.wy + row), rq = ld4(a.rho + row);
        float4 a11 = make_float4(0, 0, 0, 0), a12 = a11, a21 = a11, a22 = a11, up12 = a11, up22 = a11;
        float l11 = 0.f, l21 = 0.f;
        if (!pzero) {
            a11 = ld4(a.sb.p11[pc] + row); a12 = ld4(a.sb.p12[pc] + row);
            a21 = ld4(a.sb.p21[pc] + row); a22 = ld4(a.sb.p22[pc] + row);
            if (y > 0) { up12 = ld4(a.sb.p12[pc] + row - pitch); up22 = ld4(a.sb.p22[pc] + row - pitch); }
            if (x > 0) { l11 = a.sb.p11[pc][row - 1]; l21 = a.sb.p21[pc][row - 1]; }
        }
        QuadU qu;
        UNPACK4(qu.u1k, u1q) UNPACK4(qu.u2k, u2q) UNPACK4(qu.wx, wxq) UNPACK4(qu.wy, wyq) UNPACK4(qu.r, rq)
        UNPACK4(qu.p11, a11) UNPACK4(qu.p12, a12) UNPACK4(qu.p21, a21) UNPACK4(qu.p22, a22)
        UNPACK4(qu.p12u, up12) UNPACK4(qu.p22u, up22)
        qu.l11 = l11; qu.l21 = l21;
        UNPACK4(u0_1, u1q) UNPACK4(u0_2, u2q) UNPACK4(wx, wxq) UNPACK4(wy, wyq) UNPACK4(rc, rq)
        UNPACK4(p0_11, a11) UNPACK4(p0_12, a12) UNPACK4(p0_21, a21) UNPACK4(p0_22, a22)
        tv_u_quad(a.l_t, a.theta, qu, y == 0, x == 0, u1_1, u1_2);
        if (!replay) accA += tv_err_quad(u1_1, u0_1, u1_2, u0_2, keep);
        st4(&sA[ty][tx * 4], PACK4(u1_1));
        st4(&sB[ty][tx * 4], PACK4(u1_2));
    }
    __syncthreads();
    // ---- first dual update: quads 0..14, rows 0..14 (the right / lower neighbour of the first iterate is in the region) ----
    float p1_11[4], p1_12[4], p1_21[4], p1_22[4];
    const bool vP1 = inr && tx <= 14 && ty <= 14;
    if (vP1) {
        const float4 dn1 = ld4(&sA[ty + 1][tx * 4]), dn2 = ld4(&sB[ty + 1][tx * 4]);     // masked where y is the last image row
        const float rr1 = sA[ty][tx * 4 + 4], rr2 = sB[ty][tx * 4 + 4];                 // masked where the column is the last one
        float dv1[4], dv2[4], u1x[4], u1y[4], u2x[4], u2y[4];
        UNPACK4(dv1, dn1) UNPACK4(dv2, dn2)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float e1 = i < 3 ? u1_1[i + 1] : rr1, e2 = i < 3 ? u1_2[i + 1] : rr2;
            u1x[i] = mask_f(e1 - u1_1[i], inw[i + 1]); u2x[i] = mask_f(e2 - u1_2[i], inw[i + 1]);
            u1y[i] = mask_f(dv1[i] - u1_1[i], mnl); u2y[i] = mask_f(dv2[i] - u1_2[i], mnl);
        }
        tv_p_quad(a.taut, u1x, u1y, u2x, u2y, p0_11, p0_12, p0_21, p0_22, p1_11, p1_12, p1_21, p1_22);
        if (replay) {
            if (outq) {
                st4(a.sb.u1[uc ^ 1] + row, PACK4(u1_1)); st4(a.sb.u2[uc ^ 1] + row, PACK4(u1_2));
                st4(a.sb.p11[pc ^ 1] + row, PACK4(p1_11)); st4(a.sb.p12[pc ^ 1] + row, PACK4(p1_12));
                st4(a.sb.p21[pc ^ 1] + row, PACK4(p1_21)); st4(a.sb.p22[pc ^ 1] + row, PACK4(p1_22));
            }
        } else {
            st4(&s12[ty][tx * 4], PACK4(p1_12));
            st4(&s22[ty][tx * 4], PACK4(p1_22));
            s11w[ty][tx] = p1_11[3];
            s21w[ty][tx] = p1_21[3];
        }
    }
    if (replay) return;                                                          // block-uniform
    __syncthreads();
    // ---- second primal update: quads 1..14, rows 1..14 ----
    float u2_1[4], u2_2[4];
    const bool vU2 = vP1 && tx >= 1 && ty >= 1;
    if (vU2) {
        const float4 up12 = ld4(&s12[ty - 1][tx * 4]), up22 = ld4(&s22[ty - 1][tx * 4]);  // unused in the first image row
        QuadU qu;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            qu.u1k[i] = u1_1[i]; qu.u2k[i] = u1_2[i]; qu.wx[i] = wx[i]; qu.wy[i] = wy[i]; qu.r[i] = rc[i];
            qu.p11[i] = p1_11[i]; qu.p12[i] = p1_12[i]; qu.p21[i] = p1_21[i]; qu.p22[i] = p1_22[i];
        }
        UNPACK4(qu.p12u, up12) UNPACK4(qu.p22u, up22)
        qu.l11 = s11w[ty][tx - 1]; qu.l21 = s21w[ty][tx - 1];                   // unused for the first image column
        tv_u_quad(a.l_t, a.theta, qu, y == 0, x == 0, u2_1, u2_2);
        accB += tv_err_quad(u2_1, u1_1, u2_2, u1_2, keep);
        st4(&sA[ty][tx * 4], PACK4(u2_1));                                      // the first iterate's LDS copy was last read before the barrier above
        st4(&sB[ty][tx * 4], PACK4(u2_2));
    }
    __syncthreads();
    // ---- second dual update and store: quads 1..13, rows 1..13 ----
    if (outq) {
        const float4 dn1 = ld4(&sA[ty + 1][tx * 4]), dn2 = ld4(&sB[ty + 1][tx * 4]);
        const float rr1 = sA[ty][tx * 4 + 4], rr2 = sB[ty][tx * 4 + 4];
        float dv1[4], dv2[4], u1x[4], u1y[4], u2x[4], u2y[4], o11[4], o12[4], o21[4], o22[4];
        UNPACK4(dv1, dn1) UNPACK4(dv2, dn2)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float e1 = i < 3 ? u2_1[i + 1] : rr1, e2 = i < 3 ? u2_2[i + 1] : rr2;
            u1x[i] = mask_f(e1 - u2_1[i], inw[i + 1]); u2x[i] = mask_f(e2 - u2_2[i], inw[i + 1]);
            u1y[i] = mask_f(dv1[i] - u2_1[i], mnl); u2y[i] = mask_f(dv2[i] - u2_2[i], mnl);
        }
        tv_p_quad(a.taut, u1x, u1y, u2x, u2y, p1_11, p1_12, p1_21, p1_22, o11, o12, o21, o22);
        st4(a.sb.u1[uc ^ 1] + row, PACK4(u2_1)); st4(a.sb.u2[uc ^ 1] + row, PACK4(u2_2));
        st4(a.sb.p11[pc ^ 1] + row, PACK4(o11)); st4(a.sb.p12[pc ^ 1] + row, PACK4(o12));
        st4(a.sb.p21[pc ^ 1] + row, PACK4(o21)); st4(a.sb.p22[pc ^ 1] + row, PACK4(o22));
    }
    u64 qA = (u64)accA, qB = (u64)accB;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { qA += __shfl_down(qA, off, 64); qB += __shfl_down(qB, off, 64); }
    if ((threadIdx.x & 63) == 0) { sred[threadIdx.x >> 6] = qA; sred[4 + (threadIdx.x >> 6)] = qB; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&errb[a.it], sred[0] + sred[1] + sred[2] + sred[3]);
        atomicAdd(&errb[a.it + 1], sred[4] + sred[5] + sred[6] + sred[7]);
    }
}

// ---------------------------------------------------------------------------------------------
// control kernels (a few threads; they keep the stop/continue decisions on the device)
// ---------------------------------------------------------------------------------------------
// end of one (level, warp) stage: executed iteration counts -> stats; advance the ping-pong bases by the launches the pair took
// part in (`step` iterations per launch: n_it, or ceil(n_it/2)) and its medians
__global__ void k_stage_end(const u64* __restrict__ err, int errstride, PairCtl* ctl, int* iters, int B,
                            int total, int inner, int median_on, double thr_q, int level, int warp, int nlev, int warps,
                            int variant, double thr_d, int step)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const u64* e = err + (size_t)b * errstride;
    int n_it = total;
    if (variant) (void)pair_mode_cuda(e, total, total, thr_d, &n_it);
    else
        for (int j = 0; j < total; ++j)
            if (!((double)e[j] > thr_q)) { n_it = j + 1; break; }
    const int n_out = variant ? 0 : (n_it > 0 ? (n_it - 1) / inner + 1 : 0);      // the CUDA variant has no outer loop / median
    const int launches = step == 2 ? (n_it + 1) / 2 : n_it;
    PairCtl c = ctl[b];
    c.ubase = (c.ubase + launches + (median_on ? n_out : 0)) & 1;
    c.pbase = (c.pbase + launches) & 1;
    ctl[b] = c;
    int* o = iters + (((size_t)b * nlev + level) * warps + warp) * 2;
    o[0] = n_it; o[1] = n_out;
}

// mode 0: reset (coarsest level start); mode 1: after k_flow_up (flow moved to the other buffer, p restarts)
__global__ void k_ctl_set(PairCtl* ctl, int B, int mode)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (mode == 0) { ctl[b].ubase = 0; ctl[b].pbase = 0; }
    else { ctl[b].ubase ^= 1; ctl[b].pbase = 0; }
}
