// teeflow_dbg.hip.h -- the tf_dbg_* hooks: single kernels and single stages on caller-supplied planes, for the tests that pin them
// against the oracle; included by teeflow.hip last (one translation unit)
namespace {
// small RAII device buffer of the hooks
template <class T> struct DevBuf { T* p = nullptr; ~DevBuf() { if (p) (void)hipFree(p); } };
using DBuf = DevBuf<float>;

int dbg_up(tf_handle* h, DBuf& d, const float* src, const Geom& g)
{
    HIPC(h, hipMalloc(&d.p, (size_t)g.plane * sizeof(float)));
    // stream-ordered on the handle's (non-blocking) stream: legacy-stream copies would race with its kernels
    HIPC(h, hipMemsetAsync(d.p, 0, (size_t)g.plane * sizeof(float), h->stream));
    if (src) HIPC(h, hipMemcpy2DAsync(d.p, (size_t)g.pitch * 4, src, (size_t)g.w * 4, (size_t)g.w * 4, g.h, hipMemcpyHostToDevice, h->stream));
    return TF_OK;
}
int dbg_down(tf_handle* h, float* dst, const float* d, const Geom& g)
{
    HIPC(h, hipMemcpy2DAsync(dst, (size_t)g.w * 4, d, (size_t)g.pitch * 4, (size_t)g.w * 4, g.h, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return TF_OK;
}

// frames [I0, I1] in one allocation, so that pair 0 = (frame 0, frame 1)
int dbg_up2(tf_handle* h, DBuf& fr, const float* I0, const float* I1, const Geom& g)
{
    HIPC(h, hipMalloc(&fr.p, 2 * (size_t)g.plane * sizeof(float)));
    HIPC(h, hipMemsetAsync(fr.p, 0, 2 * (size_t)g.plane * sizeof(float), h->stream));
    HIPC(h, hipMemcpy2DAsync(fr.p, (size_t)g.pitch * 4, I0, (size_t)g.w * 4, (size_t)g.w * 4, g.h, hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpy2DAsync(fr.p + g.plane, (size_t)g.pitch * 4, I1, (size_t)g.w * 4, (size_t)g.w * 4, g.h, hipMemcpyHostToDevice, h->stream));
    return TF_OK;
}
}  // namespace

// ---- kernel-level hooks --------------------------------------------------------------------------
TF_API int tf_dbg_resize(tf_handle* h, const float* src, int sw, int sh, float* dst, int dw, int dh,
                         double inv_scale_x, double inv_scale_y, float mul)
{
    if (!h || !src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1) return TF_ERR_INVALID_ARG;
    HIPC(h, hipSetDevice(h->dev));
    const Geom gs = make_geom(sw, sh), gd = make_geom(dw, dh);
    DBuf s, d;
    int rc;
    if ((rc = dbg_up(h, s, src, gs)) || (rc = dbg_up(h, d, nullptr, gd))) return rc;
    hipLaunchKernelGGL(k_pyr_down, grid64x4(gd, 1), dim3(256), 0, h->stream, s.p, gs, d.p, gd, 1.0 / inv_scale_x, 1.0 / inv_scale_y);
    HIPC(h, hipStreamSynchronize(h->stream));
    if ((rc = dbg_down(h, dst, d.p, gd))) return rc;
    if (mul != 1.0f) for (size_t i = 0; i < (size_t)dw * dh; ++i) dst[i] *= mul;
    return TF_OK;
}

TF_API int tf_dbg_pyramid(tf_handle* h, const uint8_t* img, int H, int W, int level, float* out, int* ow, int* oh)
{
    if (!h || !img || !ow || !oh || H < 1 || W < 1 || level < 0 || level >= MAXLEV) return TF_ERR_INVALID_ARG;
    HIPC(h, hipSetDevice(h->dev));
    Geom g = make_geom(W, H);
    DevBuf<uint8_t> d8;
    HIPC(h, hipMalloc(&d8.p, (size_t)H * W));
    HIPC(h, hipMemcpyAsync(d8.p, img, (size_t)H * W, hipMemcpyHostToDevice, h->stream));
    DBuf cur;
    int rc = dbg_up(h, cur, nullptr, g);
    if (rc) return rc;
    hipLaunchKernelGGL(k_u8_to_f32, dim3((g.w + 255) / 256, g.h, 1), dim3(256), 0, h->stream, d8.p, cur.p, g);
    for (int s = 1; s <= level; ++s) {
        Geom gn = make_geom(cv_round_d(g.w * h->P.scale_step), cv_round_d(g.h * h->P.scale_step));
        if (gn.w < 1 || gn.h < 1) return fail(h, TF_ERR_INVALID_ARG, "pyramid level %d is empty", s);
        DBuf nxt;
        if ((rc = dbg_up(h, nxt, nullptr, gn))) return rc;
        const double sc = 1.0 / h->P.scale_step;
        hipLaunchKernelGGL(k_pyr_down, grid64x4(gn, 1), dim3(256), 0, h->stream, cur.p, g, nxt.p, gn, sc, sc);
        HIPC(h, hipStreamSynchronize(h->stream));
        std::swap(cur.p, nxt.p);
        g = gn;
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    *ow = g.w; *oh = g.h;
    if (out) return dbg_down(h, out, cur.p, g);
    return TF_OK;
}

TF_API int tf_dbg_warp(tf_handle* h, const float* I0, const float* I1, const float* u1, const float* u2, int w, int hgt,
                       float* I1wx, float* I1wy, float* rho_c)
{
    if (!h || !I0 || !I1 || !u1 || !u2 || !I1wx || !I1wy || !rho_c || w < 1 || hgt < 1) return TF_ERR_INVALID_ARG;
    HIPC(h, hipSetDevice(h->dev));
    const Geom g = make_geom(w, hgt);
    DBuf fr, du1, du2, dwx, dwy, drho;
    int rc;
    if ((rc = dbg_up2(h, fr, I0, I1, g)) || (rc = dbg_up(h, du1, u1, g)) || (rc = dbg_up(h, du2, u2, g)) || (rc = dbg_up(h, dwx, nullptr, g)) ||
        (rc = dbg_up(h, dwy, nullptr, g)) || (rc = dbg_up(h, drho, nullptr, g))) return rc;
    DevBuf<PairCtl> ctl;
    HIPC(h, hipMalloc(&ctl.p, sizeof(PairCtl)));
    HIPC(h, hipMemsetAsync(ctl.p, 0, sizeof(PairCtl), h->stream));
    WarpArgs wa = {};
    wa.pyr = fr.p; wa.off0 = 0; wa.off1 = 1; wa.sb.u1[0] = du1.p; wa.sb.u2[0] = du2.p; wa.ctl = ctl.p; wa.tab = h->tv.tab;
    wa.wx = dwx.p; wa.wy = dwy.p; wa.rho = drho.p; wa.g = g;
    DBuf dgx, dgy;
    if (h->P.variant == TF_VARIANT_CUDA) {
        HIPC(h, hipMalloc(&dgx.p, 2 * (size_t)g.plane * sizeof(float))); HIPC(h, hipMalloc(&dgy.p, 2 * (size_t)g.plane * sizeof(float)));
        hipLaunchKernelGGL(k_grad, grid64x4(g, 2), dim3(256), 0, h->stream, fr.p, dgx.p, dgy.p, g);
    }
    launch_warp(h, wa, 1, h->stream, dgx.p, dgy.p);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "k_warp: %s", hipGetErrorString(e));
    if ((rc = dbg_down(h, I1wx, dwx.p, g)) || (rc = dbg_down(h, I1wy, dwy.p, g)) || (rc = dbg_down(h, rho_c, drho.p, g))) return rc;
    return TF_OK;
}

TF_API int tf_dbg_df_blur(tf_handle* h, const float* src, int w, int hgt, float* dst)
{
    if (!h || !src || !dst || w < 1 || hgt < 1) return TF_ERR_INVALID_ARG;
    HIPC(h, hipSetDevice(h->dev));
    const Geom g = make_geom(w, hgt);
    DBuf a, b;
    int rc;
    if ((rc = dbg_up(h, a, src, g)) || (rc = dbg_up(h, b, nullptr, g))) return rc;
    float k0, k1;
    df_gauss3(h->DP.sigma > 0 ? h->DP.sigma : 0.6f, &k0, &k1);
    hipLaunchKernelGGL(k_df_blur, grid64x4(g, 1), dim3(256), 0, h->stream, a.p, b.p, g, k0, k1);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "k_df_blur: %s", hipGetErrorString(e));
    return dbg_down(h, dst, b.p, g);
}

// level `level` of DeepFlow's pyramid of one frame, through the kernels and the level table df_solve_resident uses
TF_API int tf_dbg_df_pyramid(tf_handle* h, const void* frame, int is_f32, int H, int W, int level, float* out, int* ow, int* oh)
{
    if (!h || !frame || !ow || !oh || H < 1 || W < 1 || level < 0) return TF_ERR_INVALID_ARG;
    if (h->P.algo != TF_ALGO_DEEPFLOW) return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_df_pyramid needs a handle from tf_create_deepflow");
    std::vector<Geom> lv(DF_MAXLEV);
    const int nlev = df_levels(h->DP, H, W, lv.data());
    if (level >= nlev) return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_df_pyramid: level %d of a pyramid of %d", level, nlev);
    *ow = lv[level].w; *oh = lv[level].h;
    if (!out) return TF_OK;
    HIPC(h, hipSetDevice(h->dev));
    const Geom g0 = lv[0];
    const size_t bytes = (size_t)H * W * (is_f32 ? sizeof(float) : 1);
    DevBuf<uint8_t> din;
    HIPC(h, hipMalloc(&din.p, bytes));
    HIPC(h, hipMemcpyAsync(din.p, frame, bytes, hipMemcpyHostToDevice, h->stream));
    DBuf tmp, cur;
    int rc;
    if ((rc = dbg_up(h, tmp, nullptr, g0)) || (rc = dbg_up(h, cur, nullptr, g0))) return rc;
    float k0, k1;
    df_gauss3(h->DP.sigma, &k0, &k1);
    if (is_f32) hipLaunchKernelGGL(k_f32_to_level0, dim3((g0.w + 255) / 256, g0.h, 1), dim3(256), 0, h->stream, (const float*)din.p, tmp.p, g0, 0);
    else hipLaunchKernelGGL(k_u8_to_f32, dim3((g0.w + 255) / 256, g0.h, 1), dim3(256), 0, h->stream, din.p, tmp.p, g0);
    hipLaunchKernelGGL(k_df_blur, grid64x4(g0, 1), dim3(256), 0, h->stream, tmp.p, cur.p, g0, k0, k1);
    for (int l = 1; l <= level; ++l) {
        const Geom gs = lv[l - 1], gd = lv[l];
        DBuf nxt;
        if ((rc = dbg_up(h, nxt, nullptr, gd))) return rc;
        const double sx = 1.0 / ((double)gd.w / gs.w), sy = 1.0 / ((double)gd.h / gs.h);
        hipLaunchKernelGGL(k_pyr_down, grid64x4(gd, 1), dim3(256), 0, h->stream, cur.p, gs, nxt.p, gd, sx, sy);
        HIPC(h, hipStreamSynchronize(h->stream));
        std::swap(cur.p, nxt.p);
    }
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "deepflow pyramid: %s", hipGetErrorString(e));
    return dbg_down(h, out, cur.p, lv[level]);
}

// the flow hand-down of a DeepFlow solve, one level to the next finer one: k_df_up on host planes (u, v) of sw x sh -> dw x dh
TF_API int tf_dbg_df_up(tf_handle* h, const float* u, const float* v, int sw, int sh, float* ou, float* ov, int dw, int dh)
{
    if (!h || !u || !v || !ou || !ov || sw < 1 || sh < 1 || dw < 1 || dh < 1) return TF_ERR_INVALID_ARG;
    if (h->P.algo != TF_ALGO_DEEPFLOW) return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_df_up needs a handle from tf_create_deepflow");
    HIPC(h, hipSetDevice(h->dev));
    const Geom g = make_geom(sw, sh), gd = make_geom(dw, dh);
    DBuf su, sv, du, dv;
    int rc;
    if ((rc = dbg_up(h, su, u, g)) || (rc = dbg_up(h, sv, v, g)) || (rc = dbg_up(h, du, nullptr, gd)) || (rc = dbg_up(h, dv, nullptr, gd))) return rc;
    DfBufs d = {};
    const int cur = 0;
    d.avg = su.p; d.Iz = sv.p; d.Wu[cur ^ 1] = du.p; d.Wv[cur ^ 1] = dv.p;
    const float mul = 1.0f / h->DP.downscale_factor;
    const double sx = 1.0 / ((double)gd.w / g.w), sy = 1.0 / ((double)gd.h / g.h);
    hipLaunchKernelGGL(k_df_up, grid64x4(gd, 1), dim3(256), 0, h->stream, d, cur, g, gd, sx, sy, mul);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "k_df_up: %s", hipGetErrorString(e));
    if ((rc = dbg_down(h, ou, du.p, gd))) return rc;
    return dbg_down(h, ov, dv.p, gd);
}

TF_API int tf_dbg_f16_round(tf_handle* h, const float* in, size_t n, float scale, uint16_t* out)
{
    if (!h || !in || !out || n < 1) return TF_ERR_INVALID_ARG;
    if (n > ((size_t)1 << 30)) return fail(h, TF_ERR_UNSUPPORTED, "tf_dbg_f16_round: at most 2^30 values");
    HIPC(h, hipSetDevice(h->dev));
    DBuf a, b;
    HIPC(h, hipMalloc(&a.p, n * sizeof(float)));
    HIPC(h, hipMalloc(&b.p, (n + 1) / 2 * sizeof(float)));
    HIPC(h, hipMemcpyAsync(a.p, in, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_dbg_f16_round, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, a.p, n, scale, (uint16_t*)b.p);
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(out, b.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "k_dbg_f16_round: %s", hipGetErrorString(e));
    return TF_OK;
}

// what tf_otsu_masks knows of each frame's luma before it labels anything: otsu_luma_stats (teeflow_masks_host.hip.h) on the caller's frames
TF_API int tf_dbg_luma_stats(tf_handle* h, const uint8_t* rgb, int N, int H, int W, double* minmax_out, uint32_t* hist_out, double* thr_out)
{
    if (!h || !rgb || !minmax_out || !hist_out || !thr_out || N < 1 || H < 1 || W < 1) return TF_ERR_INVALID_ARG;
    if ((size_t)H * W > 0x7fffffffu || N > 65535) return TF_ERR_UNSUPPORTED;   // (frames are a grid dimension, as in tf_otsu_masks)
    HIPC(h, hipSetDevice(h->dev));
    const size_t HW = (size_t)H * W, hist_bytes = (size_t)N * otsu::NBINS * sizeof(uint32_t);
    DevBuf<uint8_t> drgb; DevBuf<u64> mm; DevBuf<uint32_t> hist; DevBuf<double> thr;
    HIPC(h, hipMalloc(&drgb.p, (size_t)N * HW * 3));
    HIPC(h, hipMalloc(&mm.p, (size_t)N * 2 * sizeof(u64)));
    HIPC(h, hipMalloc(&hist.p, hist_bytes));
    HIPC(h, hipMalloc(&thr.p, (size_t)N * sizeof(double)));
    const std::vector<u64> init = minmax_seed((size_t)N);
    HIPC(h, hipMemcpyAsync(drgb.p, rgb, (size_t)N * HW * 3, hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(mm.p, init.data(), init.size() * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(hist.p, 0, hist_bytes, h->stream));
    HIPC(h, hipMemsetAsync(thr.p, 0, (size_t)N * sizeof(double), h->stream));
    otsu_luma_stats(drgb.p, N, HW, mm.p, hist.p, thr.p, h->stream);
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(minmax_out, mm.p, (size_t)N * 2 * sizeof(u64), hipMemcpyDeviceToHost, h->stream));   // (the doubles' own bits)
    HIPC(h, hipMemcpyAsync(hist_out, hist.p, hist_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(thr_out, thr.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "tf_dbg_luma_stats: %s", hipGetErrorString(e));
    return TF_OK;
}

TF_API int tf_dbg_df_refine(tf_handle* h, const float* I0, const float* I1, int w, int hgt, float* u, float* v)
{
    if (!h || !I0 || !I1 || !u || !v || w < 1 || hgt < 1) return TF_ERR_INVALID_ARG;
    if (h->P.algo != TF_ALGO_DEEPFLOW) return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_df_refine needs a handle from tf_create_deepflow");
    HIPC(h, hipSetDevice(h->dev));
    const Geom g = make_geom(w, hgt);
    DBuf fr, planes;
    int rc = dbg_up2(h, fr, I0, I1, g);
    if (rc) return rc;
    HIPC(h, hipMalloc(&planes.p, DF_PLANES * (size_t)g.plane * sizeof(float)));
    HIPC(h, hipMemsetAsync(planes.p, 0, DF_PLANES * (size_t)g.plane * sizeof(float), h->stream));
    const DfBufs saved = h->df.bufs;
    df_carve(h->df.bufs, planes.p, (size_t)g.plane);
    hipError_t e = hipMemcpy2DAsync(h->df.bufs.Wu[0], (size_t)g.pitch * 4, u, (size_t)w * 4, (size_t)w * 4, hgt, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(h->df.bufs.Wv[0], (size_t)g.pitch * 4, v, (size_t)w * 4, (size_t)w * 4, hgt, hipMemcpyHostToDevice, h->stream);
    CoopClaim claim(h->dev);
    h->coop.share = claim.ok ? h->num_cus : 0;
    rc = h->coop.ensure(h);
    if (rc) { h->df.bufs = saved; return rc; }
    if (e == hipSuccess) {
        rc = df_refine_level(h, fr.p, 0, 1, g, 0, 1, h->stream);
        e = hipStreamSynchronize(h->stream);
        bool aborted = false;
        if (e == hipSuccess && !rc) rc = h->coop.aborted(h, &aborted);
        if (!rc && aborted) rc = fail(h, TF_ERR_HIP, "deepflow refine: the co-resident SOR launch gave up waiting for its neighbours");
    }
    if (e != hipSuccess) rc = fail(h, TF_ERR_HIP, "deepflow refine: %s", hipGetErrorString(e));
    if (!rc) rc = dbg_down(h, u, h->df.bufs.avg, g);
    if (!rc) rc = dbg_down(h, v, h->df.bufs.Iz, g);
    h->df.bufs = saved;
    return rc;
}

TF_API int tf_dbg_median(tf_handle* h, const float* src, int w, int hgt, int ksize, float* dst)
{
    if (!h || !src || !dst || w < 1 || hgt < 1 || (ksize != 3 && ksize != 5)) return TF_ERR_INVALID_ARG;
    HIPC(h, hipSetDevice(h->dev));
    const Geom g = make_geom(w, hgt);
    DBuf a0, a1, b0, b1;
    int rc;
    if ((rc = dbg_up(h, a0, src, g)) || (rc = dbg_up(h, a1, nullptr, g)) || (rc = dbg_up(h, b0, src, g)) || (rc = dbg_up(h, b1, nullptr, g))) return rc;
    DevBuf<PairCtl> ctl;
    HIPC(h, hipMalloc(&ctl.p, sizeof(PairCtl)));
    HIPC(h, hipMemsetAsync(ctl.p, 0, sizeof(PairCtl), h->stream));
    MedArgs ma = {};
    ma.sb.u1[0] = a0.p; ma.sb.u1[1] = a1.p; ma.sb.u2[0] = b0.p; ma.sb.u2[1] = b1.p;
    ma.ctl = ctl.p; ma.err = nullptr; ma.errstride = 0; ma.it = 0; ma.thr_q = 0; ma.utog = 0; ma.g = g;
    ma.total = 1; ma.step = iter_step(h, false, h->P.inner_iterations);   // the engine's skip test; at it = 0 neither form reads `err`
    const dim3 gm((g.w + 63) / 64, (g.h + 15) / 16, 2);
    if (ksize == 5) hipLaunchKernelGGL(k_median<5>, gm, dim3(256), 0, h->stream, ma);
    else hipLaunchKernelGGL(k_median<3>, gm, dim3(256), 0, h->stream, ma);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "k_median: %s", hipGetErrorString(e));
    return dbg_down(h, dst, a1.p, g);
}

TF_API int tf_dbg_iterate(tf_handle* h, const float* I1wx, const float* I1wy, const float* rho_c,
                          float* u1, float* u2, float* p11, float* p12, float* p21, float* p22,
                          int w, int hgt, int nsteps, int p_is_zero, unsigned long long* err_q)
{
    if (!h || !I1wx || !I1wy || !rho_c || !u1 || !u2 || !p11 || !p12 || !p21 || !p22 || w < 1 || hgt < 1 || nsteps < 0)
        return TF_ERR_INVALID_ARG;
    HIPC(h, hipSetDevice(h->dev));
    const Geom g = make_geom(w, hgt);
    DBuf cx, cy, cr, s[12];
    int rc;
    if ((rc = dbg_up(h, cx, I1wx, g)) || (rc = dbg_up(h, cy, I1wy, g)) || (rc = dbg_up(h, cr, rho_c, g))) return rc;
    float* hostp[6] = {u1, u2, p11, p12, p21, p22};
    for (int k = 0; k < 6; ++k) {
        if ((rc = dbg_up(h, s[2 * k], hostp[k], g)) || (rc = dbg_up(h, s[2 * k + 1], nullptr, g))) return rc;
    }
    DevBuf<PairCtl> ctl; DevBuf<u64> errs;
    HIPC(h, hipMalloc(&ctl.p, sizeof(PairCtl)));
    HIPC(h, hipMemsetAsync(ctl.p, 0, sizeof(PairCtl), h->stream));
    HIPC(h, hipMalloc(&errs.p, (size_t)(nsteps + 1) * sizeof(u64)));
    HIPC(h, hipMemsetAsync(errs.p, 0, (size_t)(nsteps + 1) * sizeof(u64), h->stream));
    Iter2Args A = {};
    IterArgs& ia = A.a;
    ia.wx = cx.p; ia.wy = cy.p; ia.rho = cr.p;
    for (int k = 0; k < 2; ++k) {
        ia.sb.u1[k] = s[0 + k].p; ia.sb.u2[k] = s[2 + k].p; ia.sb.p11[k] = s[4 + k].p;
        ia.sb.p12[k] = s[6 + k].p; ia.sb.p21[k] = s[8 + k].p; ia.sb.p22[k] = s[10 + k].p;
    }
    ia.ctl = ctl.p; ia.err = errs.p; ia.errstride = nsteps + 1; ia.thr_q = -1.0; ia.g = g; ia.host_slot = nullptr; ia.B = 1;
    ia.l_t = (float)(h->P.lambda * h->P.theta); ia.theta = (float)h->P.theta; ia.taut = (float)(h->P.tau / h->P.theta);
    const int step = iter_step(h, false, nsteps);     // (ia.variant = 0: these launches run the CPU form whatever the handle's variant)
    A.total = nsteps;
    int launches = 0;
    // run_stage's loop without its last launch: thr_q < 0 keeps the pair in NORMAL mode, so there is never an iteration to REPLAY
    for (int it = 0; it < nsteps; it += step, ++launches) {
        ia.it = it; ia.utog = ia.ptog = launches; ia.pzero = (p_is_zero && it == 0) ? 1 : 0;
        launch_iter(h, A, step, 1, h->stream);
    }
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && err_q && nsteps > 0) {
        e = hipMemcpyAsync(err_q, errs.p, (size_t)nsteps * sizeof(u64), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "k_iter: %s", hipGetErrorString(e));
    const int cur = launches & 1;
    for (int k = 0; k < 6; ++k)
        if ((rc = dbg_down(h, hostp[k], s[2 * k + cur].p, g))) return rc;
    return TF_OK;
}

// One (level, warp) stage without its warp, for B pairs on the caller's planes: run_stage_loop (teeflow_tvl1_host.hip.h), the loop a
// solve runs -- medians, tvl1_iter launches in the engine's current form, the active-pair reports that end the stage early -- and
// k_stage_end.  Pair b's planes sit at b * splane of the geometry, as in a solve; its state comes back from the ping-pong halves its
// PairCtl names after k_stage_end.
TF_API int tf_dbg_stage(tf_handle* h, const float* I1wx, const float* I1wy, const float* rho_c,
                        float* u1, float* u2, float* p11, float* p12, float* p21, float* p22,
                        int B, int w, int hgt, int inner, int outer, int ksize, float thr, int variant, int p_is_zero,
                        unsigned long long* err_q, int* iters)
{
    if (!h || !I1wx || !I1wy || !rho_c || !u1 || !u2 || !p11 || !p12 || !p21 || !p22 || !err_q || !iters) return TF_ERR_INVALID_ARG;
    if (B < 1 || B > 4096) return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_stage: B must be in [1,4096], got %d", B);
    if (w < 1 || hgt < 1 || inner < 1 || outer < 1 || (long long)inner * outer > 100000)
        return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_stage: bad size %d x %d or iteration counts %d / %d", w, hgt, inner, outer);
    if (ksize != 0 && ksize != 3 && ksize != 5) return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_stage: ksize must be 0, 3 or 5, got %d", ksize);
    if (variant != TF_VARIANT_CPU && variant != TF_VARIANT_CUDA) return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_stage: variant must be 0 or 1, got %d", variant);
    if (variant == TF_VARIANT_CUDA && (inner * outer) % 2 != 0)
        return fail(h, TF_ERR_INVALID_ARG, "tf_dbg_stage: TF_VARIANT_CUDA needs an even iteration count (inner*outer), got %d", inner * outer);
    HIPC(h, hipSetDevice(h->dev));
    const Geom g = make_geom(w, hgt);
    const int total = inner * outer, errstride = total + 1;
    const size_t pl = (size_t)B * (size_t)g.splane * sizeof(float), rowb = (size_t)w * 4, pitchb = (size_t)g.pitch * 4;
    DBuf cst[3], st[12];
    // [B][h][w] -> B planes of h pitched rows, one after the other (splane == pitch * h); the padding and the second halves are zero
    const auto up = [&](DBuf& d, const float* src) -> int {
        HIPC(h, hipMalloc(&d.p, pl));
        HIPC(h, hipMemsetAsync(d.p, 0, pl, h->stream));
        if (src) HIPC(h, hipMemcpy2DAsync(d.p, pitchb, src, rowb, rowb, (size_t)B * hgt, hipMemcpyHostToDevice, h->stream));
        return TF_OK;
    };
    const float* hostc[3] = {I1wx, I1wy, rho_c};
    float* hostp[6] = {u1, u2, p11, p12, p21, p22};
    int rc;
    for (int k = 0; k < 3; ++k) if ((rc = up(cst[k], hostc[k]))) return rc;
    for (int k = 0; k < 6; ++k) if ((rc = up(st[2 * k], hostp[k])) || (rc = up(st[2 * k + 1], nullptr))) return rc;
    DevBuf<PairCtl> ctl; DevBuf<u64> errs; DevBuf<int> dit;
    HIPC(h, hipMalloc(&ctl.p, (size_t)B * sizeof(PairCtl)));
    HIPC(h, hipMemsetAsync(ctl.p, 0, (size_t)B * sizeof(PairCtl), h->stream));
    HIPC(h, hipMalloc(&errs.p, (size_t)B * errstride * sizeof(u64)));
    HIPC(h, hipMalloc(&dit.p, (size_t)B * 2 * sizeof(int)));

    StageRun r;
    r.wx = cst[0].p; r.wy = cst[1].p; r.rho = cst[2].p;
    for (int k = 0; k < 2; ++k) {
        r.sb.u1[k] = st[0 + k].p; r.sb.u2[k] = st[2 + k].p; r.sb.p11[k] = st[4 + k].p;
        r.sb.p12[k] = st[6 + k].p; r.sb.p21[k] = st[8 + k].p; r.sb.p22[k] = st[10 + k].p;
    }
    r.ctl = ctl.p; r.errs = errs.p; r.errstride = errstride; r.iters_dev = dit.p; r.g = g;
    r.inner = inner; r.total = total; r.ksize = ksize; r.variant = variant;
    r.thr_f = thr; r.thr_d = (double)thr;
    r.l_t = (float)(h->P.lambda * h->P.theta); r.theta = (float)h->P.theta; r.taut = (float)(h->P.tau / h->P.theta);
    r.pzero = p_is_zero ? 1 : 0;
    r.l = 0; r.wi = 0; r.nlev = 1; r.warps = 1;
    if ((rc = run_stage_loop(h, r, B))) return rc;

    std::vector<PairCtl> hc((size_t)B);
    hipError_t e = hipMemcpyAsync(hc.data(), ctl.p, (size_t)B * sizeof(PairCtl), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(err_q, errs.p, (size_t)B * errstride * sizeof(u64), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(iters, dit.p, (size_t)B * 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, TF_ERR_HIP, "tf_dbg_stage: %s", hipGetErrorString(e));
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < 6; ++k) {
            const int half = (k < 2 ? hc[b].ubase : hc[b].pbase) & 1;
            HIPC(h, hipMemcpy2DAsync(hostp[k] + (size_t)b * hgt * w, rowb, st[2 * k + half].p + (size_t)b * g.splane, pitchb, rowb, hgt,
                                     hipMemcpyDeviceToHost, h->stream));
        }
    HIPC(h, hipStreamSynchronize(h->stream));
    return TF_OK;
}
