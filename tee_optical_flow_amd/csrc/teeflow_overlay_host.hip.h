// The two overlay renderers: tf_radlong_overlay, which reads the resident rad/long planes, and tf_magnitude_overlay, which makes its field from the flow itself.
// Relies on teeflow_scratch.hip.h, on dispatch_param of teeflow_analysis_host.hip.h and on the kernels of teeflow_overlay.hip.h and teeflow_magoverlay.hip.h.

static_assert(TF_ECHO_F16 == ovl::ECHO_F16 && TF_ECHO_U8 == ovl::ECHO_U8, "echo kinds of the header and the kernel differ");

namespace {
// tf_radlong_overlay: the indices (2 B per pixel of the study, an eighth of the resident planes) are made for all frames at once, since
// m2 needs every frame's; the echo upload and the output (eb + 6 B per pixel) go through in chunks of as many frames as fit in
// MASK_CHUNK_BYTES.  A study of one chunk uploads its echo once; a longer one uploads it a second time for the compose pass.
template <int KIND>
int radlong_overlay(tf_handle* h, const Src& echo, const double* lut_rad, const double* lut_long, uint8_t* out, double* info)
{
    using namespace ovl;
    using ET = typename Echo<KIND>::T;
    const int n = h->anN, H = h->anH, W = h->anW;
    const size_t HW = (size_t)H * W, tot = (size_t)n * HW, eb = sizeof(ET);
    const int nf = chunk_frames(HW * (eb + 6), n, (size_t)n, h->overlay_chunk_kib > 0 ? (size_t)h->overlay_chunk_kib << 10 : MASK_CHUNK_BYTES);
    const size_t out_dwords = ((size_t)nf * HW * 2 + 3) / 4 * 3;      // 3 dwords per run of 4 slots, whole runs: what k_ov_compose stores
    HIPC(h, hipSetDevice(h->dev));
    // meta: [0, 8) half bits, [8, 16) echo max bits + bad flag, [16, 80) used bitsets [2][8], [128, 128 + 12288) colour terms [2][256][3] f64
    Pre pre(h);
    auto* didx = pre.get<uint16_t>(tf_handle::PRE_OV_IDX, tot);
    auto* uecho = echo.dev ? nullptr : pre.get<ET>(tf_handle::PRE_OV_ECHO, (size_t)nf * HW);
    auto* dout = pre.get<unsigned>(tf_handle::PRE_OV_OUT, out_dwords);
    auto* meta = pre.get<uint8_t>(tf_handle::PRE_OV_META, 128 + 2 * 256 * 3 * sizeof(double));
    if (pre.rc) return pre.rc;
    u64* dhalf = (u64*)meta;
    unsigned* demax = (unsigned*)(meta + 8);
    unsigned* dused = (unsigned*)(meta + 16);
    double* dcol = (double*)(meta + 128);
    const hipStream_t s = h->stream;
    const dim3 blk(256);
    auto grid = [](size_t work, size_t cap) { const size_t g = (work + 255) / 256; return dim3((unsigned)(g < cap ? g : cap)); };
    HIPC(h, hipMemsetAsync(meta, 0, 128, s));
    hipLaunchKernelGGL(k_ov_half, grid(HW, 256), blk, 0, s, h->an_rad, HW, dhalf);
    hipLaunchKernelGGL(k_ov_index, grid(tot, 2048), blk, 0, s, h->an_rad, h->an_lon, tot, dhalf, didx, dused);
    HIPC(h, hipGetLastError());
    const uint8_t* de = nullptr;                                      // the current chunk's echo
    for (int f0 = 0; f0 < n; f0 += nf) {
        const size_t c = (size_t)std::min(nf, n - f0) * HW;
        const int rc = src_to_device(h, echo, (size_t)f0 * HW * eb, c * eb, uecho, &de);
        if (rc) return rc;
        hipLaunchKernelGGL(k_ov_echo<KIND>, grid(c, 1024), blk, 0, s, (const ET*)de, c, demax);
        HIPC(h, hipGetLastError());
    }
    struct { u64 half; unsigned emax, bad; unsigned used[16]; } m;
    static_assert(sizeof m == 80, "layout of the overlay's meta words");
    HIPC(h, hipMemcpyAsync(&m, meta, sizeof m, hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));
    union { u64 u; double d; } hb; hb.u = m.half;
    union { unsigned u; float f; } em; em.u = m.emax;
    const double half = hb.d, emax = (double)em.f;
    if (m.bad) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay: the echo holds a negative or non-finite value");
    if (emax == 0.0) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay: the echo's maximum is 0");
    if (!std::isfinite(half - (-half))) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay: the norm's range 2 * %g overflows", half);
    double m2 = 0.0;
    for (int c = 0; c < 2; ++c)
        for (int j = 0; j < 256; ++j)
            if ((m.used[8 * c + (j >> 5)] >> (j & 31)) & 1u)
                for (int ch = 0; ch < 3; ++ch) { const double v = (c ? lut_long : lut_rad)[3 * j + ch]; m2 = v > m2 ? v : m2; }
    if (m2 == 0.0) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay: every colour used is black (the colour maximum is 0)");
    std::vector<double> col(2 * 256 * 3);
    for (int c = 0; c < 2; ++c)
        for (int j = 0; j < 256 * 3; ++j) col[(size_t)c * 768 + j] = 0.5 * ((c ? lut_long : lut_rad)[j] / m2);
    HIPC(h, hipMemcpyAsync(dcol, col.data(), col.size() * sizeof(double), hipMemcpyHostToDevice, s));
    for (int f0 = 0; f0 < n; f0 += nf) {
        const int nc = std::min(nf, n - f0);
        const size_t c = (size_t)nc * HW, slots = 2 * c;                                // nc <= nf: the runs of `slots` fit out_dwords
        if (n > nf) { const int rc = src_to_device(h, echo, (size_t)f0 * HW * eb, c * eb, uecho, &de); if (rc) return rc; }
        hipLaunchKernelGGL(k_ov_compose<KIND>, dim3((unsigned)((slots + 1023) / 1024)), blk, 0, s, didx + (size_t)f0 * HW, (const ET*)de, emax, dcol,
                           (size_t)nc * H, W, dout);
        HIPC(h, hipGetLastError());
        HIPC(h, hipMemcpyAsync(out + (size_t)f0 * HW * 6, dout, c * 6, hipMemcpyDeviceToHost, s));
    }
    HIPC(h, hipStreamSynchronize(s));
    info[0] = half; info[1] = emax; info[2] = m2;
    return TF_OK;
}

// what tf_radlong_overlay checks of its tables and of the resident planes (h and the tables are not null)
int check_overlay(tf_handle* h, const double* lut_rad, const double* lut_long)
{
    for (int j = 0; j < 256 * 3; ++j)
        if (!(lut_rad[j] >= 0.0 && std::isfinite(lut_rad[j]) && lut_long[j] >= 0.0 && std::isfinite(lut_long[j])))
            return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay: a colormap entry is negative or not finite");
    if (h->anN < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay needs a preceding tf_radlong_project or tf_radlong_project_param");
    if (h->an_polar) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay: the handle's last projection was tf_polar_project_param, not a rad/long one");
    if (!h->an_finite) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_overlay: the rad/long planes hold NaN or inf");
    if ((size_t)h->anH * h->anW > 0x7fffffffu / 8) return fail(h, TF_ERR_UNSUPPORTED, "tf_radlong_overlay: at most 2^28 - 1 pixels per frame");
    return TF_OK;
}
}  // namespace

TF_API int tf_radlong_overlay(tf_handle* h, const void* echo, int echo_kind, const double* lut_rad, const double* lut_long, uint8_t* out,
                              double* info)
{
    if (!h || !echo || !lut_rad || !lut_long || !out || !info || (echo_kind != TF_ECHO_F16 && echo_kind != TF_ECHO_U8)) return TF_ERR_INVALID_ARG;
    if (int rc = check_overlay(h, lut_rad, lut_long)) return rc;
    return finish_host_call(h, echo_kind == TF_ECHO_F16 ? radlong_overlay<ovl::ECHO_F16>(h, Src::on_host(echo), lut_rad, lut_long, out, info)
                                                        : radlong_overlay<ovl::ECHO_U8>(h, Src::on_host(echo), lut_rad, lut_long, out, info));
}

namespace {
// tf_magnitude_overlay: the flow and the mask of all N frames are on the device for the whole call (uploaded into the projections'
// upload scratch, or read where a held study keeps them); the indices (1 B per pixel of the n frames rendered), the per-frame words and
// colour terms (64 B + 6 KiB per frame) are made for all frames at once; the echo upload and the output (eb + 3 B per pixel) go
// through in chunks of as many frames as fit in MASK_CHUNK_BYTES (tests: the overlay_chunk_kib knob).  A study of one chunk uploads
// its echo once; a longer one uploads it a second time for the compose pass.  The host waits once between the passes, for the
// extrema and the flags that decide the refusals; the colour maxima are made on the device (k_mo_scale).  Nothing here touches the
// resident analysis planes.
template <int KIND>
int magnitude_overlay(tf_handle* h, const Src& flow, int f16, int N, int n, int H, int W, const Src& mask, int C, int param, double spacing,
                      int grad_f64, int norm_f64, const Src& echo, const double* lut, uint8_t* out, double* info, double* frame_info)
{
    using namespace mov;
    using ET = typename ovl::Echo<KIND>::T;
    const size_t HW = (size_t)H * W, eb = sizeof(ET);
    const size_t flow_bytes = (size_t)N * HW * 2 * (f16 ? 2 : 4);
    const int nf = chunk_frames(HW * (eb + 3), n, (size_t)n, h->overlay_chunk_kib > 0 ? (size_t)h->overlay_chunk_kib << 10 : MASK_CHUNK_BYTES);
    const size_t out_dwords = ((size_t)nf * HW + 3) / 4 * 3;          // 3 dwords per run of 4 slots, whole runs: what k_mo_compose stores
    HIPC(h, hipSetDevice(h->dev));
    // meta: [0, 16) the study's Range, [64, 64 + 6144) the table, then FrameMeta [n], then the colour terms [n][256][3] f64
    const size_t off_lut = 64, off_fm = off_lut + 768 * sizeof(double), off_col = off_fm + (size_t)n * sizeof(FrameMeta);
    Pre pre(h);
    uint8_t* uflow = flow.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_AN_FLOW, flow_bytes);
    uint8_t* umask = mask.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_AN_MASK, (size_t)N * HW * C);
    auto* didx = pre.get<uint8_t>(tf_handle::PRE_MO_IDX, (size_t)n * HW);
    auto* uecho = echo.dev ? nullptr : pre.get<ET>(tf_handle::PRE_MO_ECHO, (size_t)nf * HW);
    auto* dout = pre.get<unsigned>(tf_handle::PRE_MO_OUT, out_dwords);
    auto* meta = pre.get<uint8_t>(tf_handle::PRE_MO_META, off_col + (size_t)n * 768 * sizeof(double));
    if (pre.rc) return pre.rc;
    Range* drng = (Range*)meta;
    double* dlut = (double*)(meta + off_lut);
    FrameMeta* dfm = (FrameMeta*)(meta + off_fm);
    double* dcol = (double*)(meta + off_col);
    const hipStream_t s = h->stream;
    const dim3 blk(256);
    const uint8_t* dflow = nullptr; const uint8_t* dmask = nullptr;
    int rc;
    if ((rc = src_to_device(h, flow, 0, flow_bytes, uflow, &dflow))) return rc;
    if ((rc = src_to_device(h, mask, 0, (size_t)N * HW * C, umask, &dmask))) return rc;
    const Range seed{~0u, 0u, 0u, 0u};
    HIPC(h, hipMemcpyAsync(drng, &seed, sizeof seed, hipMemcpyHostToDevice, s));
    HIPC(h, hipMemcpyAsync(dlut, lut, 768 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPC(h, hipMemsetAsync(dfm, 0, (size_t)n * sizeof(FrameMeta), s));
    const unsigned gpx = (unsigned)((HW + 255) / 256);
    dispatch_param(param, f16, grad_f64, [&](auto pc, auto ft, auto gt) {
        using FT = decltype(ft);
        hipLaunchKernelGGL((k_mo_range<decltype(pc)::value, FT, decltype(gt)>), dim3(gpx < 256 ? gpx : 256, N), blk, 0, s, (const FT*)dflow, N, dmask, C,
                           spacing, HW, drng);
        hipLaunchKernelGGL((k_mo_index<decltype(pc)::value, FT, decltype(gt)>), dim3(gpx < 128 ? gpx : 128, n), blk, 0, s, (const FT*)dflow, N, dmask, C,
                           spacing, HW, drng, norm_f64, didx, dfm);
    });
    HIPC(h, hipGetLastError());
    const uint8_t* de = nullptr;                                      // the current chunk's echo
    for (int f0 = 0; f0 < n; f0 += nf) {
        const int nc = std::min(nf, n - f0);
        if ((rc = src_to_device(h, echo, (size_t)f0 * HW * eb, (size_t)nc * HW * eb, uecho, &de))) return rc;
        hipLaunchKernelGGL(k_mo_echo<KIND>, dim3(gpx < 64 ? gpx : 64, nc), blk, 0, s, (const ET*)de, HW, dfm + f0);
        HIPC(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_mo_scale, dim3(n), blk, 0, s, dlut, dfm, dcol);
    HIPC(h, hipGetLastError());
    Range r;
    std::vector<FrameMeta> fm((size_t)n);
    HIPC(h, hipMemcpyAsync(&r, drng, sizeof r, hipMemcpyDeviceToHost, s));
    HIPC(h, hipMemcpyAsync(fm.data(), dfm, fm.size() * sizeof(FrameMeta), hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));                                 // (`seed` leaves scope after this, too)
    if (r.bad) return fail(h, TF_ERR_INVALID_ARG, "tf_magnitude_overlay: the magnitude holds NaN or inf");
    for (int f = 0; f < n; ++f)
        if (fm[f].ebad) return fail(h, TF_ERR_INVALID_ARG, "tf_magnitude_overlay: the echo holds a negative or non-finite value");
    for (int f0 = 0; f0 < n; f0 += nf) {
        const int nc = std::min(nf, n - f0);
        const size_t slots = (size_t)nc * HW;                         // nc <= nf: the runs of `slots` fit out_dwords
        if (n > nf && (rc = src_to_device(h, echo, (size_t)f0 * HW * eb, slots * eb, uecho, &de))) return rc;
        hipLaunchKernelGGL(k_mo_compose<KIND>, dim3((unsigned)((slots + 1023) / 1024)), blk, 0, s, didx + (size_t)f0 * HW, (const ET*)de, dfm + f0,
                           dcol + (size_t)f0 * 768, HW, slots, dout);
        HIPC(h, hipGetLastError());
        HIPC(h, hipMemcpyAsync(out + (size_t)f0 * HW * 3, dout, slots * 3, hipMemcpyDeviceToHost, s));
    }
    HIPC(h, hipStreamSynchronize(s));
    union { unsigned u; float f; } c;
    c.u = r.lo; info[0] = (double)c.f;
    c.u = r.hi; info[1] = (double)c.f;
    for (int f = 0; f < n; ++f) { c.u = fm[f].emax; frame_info[2 * f] = (double)c.f; frame_info[2 * f + 1] = fm[f].cmax; }
    return TF_OK;
}

// what tf_magnitude_overlay and its held twin check of the table and the frame size (h and lut are not null)
int check_magnitude_overlay(tf_handle* h, const char* who, int N, int H, int W, const double* lut)
{
    for (int j = 0; j < 256 * 3; ++j)
        if (!(lut[j] >= 0.0 && std::isfinite(lut[j]))) return fail(h, TF_ERR_INVALID_ARG, "%s: a colormap entry is negative or not finite", who);
    if ((size_t)H * W > 0x7fffffffu / 8) return fail(h, TF_ERR_UNSUPPORTED, "%s: at most 2^28 - 1 pixels per frame", who);
    if (N > 65535) return fail(h, TF_ERR_UNSUPPORTED, "%s: at most 65535 frames", who);                    // frames are grid.y
    return TF_OK;
}
}  // namespace

TF_API int tf_magnitude_overlay(tf_handle* h, const void* flow, int flow_is_f16, int N, int n_used, int H, int W, const uint8_t* mask, int mask_C,
                                int param, double spacing, int grad_f64, int norm_f64, const void* echo, int echo_kind, const double* lut,
                                uint8_t* out, double* info, double* frame_info)
{
    if (!h || !flow || !mask || !echo || !lut || !out || !info || !frame_info || N < 1 || n_used < 1 || H < 1 || W < 1 || n_used > N)
        return TF_ERR_INVALID_ARG;
    if ((mask_C != 1 && mask_C != 2) || param < TF_PARAM_VELOCITY || param > TF_PARAM_PWR) return TF_ERR_INVALID_ARG;
    if (echo_kind != TF_ECHO_F16 && echo_kind != TF_ECHO_U8) return TF_ERR_INVALID_ARG;
    if (param != TF_PARAM_VELOCITY && (N < 2 || !std::isfinite(spacing) || spacing == 0.0)) return TF_ERR_INVALID_ARG;   // np.gradient needs 2 frames
    if (int rc = check_magnitude_overlay(h, "tf_magnitude_overlay", N, H, W, lut)) return rc;
    const Src f = Src::on_host(flow), m = Src::on_host(mask), e = Src::on_host(echo);
    const int f16 = flow_is_f16 ? 1 : 0, g64 = grad_f64 ? 1 : 0, n64 = norm_f64 ? 1 : 0;
    return finish_host_call(h, echo_kind == TF_ECHO_F16
        ? magnitude_overlay<ovl::ECHO_F16>(h, f, f16, N, n_used, H, W, m, mask_C, param, spacing, g64, n64, e, lut, out, info, frame_info)
        : magnitude_overlay<ovl::ECHO_U8>(h, f, f16, N, n_used, H, W, m, mask_C, param, spacing, g64, n64, e, lut, out, info, frame_info));
}
