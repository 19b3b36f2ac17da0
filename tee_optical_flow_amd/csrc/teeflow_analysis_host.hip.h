// The analysis session: the rad/long and polar projections of a study's flow into the handle's resident planes (Projection), and what reads the
// planes afterwards, tf_radlong_hist and tf_radlong_select.  Relies on teeflow_scratch.hip.h and on the kernels of teeflow_analysis.hip.h and teeflow_polar.hip.h.

namespace {
// the resident analysis planes hold at least tot doubles each (grown, never shrunk); they are invalid until the caller's projection
// has run (anN = 0)
int grow_an_planes(tf_handle* h, size_t tot)
{
    h->anN = 0;
    if (h->an_cap < tot) {
        HIPC(h, hipStreamSynchronize(h->stream));
        if (h->an_rad) { (void)hipFree(h->an_rad); h->an_rad = nullptr; }
        if (h->an_lon) { (void)hipFree(h->an_lon); h->an_lon = nullptr; }
        h->an_cap = 0;
        HIPC(h, hipMalloc(&h->an_rad, tot * sizeof(double)));
        HIPC(h, hipMalloc(&h->an_lon, tot * sizeof(double)));
        h->an_cap = tot;
    }
    return TF_OK;
}

// What the projections share.  begin(): the resident planes for n frames, the flow and mask uploads, and a meta block whose head
// is the planes' min/max keys [4] at 0 (seeded) and their non-zero counts [n][2] at 32; what follows the head is the caller's, and all
// but the keys starts as zeroes.  end(), after the caller's kernel: keys and counts back to the host, and the handle's bookkeeping.
struct Projection {
    tf_handle* h;
    int n, H, W;
    const size_t npx = (size_t)H * W, tot = (size_t)n * npx;
    const uint8_t* dflow = nullptr; const uint8_t* dmask = nullptr; uint8_t* meta = nullptr;
    u64* mm = nullptr; unsigned long long* cnt = nullptr;
    std::vector<u64> seed = minmax_seed(2);

    // flow: N frames of float16 (f16) or float32 pairs, of which the field `param` of frames [0, n) reads the first nflow;
    // mask: C bytes per pixel of frames [0, n), or C == 0 for a call without masks (tf_radlong_project).  Either is uploaded, or read
    // where it is on the device (Src).
    int begin(const Src& flow, int f16, int N, int param, const Src& mask, int C, int meta_slot, size_t meta_bytes)
    {
        const int nflow = param == RL_PARAM_VELOCITY ? n : (n + 1 < N ? n + 1 : N);   // the gradient of [0, n) reads one frame more
        const size_t flow_bytes = (size_t)nflow * npx * 2 * (f16 ? 2 : 4);
        HIPC(h, hipSetDevice(h->dev));
        int rc = grow_an_planes(h, tot);
        if (rc) return rc;
        Pre pre(h);
        uint8_t* uflow = flow.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_AN_FLOW, flow_bytes);
        uint8_t* umask = C && !mask.dev ? pre.get<uint8_t>(tf_handle::PRE_AN_MASK, tot * C) : nullptr;
        meta = pre.get<uint8_t>(meta_slot, meta_bytes);
        if (pre.rc) return pre.rc;
        mm = (u64*)meta;
        cnt = (unsigned long long*)(meta + 32);
        const hipStream_t s = h->stream;
        if ((rc = src_to_device(h, flow, 0, flow_bytes, uflow, &dflow))) return rc;
        if (C && (rc = src_to_device(h, mask, 0, tot * C, umask, &dmask))) return rc;
        HIPC(h, hipMemcpyAsync(mm, seed.data(), 32, hipMemcpyHostToDevice, s));
        HIPC(h, hipMemsetAsync(cnt, 0, meta_bytes - 32, s));
        return TF_OK;
    }

    // (checks the launches only once the read-backs are queued: a failed one is caught all the same, and finish_host_call drains the
    // stream.  an_finite is written for polar planes too; only tf_radlong_overlay reads it, after it has refused polar planes.)
    int end(double* minmax, long long* nonzero, bool polar)
    {
        u64 mmh[4];
        std::vector<unsigned long long> ch((size_t)n * 2);
        HIPC(h, hipGetLastError());
        HIPC(h, hipMemcpyAsync(mmh, mm, sizeof mmh, hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipMemcpyAsync(ch.data(), cnt, ch.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        for (int j = 0; j < 4; ++j) minmax[j] = f64_unkey(mmh[j]);
        for (size_t i = 0; i < ch.size(); ++i) nonzero[i] = (long long)ch[i];
        h->anN = n; h->anH = H; h->anW = W;
        h->an_polar = polar;
        h->an_finite = std::isfinite(minmax[0]) && std::isfinite(minmax[1]) && std::isfinite(minmax[2]) && std::isfinite(minmax[3]);
        return TF_OK;
    }
};

int radlong_hist(tf_handle* h, int which, const double* edges, int nbins, long long* freq_out)
{
    HIPC(h, hipSetDevice(h->dev));
    const size_t npx = (size_t)h->anH * h->anW, nfreq = (size_t)h->anN * nbins;
    Pre pre(h);
    auto* df = pre.get<unsigned long long>(tf_handle::PRE_AN_HIST, nfreq + nbins + 1);   // counts [anN][nbins], then the edges [nbins + 1] f64
    if (pre.rc) return pre.rc;
    double* de = (double*)(df + nfreq);
    HIPC(h, hipMemcpyAsync(de, edges, (size_t)(nbins + 1) * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(df, 0, nfreq * sizeof(unsigned long long), h->stream));
    const int gx = (int)((npx + 255) / 256);
    hipLaunchKernelGGL(k_radlong_hist, dim3(gx < 256 ? gx : 256, h->anN), dim3(256), 0, h->stream, which ? h->an_lon : h->an_rad, npx, de, nbins, df);
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(freq_out, df, nfreq * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return TF_OK;
}

int radlong_select(tf_handle* h, int which, const long long* ranks, double* values_out)
{
    HIPC(h, hipSetDevice(h->dev));
    const int N = h->anN, NS = N * RL_NSLOT;
    const size_t npx = (size_t)h->anH * h->anW, hist_bytes = (size_t)NS * 65536 * sizeof(unsigned);
    std::vector<int> act((size_t)NS);
    for (int i = 0; i < NS; ++i) act[i] = ranks[i] >= 0;
    // per slot: a histogram of 65536 digits; then the key prefixes u64, the ranks i64 and the active flags i32, [NS] each
    Pre pre(h);
    auto* hist = pre.get<unsigned>(tf_handle::PRE_AN_SEL, (size_t)NS * (65536 + 2 + 2 + 1));
    if (pre.rc) return pre.rc;
    u64* pf = (u64*)(hist + (size_t)NS * 65536);
    long long* rk = (long long*)(pf + NS);
    int* ac = (int*)(rk + NS);
    HIPC(h, hipMemsetAsync(pf, 0, (size_t)NS * sizeof(u64), h->stream));
    HIPC(h, hipMemcpyAsync(rk, ranks, (size_t)NS * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(ac, act.data(), (size_t)NS * sizeof(int), hipMemcpyHostToDevice, h->stream));
    const double* v = which ? h->an_lon : h->an_rad;
    const int gx = (int)((npx + 255) / 256);
    for (int shift = 48; shift >= 0; shift -= 16) {
        HIPC(h, hipMemsetAsync(hist, 0, hist_bytes, h->stream));
        hipLaunchKernelGGL(k_radlong_sel_hist, dim3(gx < 256 ? gx : 256, N), dim3(256), 0, h->stream, v, npx, shift, pf, ac, hist);
        hipLaunchKernelGGL(k_radlong_sel_scan, dim3(NS), dim3(256), 0, h->stream, hist, shift, pf, rk, ac);
    }
    HIPC(h, hipGetLastError());
    std::vector<u64> keys((size_t)NS);
    HIPC(h, hipMemcpyAsync(keys.data(), pf, (size_t)NS * sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < NS; ++i) values_out[i] = act[i] ? f64_unkey(keys[i]) : 0.0;
    return TF_OK;
}
}  // namespace

TF_API int tf_radlong_hist(tf_handle* h, int which, const double* edges, int nbins, long long* freq_out)
{
    if (!h || !edges || !freq_out || nbins < 1 || which < 0 || which > 1) return TF_ERR_INVALID_ARG;
    if (h->anN < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_hist needs a preceding tf_radlong_project");
    return finish_host_call(h, radlong_hist(h, which, edges, nbins, freq_out));
}

TF_API int tf_radlong_select(tf_handle* h, int which, const long long* ranks, double* values_out)
{
    if (!h || !ranks || !values_out || which < 0 || which > 1) return TF_ERR_INVALID_ARG;
    if (h->anN < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_radlong_select needs a preceding tf_radlong_project");
    return finish_host_call(h, radlong_select(h, which, ranks, values_out));
}

namespace {
// calls f(param, flow element, gradient element) with values of the static types that the three run-time codes select: the
// instantiations of k_radlong_project_param and k_polar_project_param
template <typename F>
void dispatch_param(int param, int f16, int grad_f64, F f)
{
    auto with_param = [&](auto p) {
        auto with_flow = [&](auto ft) { grad_f64 ? f(p, ft, double{}) : f(p, ft, float{}); };
        f16 ? with_flow(_Float16{}) : with_flow(float{});
    };
    if (param == RL_PARAM_VELOCITY) with_param(std::integral_constant<int, RL_PARAM_VELOCITY>{});
    else if (param == RL_PARAM_ACCELERATION) with_param(std::integral_constant<int, RL_PARAM_ACCELERATION>{});
    else with_param(std::integral_constant<int, RL_PARAM_PWR>{});
}

// the rad/long calls around their kernel: launch(p, dcent, grid) runs it on the uploads of p and the centroids [n_used][2] at dcent
template <typename Launch>
int radlong_project(tf_handle* h, const Src& flow, int f16, int N, int n_used, int H, int W, const Src& mask, int C, int param,
                    const double* centroids, double* rad_out, double* long_out, double* minmax, long long* nonzero, Launch launch)
{
    Projection p{h, n_used, H, W};                              // meta: the head, then centroids [n_used][2]
    int rc = p.begin(flow, f16, N, param, mask, C, tf_handle::PRE_AN_META, 32 + (size_t)n_used * 32);
    if (rc) return rc;
    const hipStream_t s = h->stream;
    double* dcent = (double*)(p.meta + 32 + (size_t)n_used * 16);
    HIPC(h, hipMemcpyAsync(dcent, centroids, (size_t)n_used * 16, hipMemcpyHostToDevice, s));
    const int gx = (int)((p.npx + 255) / 256);
    launch(p, dcent, dim3(gx < 256 ? gx : 256, n_used));
    if (rad_out) HIPC(h, hipMemcpyAsync(rad_out, h->an_rad, p.tot * sizeof(double), hipMemcpyDeviceToHost, s));
    if (long_out) HIPC(h, hipMemcpyAsync(long_out, h->an_lon, p.tot * sizeof(double), hipMemcpyDeviceToHost, s));
    return p.end(minmax, nonzero, false);
}

int radlong_project_param(tf_handle* h, const Src& flow, int f16, int N, int n_used, int H, int W, const Src& mask, int C, int param,
                          double spacing, int grad_f64, const double* centroids, double* rad_out, double* long_out, double* minmax,
                          long long* nonzero)
{
    return radlong_project(h, flow, f16, N, n_used, H, W, mask, C, param, centroids, rad_out, long_out, minmax, nonzero,
        [&](const Projection& p, const double* dcent, dim3 g) {
            dispatch_param(param, f16, grad_f64, [&](auto pc, auto ft, auto gt) {
                using FT = decltype(ft);
                hipLaunchKernelGGL((k_radlong_project_param<decltype(pc)::value, FT, decltype(gt)>), g, dim3(256), 0, h->stream, (const FT*)p.dflow, N,
                                   p.dmask, C, spacing, dcent, H, W, h->an_rad, h->an_lon, p.mm, p.cnt);
            });
        });
}

int polar_project_param(tf_handle* h, const Src& flow, int f16, int N, int n_used, int H, int W, const Src& mask, int C, int param,
                        double spacing, int grad_f64, float* mag_out, float* ang_out, float* minmax, long long* nonzero, float* ang_mode)
{
    const bool arrays = mag_out || ang_out;
    Projection p{h, n_used, H, W};                              // meta: the head, then mode k [n_used], angle bins [n_used][PO_NBINS]
    int rc = p.begin(flow, f16, N, param, mask, C, tf_handle::PRE_PO_META, 32 + (size_t)n_used * (16 + 4 + PO_NBINS * 4));
    if (rc) return rc;
    Pre pre(h);
    float* m32 = arrays ? pre.get<float>(tf_handle::PRE_PO_OUT, p.tot * 2) : nullptr;
    if (pre.rc) return pre.rc;
    float* a32 = arrays ? m32 + p.tot : nullptr;
    int* dmode = (int*)(p.meta + 32 + (size_t)n_used * 16);
    unsigned* bins = (unsigned*)(p.meta + 32 + (size_t)n_used * 20);
    std::vector<int> kh((size_t)n_used);
    const hipStream_t s = h->stream;
    // each block takes >= 4096 pixels of a frame: its angle bins go to global memory once per block
    const int gx = (int)((p.npx + 4095) / 4096);
    const dim3 g(gx < 64 ? gx : 64, n_used);
    dispatch_param(param, f16, grad_f64, [&](auto pc, auto ft, auto gt) {
        using FT = decltype(ft);
        hipLaunchKernelGGL((k_polar_project_param<decltype(pc)::value, FT, decltype(gt)>), g, dim3(256), 0, s, (const FT*)p.dflow, N, p.dmask, C,
                           spacing, H, W, h->an_rad, h->an_lon, m32, a32, p.mm, p.cnt, bins);
    });
    hipLaunchKernelGGL(k_polar_mode, dim3((unsigned)n_used), dim3(256), 0, s, bins, dmode);
    HIPC(h, hipMemcpyAsync(kh.data(), dmode, kh.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    if (mag_out) HIPC(h, hipMemcpyAsync(mag_out, m32, p.tot * sizeof(float), hipMemcpyDeviceToHost, s));
    if (ang_out) HIPC(h, hipMemcpyAsync(ang_out, a32, p.tot * sizeof(float), hipMemcpyDeviceToHost, s));
    double mm[4];
    if ((rc = p.end(mm, nonzero, true))) return rc;
    for (int j = 0; j < 4; ++j) minmax[j] = (float)mm[j];                    // exact: the planes hold float32 values
    for (int i = 0; i < n_used; ++i) ang_mode[i] = kh[i] ? (float)kh[i] / 100.f : std::numeric_limits<float>::quiet_NaN();
    return TF_OK;
}

// what tf_radlong_project_param and tf_polar_project_param check alike
int check_project_param(const tf_handle* h, const void* flow, const uint8_t* mask, const void* minmax, const long long* nonzero, int N, int n_used,
                        int H, int W, int mask_C, int param, double spacing)
{
    if (!h || !flow || !mask || !minmax || !nonzero || N < 1 || n_used < 1 || H < 1 || W < 1 || n_used > N) return TF_ERR_INVALID_ARG;
    if ((mask_C != 1 && mask_C != 2) || param < TF_PARAM_VELOCITY || param > TF_PARAM_PWR) return TF_ERR_INVALID_ARG;
    if (param != TF_PARAM_VELOCITY && (N < 2 || !std::isfinite(spacing) || spacing == 0.0)) return TF_ERR_INVALID_ARG;   // np.gradient needs 2 frames
    return n_used > 65535 ? TF_ERR_UNSUPPORTED : TF_OK;                                                                // frames are grid.y
}
}  // namespace

static_assert(TF_PARAM_VELOCITY == RL_PARAM_VELOCITY && TF_PARAM_ACCELERATION == RL_PARAM_ACCELERATION && TF_PARAM_PWR == RL_PARAM_PWR,
              "param codes of the header and the kernel differ");

TF_API int tf_radlong_project(tf_handle* h, const float* flow, const double* centroids, int N, int H, int W,
                              double* rad_out, double* long_out, double* minmax, long long* nonzero)
{
    if (!h || !flow || !centroids || !minmax || !nonzero || N < 1 || H < 1 || W < 1) return TF_ERR_INVALID_ARG;
    return finish_host_call(h, radlong_project(h, Src::on_host(flow), 0, N, N, H, W, Src(), 0, RL_PARAM_VELOCITY, centroids, rad_out, long_out, minmax, nonzero,
        [&](const Projection& p, const double* dcent, dim3 g) {   // the flows as they are: no mask, no param field
            hipLaunchKernelGGL(k_radlong_project, g, dim3(256), 0, h->stream, (const float*)p.dflow, dcent, H, W, h->an_rad, h->an_lon, p.mm, p.cnt);
        }));
}

TF_API int tf_radlong_project_param(tf_handle* h, const void* flow, int flow_is_f16, int N, int n_used, int H, int W, const uint8_t* mask,
                                    int mask_C, int param, double spacing, int grad_f64, const double* centroids, double* rad_out,
                                    double* long_out, double* minmax, long long* nonzero)
{
    if (!centroids) return TF_ERR_INVALID_ARG;
    if (int rc = check_project_param(h, flow, mask, minmax, nonzero, N, n_used, H, W, mask_C, param, spacing)) return rc;
    return finish_host_call(h, radlong_project_param(h, Src::on_host(flow), flow_is_f16 ? 1 : 0, N, n_used, H, W, Src::on_host(mask), mask_C, param, spacing, grad_f64 ? 1 : 0,
                                                     centroids, rad_out, long_out, minmax, nonzero));
}

TF_API int tf_polar_project_param(tf_handle* h, const void* flow, int flow_is_f16, int N, int n_used, int H, int W, const uint8_t* mask,
                                  int mask_C, int param, double spacing, int grad_f64, float* mag_out, float* ang_out, float* minmax,
                                  long long* nonzero, float* ang_mode)
{
    if (!ang_mode) return TF_ERR_INVALID_ARG;
    if (int rc = check_project_param(h, flow, mask, minmax, nonzero, N, n_used, H, W, mask_C, param, spacing)) return rc;
    if ((size_t)H * W > 0xFFFFFFFFu) return TF_ERR_UNSUPPORTED;                         // a frame's counts are 32-bit
    return finish_host_call(h, polar_project_param(h, Src::on_host(flow), flow_is_f16 ? 1 : 0, N, n_used, H, W, Src::on_host(mask), mask_C, param, spacing, grad_f64 ? 1 : 0,
                                                   mag_out, ang_out, minmax, nonzero, ang_mode));
}

TF_API int tf_radlong_shape(tf_handle* h, int* shape)
{
    if (!h || !shape) return TF_ERR_INVALID_ARG;
    const bool have = h->anN >= 1 && !h->an_polar;
    shape[0] = have ? h->anN : 0; shape[1] = have ? h->anH : 0; shape[2] = have ? h->anW : 0;
    return TF_OK;
}
