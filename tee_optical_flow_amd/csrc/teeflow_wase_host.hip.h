// WASE background compensation of flows that are already solved: the per-flow reduction (also the tail of a WASE study,
// teeflow_study_host.hip.h) and the apply.  Relies on teeflow_scratch.hip.h and on the kernels of teeflow_wase.hip.h.

// ---- WASE background compensation (rows a7 / f2) ---------------------------------------------------------------
namespace {
// flows, bkgd: device.  The per-flow reduction -- count, scan, scatter, piece sums, finish -- leaves the backgrounds in (*dbg)[0..P).
int wase_backgrounds(tf_handle* h, const float* flows, const uint8_t* bkgd, int P, int N, int H, int W, float** dbg)
{
    const size_t hw2 = (size_t)H * W * 2;
    const int C = (int)((hw2 + WASE_CHUNK - 1) / WASE_CHUNK);
    const size_t ncnt = (size_t)N * C, na = (size_t)N * hw2, npieces = (na + NP_BUFSIZE - 1) / NP_BUFSIZE;
    Pre pre(h);
    auto* wa = pre.get<float>(tf_handle::PRE_WA_VALS, na);
    auto* wcnt = pre.get<unsigned>(tf_handle::PRE_WA_CNT, ncnt);
    auto* woff = pre.get<u64>(tf_handle::PRE_WA_OFF, ncnt + 1);
    auto* wsum = pre.get<float>(tf_handle::PRE_WA_SUM, npieces);
    auto* wbg = pre.get<float>(tf_handle::PRE_WA_BG, (size_t)P);
    if (pre.rc) return pre.rc;
    hipStream_t s = h->stream;
    for (int p = 0; p < P; ++p) {
        const float* f = flows + (size_t)p * hw2;
        hipLaunchKernelGGL(k_wase_count, dim3(C, N), dim3(256), 0, s, f, bkgd, hw2, C, wcnt);
        hipLaunchKernelGGL(k_wase_scan, dim3(1), dim3(1024), 0, s, wcnt, ncnt, woff);
        hipLaunchKernelGGL(k_wase_scatter, dim3(C, N), dim3(256), 0, s, f, bkgd, hw2, C, woff, wa);
        hipLaunchKernelGGL(k_wase_piece_sums, dim3((unsigned)npieces), dim3(512), 0, s, wa, woff + ncnt, wsum);
        hipLaunchKernelGGL(k_wase_finish, dim3(1), dim3(64), 0, s, wsum, woff + ncnt, wbg + p);
    }
    HIPC(h, hipGetLastError());
    *dbg = wbg;
    return TF_OK;
}

// the reduction, then the apply: leaves the compensated, scaled flows in place
int wase_device(tf_handle* h, float* flows, const uint8_t* bkgd, int P, int N, int H, int W, float scale, float** dbg)
{
    const int rc = wase_backgrounds(h, flows, bkgd, P, N, H, W, dbg);
    if (rc) return rc;
    const size_t hw2 = (size_t)H * W * 2;
    const unsigned gx = (unsigned)std::min<size_t>((hw2 + 255) / 256, 1024);
    hipLaunchKernelGGL(k_wase_apply, dim3(gx, P), dim3(256), 0, h->stream, flows, *dbg, hw2, scale);
    HIPC(h, hipGetLastError());
    return TF_OK;
}

int wase_compensate(tf_handle* h, float* flows, int n_flows, const uint8_t* bkgd, int n_frames, int H, int W, float scale, float* background_out)
{
    HIPC(h, hipSetDevice(h->dev));
    const size_t hw2 = (size_t)H * W * 2;
    const int chunk = 64;                                   // flows per round trip
    Pre pre(h);
    auto* dm = pre.get<uint8_t>(tf_handle::PRE_AN_MASK, (size_t)n_frames * hw2);
    auto* df = pre.get<float>(tf_handle::PRE_AN_FLOW, (size_t)std::min(chunk, n_flows) * hw2);
    if (pre.rc) return pre.rc;
    HIPC(h, hipMemcpyAsync(dm, bkgd, (size_t)n_frames * hw2, hipMemcpyHostToDevice, h->stream));
    for (int p0 = 0; p0 < n_flows; p0 += chunk) {
        const int np = std::min(chunk, n_flows - p0);
        float* wbg = nullptr;
        HIPC(h, hipMemcpyAsync(df, flows + (size_t)p0 * hw2, (size_t)np * hw2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
        int rc = wase_device(h, df, dm, np, n_frames, H, W, scale, &wbg);
        if (rc) return rc;
        HIPC(h, hipMemcpyAsync(flows + (size_t)p0 * hw2, df, (size_t)np * hw2 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (background_out) HIPC(h, hipMemcpyAsync(background_out + p0, wbg, (size_t)np * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    return TF_OK;
}
}  // namespace

TF_API int tf_wase_compensate_device(tf_handle* h, float* flows, int n_flows, const uint8_t* bkgd, int n_frames, int H, int W, float scale,
                                     float* background_out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!flows || !bkgd || n_flows < 1 || n_frames < 1 || H < 1 || W < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_wase_compensate: bad argument");
    HIPC(h, hipSetDevice(h->dev));
    float* wbg = nullptr;
    int rc = wase_device(h, flows, bkgd, n_flows, n_frames, H, W, scale, &wbg);
    if (rc) return rc;
    if (background_out) HIPC(h, hipMemcpyAsync(background_out, wbg, (size_t)n_flows * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return TF_OK;
}

TF_API int tf_wase_compensate(tf_handle* h, float* flows, int n_flows, const uint8_t* bkgd, int n_frames, int H, int W, float scale,
                              float* background_out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!flows || !bkgd || n_flows < 1 || n_frames < 1 || H < 1 || W < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_wase_compensate: bad argument");
    return finish_host_call(h, wase_compensate(h, flows, n_flows, bkgd, n_frames, H, W, scale, background_out));
}
