// Frames held from DICOM JPEG Lossless pixel data (tf_jpegll_decode, tf_hold_frames_jpegll; kernels: teeflow_jpegll.hip.h).  The
// Baseline row's shape (teeflow_jpeg_host.hip.h), whose job record, checks, status texts and scratch slots this file uses -- a handle
// runs one of the two decoders at a time: the host parses every frame's header (teeflow_jpegll_core.h) into a tfj::Desc, the compressed
// bytes go up as a batch of streams, k_jpeg_marks runs once and the three k_jpegll_* kernels batch by batch of frames under the
// difference budget, and only a call whose every frame decoded touches the held frames.

namespace {
constexpr size_t JPEGLL_DIFF_BUDGET = (size_t)256 << 20;      // a batch's difference scratch

// The frames of j decoded on the handle's stream into the handle's scratch, waited for: *dout [N][H][W][samples], or (planar)
// [N][samples][H * W]; status [N] (host) is complete.  A frame whose status is set has whatever the scratch held.
int jpegll_run(tf_handle* h, const JpegJob& j, bool planar, const uint8_t** dout, int* status)
{
    const int N = j.in.n;
    const size_t n = (size_t)N, stride = j.hw() * j.samples;
    const uint32_t ni_max = (uint32_t)j.H;                    // (an interval is at least a row)
    enum { DESC, OFF, LEN, STATUS, END };                     // desc [n] | off [n] u64 | len [n] u32 | status [n] i32 | scan end [n] u32
    tfs::Table t = tfs::table(j.in, {sizeof(tfj::Desc), 8, 4, 4, 4}, OFF, LEN);
    auto* descs = (tfj::Desc*)t.col(DESC);
    auto* st = (int*)t.col(STATUS);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* fr = j.in.blob + j.in.off[i];
        st[i] = tfl::parse_header([fr](uint32_t k) -> uint8_t { return fr[k]; }, j.in.len[i], j.H, j.W, j.samples, &descs[i]);
        if (st[i]) memset(&descs[i], 0, sizeof(tfj::Desc));   // (no intervals, no samples: no kernel looks at the frame)
    }
    const size_t budget = h->jpeg_batch_kib ? (size_t)h->jpeg_batch_kib << 10 : JPEGLL_DIFF_BUDGET;
    const int nf = chunk_frames(stride * sizeof(uint16_t), N, 65535, budget);
    Pre pre(h);
    auto* drst = pre.get<uint32_t>(tf_handle::PRE_JPEG_RST, n * ni_max);
    auto* ddiff = pre.get<uint16_t>(tf_handle::PRE_JPEG_COEF, (size_t)nf * stride);
    auto* out = pre.get<uint8_t>(tf_handle::PRE_JPEG_OUT, n * stride);
    if (pre.rc) return pre.rc;
    const uint8_t* dblob = nullptr; uint8_t* dtab = nullptr;
    if (int rc = streams_upload(h, j.in, t, tf_handle::PRE_JPEG_BLOB, tf_handle::PRE_JPEG_TABLE, &tf_handle::frames_upload_bytes, &dblob, &dtab)) return rc;
    const auto& at = t.at;
    auto* ddesc = (const tfj::Desc*)(dtab + at[DESC]);
    auto* doff = (const unsigned long long*)(dtab + at[OFF]);
    auto* dlen = (const uint32_t*)(dtab + at[LEN]);
    auto* dstatus = (int*)(dtab + at[STATUS]);
    auto* dend = (uint32_t*)(dtab + at[END]);
    h->dev_ms[tf_handle::DT_JPEGLL_ENTROPY] = h->dev_ms[tf_handle::DT_JPEGLL_RESTORE] = 0;
    h->jpegll_bytes = 0;
    HIPC(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(k_jpeg_marks, dim3((unsigned)N), dim3(64), 0, h->stream, dblob, doff, dlen, ddesc, N, ni_max, drst, dend, dstatus);
    HIPC(h, hipGetLastError());
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int m = std::min(nf, N - f0);
        uint32_t max_int = 0;
        for (int f = f0; f < f0 + m; ++f) max_int = std::max(max_int, descs[f].nint);
        ++h->jpegll_batches;
        HIPC(h, hipEventRecord(h->ev[1], h->stream));
        if (max_int)
            hipLaunchKernelGGL(k_jpegll_entropy, dim3(max_int, (unsigned)m), dim3(64), 0, h->stream, dblob, doff, dlen, ddesc, f0, ni_max, (const uint32_t*)drst,
                               (const uint32_t*)dend, ddiff, stride, j.hw(), dstatus);
        HIPC(h, hipEventRecord(h->ev[2], h->stream));
        if (max_int) {
            hipLaunchKernelGGL(k_jpegll_col, dim3(max_int, (unsigned)j.samples, (unsigned)m), dim3(64), 0, h->stream, ddesc, f0, ddiff, stride, j.hw(),
                               (const int*)dstatus);
            hipLaunchKernelGGL(k_jpegll_rows, dim3((unsigned)j.H, (unsigned)j.samples, (unsigned)m), dim3(64), 0, h->stream, f0, (const uint16_t*)ddiff, stride,
                               j.samples, j.H, j.W, planar ? 1 : 0, out, dstatus);
        }
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(h->ev[3], h->stream));
        if (f0 + m >= N) HIPC(h, hipMemcpyAsync(status, dstatus, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));             // the next batch writes the same scratch and records the same events
        if (f0 == 0) (void)dev_time(h, 0, 1, tf_handle::DT_JPEGLL_ENTROPY, true);     // (k_jpeg_marks counts as entropy work)
        (void)dev_time(h, 1, 2, tf_handle::DT_JPEGLL_ENTROPY, true);
        (void)dev_time(h, 2, 3, tf_handle::DT_JPEGLL_RESTORE, true);
    }
    h->jpegll_bytes = (long long)j.in.bytes() + (long long)(n * stride);
    *dout = out;
    return TF_OK;
}

int jpegll_decode(tf_handle* h, const JpegJob& j, uint8_t* out_host, int* status)
{
    HIPC(h, hipSetDevice(h->dev));
    const uint8_t* dout = nullptr;
    if (int rc = jpegll_run(h, j, false, &dout, status)) return rc;
    const int N = j.in.n;
    const size_t frame_bytes = j.hw() * j.samples;
    if (std::count(status, status + N, 0) == N) HIPC(h, hipMemcpyAsync(out_host, dout, (size_t)N * frame_bytes, hipMemcpyDeviceToHost, h->stream));
    else
        for (int i = 0; i < N; ++i)
            if (status[i] == 0) HIPC(h, hipMemcpyAsync(out_host + (size_t)i * frame_bytes, dout + (size_t)i * frame_bytes, frame_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return streams_verdict(h, "tf_jpegll_decode", "frame", "decode", jpeg_status_text, status, N);
}

int hold_frames_jpegll(tf_handle* h, const JpegJob& j, int form, bool flip, int* status_out)
{
    int rc = frames_quiesce(h);
    if (rc) return rc;
    std::vector<int> status((size_t)j.in.n);
    const uint8_t* dplanes = nullptr;
    if ((rc = jpegll_run(h, j, true, &dplanes, status.data()))) return rc;
    if (status_out) memcpy(status_out, status.data(), status.size() * sizeof(int));
    if ((rc = streams_verdict(h, "tf_hold_frames_jpegll", "frame", "decode", jpeg_status_text, status.data(), j.in.n))) return rc;
    // every frame decoded: only now are the held frames touched, the sample planes being the source
    if ((rc = frames_buffer(h, (size_t)j.in.n * j.hw() * 3, true, j.in.n, j.H, j.W))) return rc;
    return frames_commit(h, dplanes, j.hw(), form, flip, j.in.n, j.H, j.W);
}
}  // namespace

TF_API int tf_jpegll_decode(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                            uint8_t* out_host, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    JpegJob j{{blob, off, len, N}, H, W, samples};
    if (int rc = jpeg_check(h, "tf_jpegll_decode", j)) return rc;
    if (!out_host || !status) return fail(h, TF_ERR_INVALID_ARG, "tf_jpegll_decode: null out_host or status");
    return finish_host_call(h, jpegll_decode(h, j, out_host, status));
}

TF_API int tf_hold_frames_jpegll(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                                 int form, int flip_lr, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const char* who = "tf_hold_frames_jpegll";
    if (form != TF_FRAMES_RGB && form != TF_FRAMES_GRAY && form != TF_FRAMES_YBR_FULL)
        return fail(h, TF_ERR_INVALID_ARG, "%s: form %d is none of TF_FRAMES_RGB (0), TF_FRAMES_GRAY (1), TF_FRAMES_YBR_FULL (2)", who, form);
    if (samples != (form == TF_FRAMES_GRAY ? 1 : 3))
        return fail(h, TF_ERR_INVALID_ARG, "%s: form %d has %d samples a pixel, got samples = %d", who, form, form == TF_FRAMES_GRAY ? 1 : 3, samples);
    JpegJob j{{blob, off, len, N}, H, W, samples};
    if (int rc = jpeg_check(h, who, j)) return rc;
    return finish_host_call(h, hold_frames_jpegll(h, j, form, flip_lr != 0, status));
}
