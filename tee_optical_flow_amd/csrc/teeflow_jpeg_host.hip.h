// Frames held from DICOM JPEG Baseline pixel data (tf_jpeg_decode, tf_hold_frames_jpeg; kernels: teeflow_jpeg.hip.h).  The host parses
// every frame's header (teeflow_jpeg_core.h) into a descriptor -- a column of the per-frame table -- so that every grid is known before
// the first launch; the compressed bytes go up as a batch of streams, the four kernels run batch by batch of frames under the
// coefficient budget, and only a call whose every frame decoded touches the held frames.  Relies on teeflow_streams_host.hip.h and on
// teeflow_frames_host.hip.h (the RLE caps, frames_quiesce, frames_buffer, frames_commit).

namespace {
constexpr size_t JPEG_COEF_BUDGET = (size_t)256 << 20;        // a batch's coefficient scratch

const char* jpeg_status_text(int s)
{
    static const char* const text[] = {"ok", "bad header", "a process that is not decoded", "entropy data that does not decode"};
    return s >= 0 && s <= 3 ? text[s] : "unknown status";
}

struct JpegJob {
    tfs::Batch in; int H, W, samples;                         // the frames (checked: jpeg_check; in.n of them) and their shape
    size_t hw() const { return (size_t)H * W; }
    size_t plane() const { return (((size_t)H + 15) & ~(size_t)15) * (((size_t)W + 15) & ~(size_t)15); }   // a component at MCU-padded size, at most
};

// before any GPU work
int jpeg_check(tf_handle* h, const char* who, JpegJob& j)
{
    if (j.in.n < 1 || j.H < 1 || j.W < 1) return fail(h, TF_ERR_INVALID_ARG, "%s: bad sizes: N=%d H=%d W=%d", who, j.in.n, j.H, j.W);
    if (j.samples != 1 && j.samples != 3) return fail(h, TF_ERR_INVALID_ARG, "%s: samples must be 1 or 3, got %d", who, j.samples);
    if (j.H > 65535 || j.W > 65535) return fail(h, TF_ERR_INVALID_ARG, "%s: a JPEG frame has at most 65535 rows and columns, got %d x %d", who, j.H, j.W);
    if ((double)j.H * j.W > RLE_MAX_PLANE) return fail(h, TF_ERR_INVALID_ARG, "%s: a plane of %d x %d bytes, at most %u", who, j.H, j.W, RLE_MAX_PLANE);
    return streams_check(h, who, j.in, RLE_MAX_FRAME, "frame");
}

// The frames of j decoded on the handle's stream into the handle's scratch, waited for: *dout [N][H][W][samples], or (planar)
// [N][samples][H * W]; status [N] (host) is complete.  A frame whose status is set has whatever the scratch held.
int jpeg_run(tf_handle* h, const JpegJob& j, bool planar, const uint8_t** dout, int* status)
{
    const int N = j.in.n;
    const size_t n = (size_t)N, plane = j.plane(), stride = plane * j.samples;
    const uint32_t ni_max = (uint32_t)(plane / 64);
    enum { DESC, OFF, LEN, STATUS, END };                     // desc [n] | off [n] u64 | len [n] u32 | status [n] i32 | scan end [n] u32
    tfs::Table t = tfs::table(j.in, {sizeof(tfj::Desc), 8, 4, 4, 4}, OFF, LEN);
    auto* descs = (tfj::Desc*)t.col(DESC);
    auto* st = (int*)t.col(STATUS);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* fr = j.in.blob + j.in.off[i];
        st[i] = tfj::parse_header([fr](uint32_t k) -> uint8_t { return fr[k]; }, j.in.len[i], j.H, j.W, j.samples, &descs[i]);
        if (st[i]) memset(&descs[i], 0, sizeof(tfj::Desc));   // (no intervals, no blocks: no kernel looks at the frame)
    }
    const size_t budget = h->jpeg_batch_kib ? (size_t)h->jpeg_batch_kib << 10 : JPEG_COEF_BUDGET;
    const int nf = chunk_frames(stride * sizeof(int16_t), N, 65535, budget);
    Pre pre(h);
    auto* drst = pre.get<uint32_t>(tf_handle::PRE_JPEG_RST, n * ni_max);
    auto* dcoef = pre.get<int16_t>(tf_handle::PRE_JPEG_COEF, (size_t)nf * stride);
    auto* dplanes = pre.get<uint8_t>(tf_handle::PRE_JPEG_PLANES, (size_t)nf * stride);
    auto* out = pre.get<uint8_t>(tf_handle::PRE_JPEG_OUT, n * j.hw() * j.samples);
    if (pre.rc) return pre.rc;
    const uint8_t* dblob = nullptr; uint8_t* dtab = nullptr;
    if (int rc = streams_upload(h, j.in, t, tf_handle::PRE_JPEG_BLOB, tf_handle::PRE_JPEG_TABLE, &tf_handle::frames_upload_bytes, &dblob, &dtab)) return rc;
    const auto& at = t.at;
    auto* ddesc = (const tfj::Desc*)(dtab + at[DESC]);
    auto* doff = (const unsigned long long*)(dtab + at[OFF]);
    auto* dlen = (const uint32_t*)(dtab + at[LEN]);
    auto* dstatus = (int*)(dtab + at[STATUS]);
    auto* dend = (uint32_t*)(dtab + at[END]);
    for (int s : {tf_handle::DT_JPEG_MARKS, tf_handle::DT_JPEG_ENTROPY, tf_handle::DT_JPEG_IDCT, tf_handle::DT_JPEG_FINISH}) h->dev_ms[s] = 0;
    h->jpeg_bytes = 0;
    HIPC(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(k_jpeg_marks, dim3((unsigned)N), dim3(64), 0, h->stream, dblob, doff, dlen, ddesc, N, ni_max, drst, dend, dstatus);
    HIPC(h, hipGetLastError());
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int m = std::min(nf, N - f0);
        uint32_t max_int = 0, max_blocks = 0;
        for (int f = f0; f < f0 + m; ++f) { max_int = std::max(max_int, descs[f].nint); max_blocks = std::max(max_blocks, descs[f].nmcu * descs[f].bpm); }
        ++h->jpeg_batches;
        HIPC(h, hipEventRecord(h->ev[1], h->stream));
        if (max_int)
            hipLaunchKernelGGL(k_jpeg_entropy, dim3(max_int, (unsigned)m), dim3(64), 0, h->stream, dblob, doff, dlen, ddesc, f0, ni_max, (const uint32_t*)drst,
                               (const uint32_t*)dend, dcoef, stride, dstatus);
        HIPC(h, hipEventRecord(h->ev[2], h->stream));
        if (max_blocks)
            hipLaunchKernelGGL(k_jpeg_idct, dim3((max_blocks + 63) / 64, (unsigned)m), dim3(64), 0, h->stream, ddesc, f0, (const int16_t*)dcoef, stride, dplanes,
                               plane, j.samples, (const int*)dstatus);
        HIPC(h, hipEventRecord(h->ev[3], h->stream));
        if (max_blocks)
            hipLaunchKernelGGL(k_jpeg_finish, dim3((unsigned)((j.hw() + 255) / 256), (unsigned)m), dim3(256), 0, h->stream, ddesc, f0, (const uint8_t*)dplanes,
                               plane, j.samples, j.H, j.W, planar ? 1 : 0, out, (const int*)dstatus);
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(h->ev[4], h->stream));
        if (f0 + m >= N) HIPC(h, hipMemcpyAsync(status, dstatus, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));             // the next batch writes the same scratch and records the same events
        if (f0 == 0) (void)dev_time(h, 0, 1, tf_handle::DT_JPEG_MARKS, false);
        (void)dev_time(h, 1, 2, tf_handle::DT_JPEG_ENTROPY, true);
        (void)dev_time(h, 2, 3, tf_handle::DT_JPEG_IDCT, true);
        (void)dev_time(h, 3, 4, tf_handle::DT_JPEG_FINISH, true);
    }
    h->jpeg_bytes = (long long)j.in.bytes() + (long long)(n * j.hw() * j.samples);
    *dout = out;
    return TF_OK;
}

int jpeg_decode(tf_handle* h, const JpegJob& j, uint8_t* out_host, int* status)
{
    HIPC(h, hipSetDevice(h->dev));
    const uint8_t* dout = nullptr;
    if (int rc = jpeg_run(h, j, false, &dout, status)) return rc;
    const int N = j.in.n;
    const size_t frame_bytes = j.hw() * j.samples;
    if (std::count(status, status + N, 0) == N) HIPC(h, hipMemcpyAsync(out_host, dout, (size_t)N * frame_bytes, hipMemcpyDeviceToHost, h->stream));
    else
        for (int i = 0; i < N; ++i)
            if (status[i] == 0) HIPC(h, hipMemcpyAsync(out_host + (size_t)i * frame_bytes, dout + (size_t)i * frame_bytes, frame_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return streams_verdict(h, "tf_jpeg_decode", "frame", "decode", jpeg_status_text, status, N);
}

// form: TF_FRAMES_*, or tfg::YBR_LIBJPEG
int hold_frames_jpeg(tf_handle* h, const JpegJob& j, int form, bool flip, int* status_out)
{
    int rc = frames_quiesce(h);
    if (rc) return rc;
    std::vector<int> status((size_t)j.in.n);
    const uint8_t* dplanes = nullptr;
    if ((rc = jpeg_run(h, j, true, &dplanes, status.data()))) return rc;
    if (status_out) memcpy(status_out, status.data(), status.size() * sizeof(int));
    if ((rc = streams_verdict(h, "tf_hold_frames_jpeg", "frame", "decode", jpeg_status_text, status.data(), j.in.n))) return rc;
    // every frame decoded: only now are the held frames touched, the sample planes being the source
    if ((rc = frames_buffer(h, (size_t)j.in.n * j.hw() * 3, true, j.in.n, j.H, j.W))) return rc;
    return frames_commit(h, dplanes, j.hw(), form, flip, j.in.n, j.H, j.W);
}
}  // namespace

TF_API int tf_jpeg_stage_bytes(void) { return (int)jpeg::STAGE; }

TF_API int tf_jpeg_decode(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                          uint8_t* out_host, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    JpegJob j{{blob, off, len, N}, H, W, samples};
    if (int rc = jpeg_check(h, "tf_jpeg_decode", j)) return rc;
    if (!out_host || !status) return fail(h, TF_ERR_INVALID_ARG, "tf_jpeg_decode: null out_host or status");
    return finish_host_call(h, jpeg_decode(h, j, out_host, status));
}

TF_API int tf_hold_frames_jpeg(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                               int form, int color, int flip_lr, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const char* who = "tf_hold_frames_jpeg";
    if (form != TF_FRAMES_RGB && form != TF_FRAMES_GRAY && form != TF_FRAMES_YBR_FULL)
        return fail(h, TF_ERR_INVALID_ARG, "%s: form %d is none of TF_FRAMES_RGB (0), TF_FRAMES_GRAY (1), TF_FRAMES_YBR_FULL (2)", who, form);
    if (samples != (form == TF_FRAMES_GRAY ? 1 : 3))
        return fail(h, TF_ERR_INVALID_ARG, "%s: form %d has %d samples a pixel, got samples = %d", who, form, form == TF_FRAMES_GRAY ? 1 : 3, samples);
    if (color != TF_JPEG_COLOR_NONE && color != TF_JPEG_COLOR_LIBJPEG)
        return fail(h, TF_ERR_INVALID_ARG, "%s: color %d is neither TF_JPEG_COLOR_NONE (0) nor TF_JPEG_COLOR_LIBJPEG (1)", who, color);
    if (color == TF_JPEG_COLOR_LIBJPEG && form != TF_FRAMES_YBR_FULL)
        return fail(h, TF_ERR_INVALID_ARG, "%s: TF_JPEG_COLOR_LIBJPEG converts Y, Cb, Cr: it needs samples = 3 and form TF_FRAMES_YBR_FULL, got form %d", who, form);
    JpegJob j{{blob, off, len, N}, H, W, samples};
    if (int rc = jpeg_check(h, who, j)) return rc;
    return finish_host_call(h, hold_frames_jpeg(h, j, color == TF_JPEG_COLOR_LIBJPEG ? (int)tfg::YBR_LIBJPEG : form, flip_lr != 0, status));
}
