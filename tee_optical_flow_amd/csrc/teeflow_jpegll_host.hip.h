// Frames held from DICOM JPEG Lossless pixel data (tf_jpegll_decode, tf_hold_frames_jpegll; kernels: teeflow_jpegll.hip.h).  The
// Baseline row's shape (teeflow_jpeg_host.hip.h), whose job record, checks, status texts and scratch slots this file uses -- a handle
// runs one of the two decoders at a time: the host parses every frame's header (teeflow_jpegll_core.h) into a tfj::Desc, the compressed
// bytes go up as a batch of streams, k_jpeg_marks runs once and the three k_jpegll_* kernels batch by batch of frames under the
// difference budget, and only a call whose every frame decoded touches the held frames.
// The entropy pass of a batch is k_jpegll_entropy alone, or -- where the host's rule (tf_set_tuning "jpegll_split") sends a frame of the
// batch down the split decode -- k_jpegll_spec, a fixed number of k_jpegll_sync rounds, k_jpegll_scan, k_jpegll_emit and
// k_jpegll_entropy_rest for whatever is left; either way nothing between the kernels waits for the host.

namespace {
constexpr size_t JPEGLL_DIFF_BUDGET = (size_t)256 << 20;      // a batch's difference scratch (and the split decode's per-piece scratch)
// "jpegll_split" 0: a frame takes the split decode when its restart intervals hold this many bytes of entropy data on average.  Measured
// (profiles/r31_jpegll_split.txt): the split decode won at every interval length from 398 bytes up but one, 11993 bytes (600 x 800, 3
// samples, 8 rows an interval: 1.09 x the serial kernel, between clear wins at 9036 and 25290 bytes, so the length alone does not
// explain it and its cause is not known); the threshold is the next power of two above that, from which on it won everywhere (0.74 x
// at 25 KB ... 0.10 x at 900 KB).  A safe choice, not a trend: it gives up the 1.1 - 1.9 x measured on shorter intervals.
constexpr uint32_t JPEGLL_SPLIT_MIN_BYTES = 16384;

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
    // Which path, frame by frame, from what the host knows: the split decode where an interval's data is long enough to pay for it.
    // The automatic rule keeps a frame whose components name different codes on the serial kernel: there the phase is part of the
    // compared state and the truth travels a block of pieces a round, so an interval of more than 8 blocks (64 KiB) cannot converge in
    // the default rounds and would pay for both decodes.  "jpegll_split" 2 still sends it down the split decode.
    // A split frame is marked in its descriptor (reserved bit 0; bit 1: its components' tables differ) and has pmax piece slots.
    uint32_t pmax = 0;
    long long split_intervals = 0;
    for (size_t i = 0; i < n; ++i) {
        tfj::Desc& d = descs[i];
        if (st[i] || h->jpegll_split == 1 || j.in.len[i] >= tfsync::MAX_LEN) continue;
        const bool same = tfsync::same_tables(d);
        if (h->jpegll_split == 0 && (!same || (j.in.len[i] - d.scan_off) / d.nint < JPEGLL_SPLIT_MIN_BYTES)) continue;
        d.reserved = 1u | (same ? 0u : 2u);
        pmax = std::max(pmax, tfsync::slot_count(j.in.len[i], d.scan_off, d.nint));
        split_intervals += d.nint;
    }
    const int rounds = h->jpegll_sync_rounds;
    const size_t sync_frame = pmax ? (size_t)pmax * 5 * sizeof(uint32_t) + (size_t)ni_max * 2 * sizeof(uint32_t) : 0;   // (none: the batches are the serial path's)
    const size_t budget = h->jpeg_batch_kib ? (size_t)h->jpeg_batch_kib << 10 : JPEGLL_DIFF_BUDGET;
    const int nf = chunk_frames(stride * sizeof(uint16_t) + sync_frame, N, 65535, budget);
    Pre pre(h);
    auto* drst = pre.get<uint32_t>(tf_handle::PRE_JPEG_RST, n * ni_max);
    auto* ddiff = pre.get<uint16_t>(tf_handle::PRE_JPEG_COEF, (size_t)nf * stride);
    auto* out = pre.get<uint8_t>(tf_handle::PRE_JPEG_OUT, n * stride);
    // the split decode's scratch of a batch: owner | entry | exit 0 | exit 1 | cnt, nf * pmax each; lastchg | conv, nf * ni_max each; a counter
    const size_t np = (size_t)nf * pmax, nk = (size_t)nf * ni_max;
    uint32_t* dsync = pmax ? pre.get<uint32_t>(tf_handle::PRE_JPEG_SYNC, 5 * np + 2 * nk + 4) : nullptr;
    if (pre.rc) return pre.rc;
    auto part = [dsync](size_t at) -> uint32_t* { return dsync ? dsync + at : nullptr; };      // (no split frame: no scratch, and nobody uses a part)
    uint32_t* const downer = part(0), * const dentry = part(np), * const dcnt = part(4 * np), * const dconv = part(5 * np + nk), * const dctr = part(5 * np + 2 * nk);
    uint32_t* const dexit[2] = {part(2 * np), part(3 * np)};
    int* const dlast = (int*)part(5 * np);
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
    h->jpegll_rounds_launched = 0;
    unsigned int fallbacks = 0;
    if (pmax) HIPC(h, hipMemsetAsync(dctr, 0, sizeof(uint32_t), h->stream));
    HIPC(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(k_jpeg_marks, dim3((unsigned)N), dim3(64), 0, h->stream, dblob, doff, dlen, ddesc, N, ni_max, drst, dend, dstatus);
    HIPC(h, hipGetLastError());
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int m = std::min(nf, N - f0);
        uint32_t max_int = 0;
        bool split = false;
        for (int f = f0; f < f0 + m; ++f) { max_int = std::max(max_int, descs[f].nint); split = split || (descs[f].reserved & 1); }
        ++h->jpegll_batches;
        HIPC(h, hipEventRecord(h->ev[1], h->stream));
        if (max_int && !split)
            hipLaunchKernelGGL(k_jpegll_entropy, dim3(max_int, (unsigned)m), dim3(64), 0, h->stream, dblob, doff, dlen, ddesc, f0, ni_max, (const uint32_t*)drst,
                               (const uint32_t*)dend, ddiff, stride, j.hw(), dstatus);
        else if (max_int) {
            // speculation, `rounds` rounds, the verdicts and prefix sums, the differences of what converged; then the serial kernel for
            // the batch's other frames and for what did not converge.  Nothing here waits for the host.
            const dim3 pieces((pmax + 255) / 256, (unsigned)m), waves(max_int, (unsigned)m);
            const uint32_t* crst = drst; const uint32_t* cend = dend;
            hipLaunchKernelGGL(k_jpegll_spec, pieces, dim3(256), 0, h->stream, dblob, doff, dlen, ddesc, f0, ni_max, crst, cend, pmax, downer, dentry, dexit[0], dcnt,
                               dlast, (const int*)dstatus);
            for (int r = 1; r <= rounds; ++r)
                hipLaunchKernelGGL(k_jpegll_sync, pieces, dim3(256), 0, h->stream, dblob, doff, dlen, ddesc, f0, ni_max, crst, cend, pmax, (const uint32_t*)downer, dentry,
                                   (const uint32_t*)dexit[(r - 1) & 1], dexit[r & 1], dcnt, dlast, r, (const int*)dstatus);
            hipLaunchKernelGGL(k_jpegll_scan, waves, dim3(64), 0, h->stream, dlen, ddesc, f0, ni_max, crst, cend, pmax, dcnt, (const int*)dlast, dconv, rounds, dctr,
                               (const int*)dstatus);
            hipLaunchKernelGGL(k_jpegll_emit, pieces, dim3(256), 0, h->stream, dblob, doff, dlen, ddesc, f0, ni_max, crst, cend, pmax, (const uint32_t*)downer,
                               (const uint32_t*)dentry, (const uint32_t*)dcnt, (const uint32_t*)dconv, ddiff, stride, j.hw(), dstatus);
            hipLaunchKernelGGL(k_jpegll_entropy_rest, waves, dim3(64), 0, h->stream, dblob, doff, dlen, ddesc, f0, ni_max, crst, cend, ddiff, stride, j.hw(), dstatus,
                               (const uint32_t*)dconv);
            h->jpegll_rounds_launched += rounds;
        }
        HIPC(h, hipEventRecord(h->ev[2], h->stream));
        if (max_int) {
            hipLaunchKernelGGL(k_jpegll_col, dim3(max_int, (unsigned)j.samples, (unsigned)m), dim3(64), 0, h->stream, ddesc, f0, ddiff, stride, j.hw(),
                               (const int*)dstatus);
            hipLaunchKernelGGL(k_jpegll_rows, dim3((unsigned)j.H, (unsigned)j.samples, (unsigned)m), dim3(64), 0, h->stream, f0, (const uint16_t*)ddiff, stride,
                               j.samples, j.H, j.W, planar ? 1 : 0, out, dstatus);
        }
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(h->ev[3], h->stream));
        if (f0 + m >= N) {
            HIPC(h, hipMemcpyAsync(status, dstatus, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            if (pmax) HIPC(h, hipMemcpyAsync(&fallbacks, dctr, sizeof fallbacks, hipMemcpyDeviceToHost, h->stream));
        }
        HIPC(h, hipStreamSynchronize(h->stream));             // the next batch writes the same scratch and records the same events
        if (f0 == 0) (void)dev_time(h, 0, 1, tf_handle::DT_JPEGLL_ENTROPY, true);     // (k_jpeg_marks counts as entropy work)
        (void)dev_time(h, 1, 2, tf_handle::DT_JPEGLL_ENTROPY, true);
        (void)dev_time(h, 2, 3, tf_handle::DT_JPEGLL_RESTORE, true);
    }
    h->jpegll_bytes = (long long)j.in.bytes() + (long long)(n * stride);
    h->jpegll_split_intervals += split_intervals;             // (counted once the call's work is done)
    h->jpegll_serial_fallbacks += fallbacks;
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

TF_API int tf_jpegll_segment_bytes(void) { return (int)tfsync::SEG; }

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
