// A call's frames: where it finds them (the caller's host pointer, or the held frames behind tf_frames_next), then what is made of
// them around the solver -- conditioned gray frames, the float16 echo, saliency maps -- and, in the second half, the held frames
// themselves (tf_hold_frames & co.), last the same from RLE Lossless pixel data (tf_rle_decode, tf_hold_frames_rle).  Relies on
// teeflow_scratch.hip.h, teeflow_streams_host.hip.h (the RLE frames are a batch of streams), and on the kernels of teeflow_cond /
// _saliency / _ingest / _rle.hip.h.

namespace {
// The RGB frames of a frames-taking call named `who`: the caller's host pointer, or -- armed by tf_frames_next, `a` being what
// spend() gave the call at its start -- frames [first, first + count) of the held frames where they are.  The armed call passes a
// null pointer, N == count, three channels and the held H x W; anything else is refused with both shapes.  Called once the call's
// own argument checks have passed.
int take_frames(tf_handle* h, const char* who, const tf_handle::Armed& a, const void* rgb, int N, int H, int W, int channels, Src* out)
{
    if (!a.frames) { *out = Src::on_host(rgb); return TF_OK; }
    const tf_handle::Frames& k = h->frames;
    const int first = a.first, count = a.count;
    if (k.N < 1) return fail(h, TF_ERR_INVALID_ARG, "%s: tf_frames_next was armed, but no frames are held (tf_hold_frames)", who);
    if (first < 0 || count < 1 || first > k.N - count)
        return fail(h, TF_ERR_INVALID_ARG, "%s: tf_frames_next armed frames [%d, %d + %d), outside the %d held frames", who, first, first, count, k.N);
    if (rgb) return fail(h, TF_ERR_INVALID_ARG, "%s: tf_frames_next was armed: the call reads the held frames and passes a null frame pointer", who);
    if (N != count || H != k.H || W != k.W || channels != 3)
        return fail(h, TF_ERR_INVALID_ARG, "%s: the call's frames are %d x %d x %d x %d, the armed range of the held frames %d x %d x %d x 3 "
                                           "(%d frames held)", who, N, H, W, channels, count, k.H, k.W, k.N);
    *out = Src::on_device(k.rgb + (size_t)first * k.H * k.W * 3);
    ++h->frames_held_reads;
    return TF_OK;
}

// What every frames-taking tail call opens with: the frames flag spent (once h is known not to be null, refused or not), a null frame
// pointer let through for the armed call alone, then the call's own argument checks -- args_rc, what they gave -- and take_frames,
// the first to read the handle.
int call_frames(tf_handle* h, const char* who, const void* rgb, int N, int H, int W, int channels, int args_rc, Src* out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const tf_handle::Armed armed = spend(h, SPEND_FRAMES);
    if (!rgb && !armed.frames) return TF_ERR_INVALID_ARG;
    if (args_rc) return args_rc;
    return take_frames(h, who, armed, rgb, N, H, W, channels, out);
}

// n pixels of uploaded RGB (device) -> their float16 `echo` values in the caller's host buffer, behind what is queued on the handle's
// stream; the copy is done when the stream has been waited for.  decho: device scratch of at least n halves.  keep (device, or null):
// gets the same halves by a copy on the device (a held study's echo).  Without a host buffer (echo16_out null) the kernel writes
// straight into `keep`: no scratch, no copy.
int echo_from_device_rgb(tf_handle* h, const uint8_t* drgb, size_t n, uint16_t* decho, uint16_t* echo16_out, uint16_t* keep = nullptr)
{
    if (!echo16_out && !keep) return TF_OK;
    hipLaunchKernelGGL(k_echo_f16, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, h->stream, drgb, n, echo16_out ? decho : keep);
    HIPC(h, hipGetLastError());
    if (!echo16_out) return TF_OK;
    if (keep) HIPC(h, hipMemcpyAsync(keep, decho, n * sizeof(uint16_t), hipMemcpyDeviceToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(echo16_out, decho, n * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
    return TF_OK;
}

// rgb (host, or the held frames) -> conditioned gray frames in the handle's preprocessing buffer (valid until the handle's next preprocessing call)
// (`own`: into that caller-owned buffer instead -- a submitted job's frames must outlive the handle's next preprocessing call)
// echo16_out (host, [N][H][W] halves, or null): also the study's `echo`, from the same upload; complete on return
// (echo_keep: device memory that gets the echo too, see echo_from_device_rgb)
int condition_to_device(tf_handle* h, const Src& rgb, int N, int H, int W, const uint8_t** dgray_out, uint8_t* own = nullptr,
                        uint16_t* echo16_out = nullptr, uint16_t* echo_keep = nullptr)
{
    const size_t npx = (size_t)H * W;
    HIPC(h, hipSetDevice(h->dev));
    Pre pre(h);
    auto* urgb = rgb.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_SRC, (size_t)N * npx * 3);
    auto* dgray = own ? own : pre.get<uint8_t>(tf_handle::PRE_OUT, (size_t)N * npx);
    auto* mm = pre.get<u64>(tf_handle::PRE_MX, (size_t)N * 2);
    auto* decho = echo16_out ? pre.get<uint16_t>(tf_handle::PRE_ECHO, (size_t)N * npx) : nullptr;
    if (pre.rc) return pre.rc;
    const std::vector<u64> init = minmax_seed((size_t)N);
    const uint8_t* drgb = nullptr;
    if (int rc = src_to_device(h, rgb, 0, (size_t)N * npx * 3, urgb, &drgb, &tf_handle::frames_upload_bytes)) return rc;
    HIPC(h, hipMemcpyAsync(mm, init.data(), init.size() * sizeof(u64), hipMemcpyHostToDevice, h->stream));
    const int gx = (int)((npx + 255) / 256);
    hipLaunchKernelGGL(k_cond_minmax, dim3(gx < 512 ? gx : 512, N), dim3(256), 0, h->stream, drgb, npx, mm);
    hipLaunchKernelGGL(k_cond_norm, dim3(gx, N), dim3(256), 0, h->stream, drgb, npx, mm, dgray);
    if (echo16_out || echo_keep) { const int rc = echo_from_device_rgb(h, drgb, (size_t)N * npx, decho, echo16_out, echo_keep); if (rc) return rc; }
    HIPC(h, hipStreamSynchronize(h->stream));            // `init` leaves scope; the solve may run on other streams (lanes)
    *dgray_out = dgray;
    return TF_OK;
}

int condition_frames(tf_handle* h, const Src& rgb, int N, int H, int W, uint8_t* gray_out)
{
    const uint8_t* dgray = nullptr;
    int rc = condition_to_device(h, rgb, N, H, W, &dgray);
    if (rc) return rc;
    HIPC(h, hipMemcpy(gray_out, dgray, (size_t)N * H * W, hipMemcpyDeviceToHost));
    return TF_OK;
}
}  // namespace

TF_API int tf_condition_frames(tf_handle* h, const uint8_t* rgb, int N, int H, int W, uint8_t* gray_out)
{
    Src fr;
    const int args_rc = !gray_out || N < 1 || H < 1 || W < 1 ? TF_ERR_INVALID_ARG : TF_OK;
    if (int rc = call_frames(h, "tf_condition_frames", rgb, N, H, W, 3, args_rc, &fr)) return rc;
    return finish_host_call(h, condition_frames(h, fr, N, H, W, gray_out));
}

// the echo alone: rgb uint8 [N][H][W][3] -> float16 [N][H][W] = half(rgb2gray), one rounding
TF_API int tf_echo_frames(tf_handle* h, const uint8_t* rgb, int N, int H, int W, uint16_t* echo16_out)
{
    Src fr;
    const int args_rc = !echo16_out || N < 1 || H < 1 || W < 1 ? TF_ERR_INVALID_ARG : TF_OK;
    if (int rc = call_frames(h, "tf_echo_frames", rgb, N, H, W, 3, args_rc, &fr)) return rc;
    const size_t n = (size_t)N * H * W;
    auto run = [&]() -> int {
        HIPC(h, hipSetDevice(h->dev));
        Pre pre(h);
        auto* urgb = fr.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_SRC, n * 3);
        auto* decho = pre.get<uint16_t>(tf_handle::PRE_ECHO, n);
        if (pre.rc) return pre.rc;
        const uint8_t* drgb = nullptr;
        int rc = src_to_device(h, fr, 0, n * 3, urgb, &drgb, &tf_handle::frames_upload_bytes);
        if (rc) return rc;
        rc = echo_from_device_rgb(h, drgb, n, decho, echo16_out);
        if (rc) return rc;
        HIPC(h, hipStreamSynchronize(h->stream));
        return TF_OK;
    };
    return finish_host_call(h, run());
}

namespace {
// frames (host, or the held frames; uint8 [N][H][W][channels]) -> fine-grained saliency maps [N][H][W] in the handle's preprocessing buffer: uint8, or
// (f32) float = map * (1/255), what computeSaliency() returns in opencv-contrib 4.x.  Frames go through in chunks so that the work
// buffers (17 B per pixel) stay below ~2.3 GB whatever the study's length; the buffers are the handle's and only ever grow.
// echo16_out (host, or null; channels == 3 only): also the study's float16 `echo`, from each chunk's upload; complete on return
// (echo_keep: device memory that gets the echo too, see echo_from_device_rgb)
int saliency_to_device(tf_handle* h, const Src& frames, int N, int H, int W, int channels, bool f32, const uint8_t** dout,
                       uint16_t* echo16_out = nullptr, uint16_t* echo_keep = nullptr)
{
    const size_t npx = (size_t)H * W, ipx = (size_t)(H + 1) * (W + 1);
    if (H > 65535 || N > 65535) return fail(h, TF_ERR_UNSUPPORTED, "saliency: at most 65535 rows and 65535 frames per call");
    const int nf = chunk_frames(npx, N, 65535, (size_t)1 << 27);   // (the budget counted in pixels: 2^27 of them per chunk)
    HIPC(h, hipSetDevice(h->dev));
    Pre pre(h);
    auto* usrc = frames.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_SRC, nf * npx * channels);
    auto* g0 = pre.get<uint8_t>(tf_handle::PRE_G0, nf * npx);
    auto* g1 = pre.get<uint8_t>(tf_handle::PRE_G1, nf * npx);
    auto* ion = pre.get<uint8_t>(tf_handle::PRE_ION, nf * npx);
    auto* ioff = pre.get<uint8_t>(tf_handle::PRE_IOFF, nf * npx);
    auto* P = pre.get<int>(tf_handle::PRE_P, nf * npx);
    auto* I = pre.get<float>(tf_handle::PRE_I, nf * ipx);
    auto* mon = pre.get<uint16_t>(tf_handle::PRE_MON, nf * npx);
    auto* moff = pre.get<uint16_t>(tf_handle::PRE_MOFF, nf * npx);
    auto* mx = pre.get<int>(tf_handle::PRE_MX, nf * SAL_MX);
    auto* out = pre.get<uint8_t>(tf_handle::PRE_OUT, (size_t)N * npx * (f32 ? sizeof(float) : 1));
    auto* decho = echo16_out ? pre.get<uint16_t>(tf_handle::PRE_ECHO, nf * npx) : nullptr;
    if (pre.rc) return pre.rc;
    h->dev_ms[tf_handle::DT_SALIENCY] = 0;
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int n = std::min(nf, N - f0);
        const size_t px = (size_t)n * npx;
        const dim3 g2((W + 255) / 256, H, n), blk(256);
        const uint8_t* src = nullptr;
        if (int rc = src_to_device(h, frames, f0 * npx * channels, px * channels, usrc, &src, &tf_handle::frames_upload_bytes)) return rc;
        HIPC(h, hipEventRecord(h->ev[0], h->stream));       // the eight kernels of the chunk, without the upload
        HIPC(h, hipMemsetAsync(mx, 0, (size_t)n * SAL_MX * sizeof(int), h->stream));
        hipLaunchKernelGGL(sal::k_sal_gray, dim3((unsigned)((px + 255) / 256)), blk, 0, h->stream, src, channels, px, g0);
        hipLaunchKernelGGL(sal::k_sal_blur3, g2, blk, 0, h->stream, g0, g1, H, W);
        hipLaunchKernelGGL(sal::k_sal_blur3, g2, blk, 0, h->stream, g1, g0, H, W);
        hipLaunchKernelGGL(sal::k_sal_rowprefix, dim3(H, n), dim3(64), 0, h->stream, g0, H, W, P);
        hipLaunchKernelGGL(sal::k_sal_integral, dim3((W + 1 + 255) / 256, n), blk, 0, h->stream, P, H, W, I);
        const dim3 g8((W + 255) / 256, (H + SAL_ROWS - 1) / SAL_ROWS, n);
        hipLaunchKernelGGL(sal::k_sal_scales, g8, blk, 0, h->stream, g0, I, H, W, mon, moff, mx);
        hipLaunchKernelGGL(sal::k_sal_mix_scales, g8, blk, 0, h->stream, mon, moff, H, W, ion, ioff, mx);
        hipLaunchKernelGGL(sal::k_sal_mix_onoff, g2, blk, 0, h->stream, ion, ioff, H, W, mx, f32 ? nullptr : out + f0 * npx,
                           f32 ? (float*)out + f0 * npx : nullptr);
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(h->ev[1], h->stream));
        if (echo16_out) {
            const int rc = echo_from_device_rgb(h, src, px, decho, echo16_out + f0 * npx, echo_keep ? echo_keep + f0 * npx : nullptr);
            if (rc) return rc;
        }
        HIPC(h, hipStreamSynchronize(h->stream));        // (one chunk holds 2^27 pixels: a study is one chunk; the event pair is read per chunk)
        HIPC(h, dev_time(h, 0, 1, tf_handle::DT_SALIENCY, true));
    }
    *dout = out;
    return TF_OK;
}

int saliency_frames(tf_handle* h, const uint8_t* host_frames, int N, int H, int W, int channels, bool f32, void* out)
{
    Src frames;
    const int args_rc = !out || N < 1 || H < 1 || W < 1 ? TF_ERR_INVALID_ARG : TF_OK;
    if (int rc = call_frames(h, "tf_saliency_frames", host_frames, N, H, W, channels, args_rc, &frames)) return rc;
    if (channels != 1 && channels != 3) return fail(h, TF_ERR_INVALID_ARG, "saliency: frames must have 1 or 3 channels, got %d", channels);
    const uint8_t* d = nullptr;
    int rc = saliency_to_device(h, frames, N, H, W, channels, f32, &d);
    if (rc) return rc;
    HIPC(h, hipMemcpy(out, d, (size_t)N * H * W * (f32 ? sizeof(float) : 1), hipMemcpyDeviceToHost));
    return TF_OK;
}
}  // namespace

TF_API int tf_saliency_frames(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, uint8_t* saliency_out)
{
    return finish_host_call(h, saliency_frames(h, frames, N, H, W, channels, false, saliency_out));
}
TF_API int tf_saliency_frames_f32(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, float* saliency_out)
{
    return finish_host_call(h, saliency_frames(h, frames, N, H, W, channels, true, saliency_out));
}

// ---- the held frames: a study's RGB frames put on the device once, in the form its file stores them, and read there by every
// frames-taking call armed with tf_frames_next (take_frames, above).  Separate from the held study (teeflow_held.hip.h): neither
// call touches the other's buffers.  Everything runs on the handle's stream (tf_set_stream included) and is waited for. --------------------
namespace {
// nothing queued anywhere still reads the held frames: the handle's stream, and tf_segmentor_input's kernel on a caller's stream
int frames_quiesce(tf_handle* h)
{
    HIPC(h, hipSetDevice(h->dev));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (h->seg_ev[1]) HIPC(h, hipEventSynchronize(h->seg_ev[1]));
    return TF_OK;
}

// k_ingest over npx pixels of src (device): interleaved pixels (hw == 0), or sample planes [N][3][hw] (a grey frame's one plane is the
// frame: GRAY reads it as interleaved whatever hw says)
template <int FORM>
void launch_ingest(tf_handle* h, bool flip, const uint8_t* src, size_t npx, int W, size_t hw, uint8_t* out)
{
    const dim3 g((unsigned)(((npx + 3) / 4 + 255) / 256)), blk(256);
    if constexpr (FORM != tfg::GRAY)
        if (hw) {
            if (flip) hipLaunchKernelGGL((tfg::k_ingest_planar<FORM, true>), g, blk, 0, h->stream, src, npx, W, hw, out);
            else hipLaunchKernelGGL((tfg::k_ingest_planar<FORM, false>), g, blk, 0, h->stream, src, npx, W, hw, out);
            return;
        }
    if (flip) hipLaunchKernelGGL((tfg::k_ingest<FORM, true>), g, blk, 0, h->stream, src, npx, W, out);
    else hipLaunchKernelGGL((tfg::k_ingest<FORM, false>), g, blk, 0, h->stream, src, npx, W, out);
}

// The held frames' buffer made at least `bytes` large, and nothing held any more.  keep_if_refused: the new buffer is allocated
// before the old one goes, so a refused allocation leaves the held frames as they were (both buffers live for a moment); otherwise the
// old one goes first and the peak is one buffer.
int frames_buffer(tf_handle* h, size_t bytes, bool keep_if_refused, int N, int H, int W)
{
    tf_handle::Frames& k = h->frames;
    if (!keep_if_refused) k.drop();
    if (k.cap < bytes) {
        if (!keep_if_refused) { (void)hipFree(k.rgb); k.rgb = nullptr; k.cap = 0; }
        uint8_t* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, e == hipErrorOutOfMemory ? TF_ERR_NOMEM : TF_ERR_HIP, "holding frames of %d x %d x %d: hipMalloc failed: %s", N, H, W, hipGetErrorString(e));
        }
        (void)hipFree(k.rgb);
        k.rgb = p; k.cap = bytes;
    }
    k.drop();
    return TF_OK;
}

// The step every hold ends with, behind frames_buffer: dsrc (device; laid out as launch_ingest says) ingested into the held buffer
// between ev[0] and ev[1] -- or no kernel at all, dsrc null: the caller has queued a copy of RGB frames straight into the buffer --
// then the stream waited for, the ingest counters, the shape, the generation.
int frames_commit(tf_handle* h, const uint8_t* dsrc, size_t hw, int form, bool flip, int N, int H, int W)
{
    tf_handle::Frames& k = h->frames;
    const size_t npx = (size_t)N * H * W;
    h->dev_ms[tf_handle::DT_INGEST] = 0; h->ingest_bytes = 0;
    if (dsrc) {
        HIPC(h, hipEventRecord(h->ev[0], h->stream));
        if (form == TF_FRAMES_GRAY) launch_ingest<tfg::GRAY>(h, flip, dsrc, npx, W, hw, k.rgb);
        else if (form == TF_FRAMES_YBR_FULL) launch_ingest<tfg::YBR_FULL>(h, flip, dsrc, npx, W, hw, k.rgb);
        else if (form == tfg::YBR_LIBJPEG) launch_ingest<tfg::YBR_LIBJPEG>(h, flip, dsrc, npx, W, hw, k.rgb);   // (internal: tf_hold_frames_jpeg alone passes it)
        else launch_ingest<tfg::RGB>(h, flip, dsrc, npx, W, hw, k.rgb);
        HIPC(h, hipGetLastError());
        HIPC(h, hipEventRecord(h->ev[1], h->stream));
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    if (dsrc) {
        HIPC(h, dev_time(h, 0, 1, tf_handle::DT_INGEST, false));
        h->ingest_bytes = (long long)(npx * (form == TF_FRAMES_GRAY ? 1 : 3) + npx * 3);
    }
    k.N = N; k.H = H; k.W = W;
    ++k.gen;
    return TF_OK;
}

int hold_frames(tf_handle* h, const uint8_t* src, int form, bool flip, int N, int H, int W)
{
    int rc = frames_quiesce(h);
    if (rc) return rc;
    const size_t npx = (size_t)N * H * W, in_bytes = npx * (form == TF_FRAMES_GRAY ? 1 : 3);
    if ((rc = frames_buffer(h, npx * 3, false, N, H, W))) return rc;
    uint8_t* dsrc = nullptr;                                  // (RGB, no flip: nothing to compute, the upload is the held frames)
    if (form != TF_FRAMES_RGB || flip) {
        Pre pre(h);
        dsrc = pre.get<uint8_t>(tf_handle::PRE_FR_SRC, in_bytes);
        if (pre.rc) return pre.rc;
    }
    HIPC(h, hipMemcpyAsync(dsrc ? dsrc : h->frames.rgb, src, in_bytes, hipMemcpyHostToDevice, h->stream));
    h->frames_upload_bytes += (long long)in_bytes;
    return frames_commit(h, dsrc, 0, form, flip, N, H, W);
}
}  // namespace

TF_API int tf_hold_frames(tf_handle* h, const void* src, int form, int flip_lr, int N, int H, int W)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!src || N < 1 || H < 1 || W < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_hold_frames: null source or bad sizes: N=%d H=%d W=%d", N, H, W);
    if (form != TF_FRAMES_RGB && form != TF_FRAMES_GRAY && form != TF_FRAMES_YBR_FULL)
        return fail(h, TF_ERR_INVALID_ARG, "tf_hold_frames: form %d is none of TF_FRAMES_RGB (0), TF_FRAMES_GRAY (1), TF_FRAMES_YBR_FULL (2)", form);
    return finish_host_call(h, hold_frames(h, (const uint8_t*)src, form, flip_lr != 0, N, H, W));
}

TF_API int tf_held_frames_shape(tf_handle* h, long long* out)
{
    if (!h || !out) return TF_ERR_INVALID_ARG;
    const tf_handle::Frames& k = h->frames;
    out[0] = k.N; out[1] = k.H; out[2] = k.W; out[3] = k.gen;
    return TF_OK;
}

TF_API int tf_release_frames(tf_handle* h)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (int rc = frames_quiesce(h)) return rc;
    h->frames.release();
    return TF_OK;
}

TF_API int tf_download_frames(tf_handle* h, uint8_t* rgb_out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const tf_handle::Frames& k = h->frames;
    if (k.N < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_download_frames: no frames are held (tf_hold_frames)");
    if (!rgb_out) return fail(h, TF_ERR_INVALID_ARG, "tf_download_frames: null output pointer");
    auto run = [&]() -> int {
        HIPC(h, hipSetDevice(h->dev));
        HIPC(h, hipMemcpyAsync(rgb_out, k.rgb, (size_t)k.N * k.H * k.W * 3, hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        return TF_OK;
    };
    return finish_host_call(h, run());
}

TF_API int tf_frames_next(tf_handle* h, int first, int count)
{
    if (!h) return TF_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_frames_next_m);
    g_frames_next[h] = tf_handle::Armed{false, false, true, first, count};
    return TF_OK;
}

// ---- frames held from DICOM RLE Lossless pixel data (kernel: teeflow_rle.hip.h): the compressed bytes go up, k_rle_decode writes the
// sample planes into the handle's PRE_RLE_* scratch, and only a call whose every frame decoded touches the held frames -----------------
namespace {
constexpr uint32_t RLE_MAX_PLANE = 1u << 30;                  // H * W
constexpr uint32_t RLE_MAX_FRAME = 0xFFFFF000u;               // a frame's bytes: the kernel's 32-bit positions, do not wrap

const char* rle_status_text(int s)
{
    static const char* const text[] = {"ok", "bad header", "bad offsets", "a segment decoded short"};
    return s >= 0 && s <= 3 ? text[s] : "unknown status";
}

struct RleJob {
    tfs::Batch in; int H, W, samples;                         // the frames (checked: rle_check; in.n of them) and their shape
    size_t plane() const { return (size_t)H * W; }
};

// before any GPU work
int rle_check(tf_handle* h, const char* who, RleJob& j)
{
    if (j.in.n < 1 || j.H < 1 || j.W < 1) return fail(h, TF_ERR_INVALID_ARG, "%s: bad sizes: N=%d H=%d W=%d", who, j.in.n, j.H, j.W);
    if (j.samples != 1 && j.samples != 3) return fail(h, TF_ERR_INVALID_ARG, "%s: samples must be 1 or 3, got %d", who, j.samples);
    if ((double)j.H * j.W > RLE_MAX_PLANE) return fail(h, TF_ERR_INVALID_ARG, "%s: a plane of %d x %d bytes, at most %u", who, j.H, j.W, RLE_MAX_PLANE);
    if ((double)j.in.n * j.samples > std::numeric_limits<int>::max()) return fail(h, TF_ERR_INVALID_ARG, "%s: %d frames of %d segments", who, j.in.n, j.samples);
    return streams_check(h, who, j.in, RLE_MAX_FRAME, "frame");
}

// what a launched decode left on the device (valid once the handle's stream has run it)
struct RleDecoded {
    const uint8_t* planes = nullptr;                          // [N][samples][H * W]
    int* status = nullptr;                                    // [N]
    tfs::Table table;                                         // the host side of the per-frame table: lives until the stream is waited for
};

// The frames of j onto the device and k_rle_decode behind them on the handle's stream, between ev[0] and ev[1]; not waited for.
int rle_launch(tf_handle* h, const RleJob& j, RleDecoded* r)
{
    const size_t n = (size_t)j.in.n;
    enum { OFF, LEN, STATUS };                                // off [n] u64 | len [n] u32 | status [n] i32
    r->table = tfs::table(j.in, {8, 4, 4}, OFF, LEN);
    Pre pre(h);
    auto* dplanes = pre.get<uint8_t>(tf_handle::PRE_RLE_PLANES, n * j.samples * j.plane());
    if (pre.rc) return pre.rc;
    const uint8_t* dblob = nullptr; uint8_t* dtab = nullptr;
    if (int rc = streams_upload(h, j.in, r->table, tf_handle::PRE_RLE_BLOB, tf_handle::PRE_RLE_TABLE, &tf_handle::frames_upload_bytes, &dblob, &dtab)) return rc;
    const auto& at = r->table.at;
    r->planes = dplanes; r->status = (int*)(dtab + at[STATUS]);
    h->dev_ms[tf_handle::DT_RLE] = 0; h->rle_bytes = 0;
    HIPC(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(k_rle_decode, dim3((unsigned)(n * j.samples)), dim3(64), 0, h->stream, dblob, (const unsigned long long*)(dtab + at[OFF]),
                       (const uint32_t*)(dtab + at[LEN]), j.in.n, j.samples, (uint32_t)j.plane(), dplanes, r->status);
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(h->ev[1], h->stream));
    return TF_OK;
}

// after the stream has been waited for: the kernel's device time and bytes into the handle's counters
void rle_counters(tf_handle* h, const RleJob& j)
{
    (void)dev_time(h, 0, 1, tf_handle::DT_RLE, false);
    h->rle_bytes = (long long)j.in.bytes() + (long long)((size_t)j.in.n * j.samples * j.plane());
}

int rle_decode(tf_handle* h, const RleJob& j, uint8_t* out_host, int* status)
{
    HIPC(h, hipSetDevice(h->dev));
    RleDecoded r;
    if (int rc = rle_launch(h, j, &r)) return rc;
    const int N = j.in.n;
    const size_t npx = (size_t)N * j.plane(), frame_bytes = j.plane() * j.samples;
    const uint8_t* dout = r.planes;                           // (one plane a frame is the frame)
    if (j.samples == 3) {
        Pre pre(h);
        auto* d = pre.get<uint8_t>(tf_handle::PRE_RLE_OUT, npx * 3);
        if (pre.rc) return pre.rc;
        launch_ingest<tfg::RGB>(h, false, r.planes, npx, j.W, j.plane(), d);   // (a frame that failed: whatever its planes hold; not copied out)
        HIPC(h, hipGetLastError());
        dout = d;
    }
    HIPC(h, hipMemcpyAsync(status, r.status, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    rle_counters(h, j);
    bool all = true;
    for (int i = 0; i < N && all; ++i) all = status[i] == 0;
    if (all) HIPC(h, hipMemcpyAsync(out_host, dout, (size_t)N * frame_bytes, hipMemcpyDeviceToHost, h->stream));
    else
        for (int i = 0; i < N; ++i)
            if (status[i] == 0) HIPC(h, hipMemcpyAsync(out_host + (size_t)i * frame_bytes, dout + (size_t)i * frame_bytes, frame_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    return streams_verdict(h, "tf_rle_decode", "frame", "decode", rle_status_text, status, N);
}

int hold_frames_rle(tf_handle* h, const RleJob& j, int form, bool flip, int* status_out)
{
    int rc = frames_quiesce(h);
    if (rc) return rc;
    RleDecoded r;
    if ((rc = rle_launch(h, j, &r))) return rc;
    std::vector<int> status((size_t)j.in.n);
    HIPC(h, hipMemcpyAsync(status.data(), r.status, status.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    rle_counters(h, j);
    if (status_out) memcpy(status_out, status.data(), status.size() * sizeof(int));
    if ((rc = streams_verdict(h, "tf_hold_frames_rle", "frame", "decode", rle_status_text, status.data(), j.in.n))) return rc;
    // every frame decoded: only now are the held frames touched, the decoded planes being the source
    if ((rc = frames_buffer(h, (size_t)j.in.n * j.plane() * 3, true, j.in.n, j.H, j.W))) return rc;
    return frames_commit(h, r.planes, j.plane(), form, flip, j.in.n, j.H, j.W);
}
}  // namespace

TF_API int tf_rle_stage_bytes(void) { return (int)rle::STAGE; }

TF_API int tf_rle_decode(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                         uint8_t* out_host, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    RleJob j{{blob, off, len, N}, H, W, samples};
    if (int rc = rle_check(h, "tf_rle_decode", j)) return rc;
    if (!out_host || !status) return fail(h, TF_ERR_INVALID_ARG, "tf_rle_decode: null out_host or status");
    return finish_host_call(h, rle_decode(h, j, out_host, status));
}

TF_API int tf_hold_frames_rle(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                              int form, int flip_lr, int* status)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const char* who = "tf_hold_frames_rle";
    if (form != TF_FRAMES_RGB && form != TF_FRAMES_GRAY && form != TF_FRAMES_YBR_FULL)
        return fail(h, TF_ERR_INVALID_ARG, "%s: form %d is none of TF_FRAMES_RGB (0), TF_FRAMES_GRAY (1), TF_FRAMES_YBR_FULL (2)", who, form);
    if (samples != (form == TF_FRAMES_GRAY ? 1 : 3))
        return fail(h, TF_ERR_INVALID_ARG, "%s: form %d has %d samples a pixel, got samples = %d", who, form, form == TF_FRAMES_GRAY ? 1 : 3, samples);
    RleJob j{{blob, off, len, N}, H, W, samples};
    if (int rc = rle_check(h, who, j)) return rc;
    return finish_host_call(h, hold_frames_rle(h, j, form, flip_lr != 0, status));
}
