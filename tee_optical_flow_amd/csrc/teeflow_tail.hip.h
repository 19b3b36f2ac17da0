// The study tail's host code: everything around the solver -- frame conditioning, saliency, tf_clean_masks, tf_otsu_masks, the
// segmentor's frame glue, tf_av_centroids, tf_first_region_areas, the rad/long and polar projections, histogram and radix select, the two overlays, WASE, the study calls.  Included by teeflow.hip (one
// translation unit); the kernels are in the kernel headers.  The entry points here keep their device scratch in the handle's PRE_*
// slots (grown on demand, never shrunk, freed with the handle), so they neither allocate nor free once a study's sizes have been seen.
// The one exception is tf_submit_seq_rgb, whose conditioned frames are a buffer of the queued job (allocated per study, freed with it).

namespace {
int pre_grow(tf_handle* h, int which, size_t bytes, void** out)
{
    tf_handle::GrowBuf& b = h->pre[which];
    if (b.cap < bytes) {
        if (b.p) { HIPC(h, hipStreamSynchronize(h->stream)); (void)hipFree(b.p); }
        b.p = nullptr; b.cap = 0;
        HIPC(h, hipMalloc(&b.p, bytes));
        b.cap = bytes;
    }
    *out = b.p;
    return TF_OK;
}

// typed access to the slots; latches the first error (get() gives nullptr from then on), to be checked once after the last get()
struct Pre {
    tf_handle* h;
    int rc = TF_OK;
    explicit Pre(tf_handle* h_) : h(h_) {}
    template <typename T>
    T* get(int which, size_t count)
    {
        void* p = nullptr;
        if (rc == TF_OK) rc = pre_grow(h, which, count * sizeof(T), &p);
        return (T*)p;
    }
};

// a failed call leaves nothing of it running: its destinations are host memory the caller may free at once
// (a call refused for its null handle passes through)
int finish_host_call(tf_handle* h, int rc)
{
    if (rc != TF_OK && h) {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        (void)hipGetLastError();
    }
    return rc;
}

// A study goes through the chunked calls in chunks of as many frames as fit in `budget` bytes of per-chunk scratch: at most N (and
// `cap`, where a chunk's planes are a grid dimension), at least 1.  The walk is the same everywhere:
//     for (int f0 = 0; f0 < N; f0 += nf) { const int n = std::min(nf, N - f0); ... frames [f0, f0 + n) ... }
constexpr size_t MASK_CHUNK_BYTES = (size_t)512 << 20;

int chunk_frames(size_t bytes_per_frame, int N, size_t cap = 65535, size_t budget = MASK_CHUNK_BYTES)
{
    const size_t nf = std::min({budget / bytes_per_frame, (size_t)N, cap});
    return nf < 1 ? 1 : (int)nf;
}

// the start values of `pairs` (min, max) key pairs; the caller keeps them alive until the stream has run their upload
std::vector<u64> minmax_seed(size_t pairs)
{
    std::vector<u64> init(pairs * 2);
    for (size_t i = 0; i < pairs; ++i) { init[2 * i] = ~0ull; init[2 * i + 1] = 0ull; }
    return init;
}

// Where a tail call finds its flow, its mask or its echo: host memory, which the call uploads into its scratch, or device memory
// that already holds it (a held study's buffers, teeflow_held.hip.h), which the call's kernels read where it is.
struct Src {
    const void* host = nullptr; const void* dev = nullptr;
    static Src on_host(const void* p) { return {p, nullptr}; }
    static Src on_device(const void* p) { return {nullptr, p}; }
};

// bytes [off, off + bytes) of src, on the device: *out is the resident bytes themselves, or `scratch` behind their upload on the
// handle's stream (counted in tail_upload_bytes)
int src_to_device(tf_handle* h, const Src& src, size_t off, size_t bytes, void* scratch, const uint8_t** out)
{
    if (src.dev) { *out = (const uint8_t*)src.dev + off; return TF_OK; }
    HIPC(h, hipMemcpyAsync(scratch, (const uint8_t*)src.host + off, bytes, hipMemcpyHostToDevice, h->stream));
    h->tail_upload_bytes += (long long)bytes;
    *out = (const uint8_t*)scratch;
    return TF_OK;
}

// The RGB frames of a frames-taking call named `who`: the caller's host pointer, or -- armed by tf_frames_next, `a` being what
// spend_frames_next gave the call at its start -- frames [first, first + count) of the held frames where they are
// (teeflow_held.hip.h).  The armed call passes a null pointer, N == count, three channels and the held H x W; anything else is
// refused with both shapes.  Called once the call's own argument checks have passed: this reads the handle.
int take_frames(tf_handle* h, const char* who, const ArmedFrames& a, const void* rgb, int N, int H, int W, int channels, Src* out)
{
    if (!a.on) { *out = Src::on_host(rgb); return TF_OK; }
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

// src_to_device for a call's frames: what is uploaded counts in frames_upload_bytes
int frames_to_device(tf_handle* h, const Src& src, size_t off, size_t bytes, void* scratch, const uint8_t** out)
{
    if (src.dev) { *out = (const uint8_t*)src.dev + off; return TF_OK; }
    HIPC(h, hipMemcpyAsync(scratch, (const uint8_t*)src.host + off, bytes, hipMemcpyHostToDevice, h->stream));
    h->frames_upload_bytes += (long long)bytes;
    *out = (const uint8_t*)scratch;
    return TF_OK;
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
    if (int rc = frames_to_device(h, rgb, 0, (size_t)N * npx * 3, urgb, &drgb)) return rc;
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
    if (!h) return TF_ERR_INVALID_ARG;
    const ArmedFrames armed = spend_frames_next(h);
    if ((!rgb && !armed.on) || !gray_out || N < 1 || H < 1 || W < 1) return TF_ERR_INVALID_ARG;
    Src fr;
    if (int rc = take_frames(h, "tf_condition_frames", armed, rgb, N, H, W, 3, &fr)) return rc;
    return finish_host_call(h, condition_frames(h, fr, N, H, W, gray_out));
}

// the echo alone: rgb uint8 [N][H][W][3] -> float16 [N][H][W] = half(rgb2gray), one rounding
TF_API int tf_echo_frames(tf_handle* h, const uint8_t* rgb, int N, int H, int W, uint16_t* echo16_out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const ArmedFrames armed = spend_frames_next(h);
    if ((!rgb && !armed.on) || !echo16_out || N < 1 || H < 1 || W < 1) return TF_ERR_INVALID_ARG;
    Src fr;
    if (int rc = take_frames(h, "tf_echo_frames", armed, rgb, N, H, W, 3, &fr)) return rc;
    const size_t n = (size_t)N * H * W;
    auto run = [&]() -> int {
        HIPC(h, hipSetDevice(h->dev));
        Pre pre(h);
        auto* urgb = fr.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_SRC, n * 3);
        auto* decho = pre.get<uint16_t>(tf_handle::PRE_ECHO, n);
        if (pre.rc) return pre.rc;
        const uint8_t* drgb = nullptr;
        int rc = frames_to_device(h, fr, 0, n * 3, urgb, &drgb);
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
    h->pre_kernel_ms = 0;
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int n = std::min(nf, N - f0);
        const size_t px = (size_t)n * npx;
        const dim3 g2((W + 255) / 256, H, n), blk(256);
        const uint8_t* src = nullptr;
        if (int rc = frames_to_device(h, frames, f0 * npx * channels, px * channels, usrc, &src)) return rc;
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
        float t = 0;
        HIPC(h, hipEventElapsedTime(&t, h->ev[0], h->ev[1]));
        h->pre_kernel_ms += t;
    }
    *dout = out;
    return TF_OK;
}

int saliency_frames(tf_handle* h, const uint8_t* host_frames, int N, int H, int W, int channels, bool f32, void* out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const ArmedFrames armed = spend_frames_next(h);
    if ((!host_frames && !armed.on) || !out || N < 1 || H < 1 || W < 1) return TF_ERR_INVALID_ARG;
    Src frames;
    if (int rc = take_frames(h, "tf_saliency_frames", armed, host_frames, N, H, W, channels, &frames)) return rc;
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

namespace {
// One labelling of `planes` planes of H x W (teeflow_ccl.hip.h): the set's components, CONN-connected, each pixel's root in dpar and
// what `acc` collects per root in its totals.  dlr is written only with LR and read only by an accumulator that counts per tile.
// The totals are zeroed after the local kernel: the masks' second set reads the first labelling's flags from the words its sizes go to.
template <int CONN, bool LR, typename Set, typename Acc>
int label_planes(tf_handle* h, const Set& set, const Acc& acc, size_t planes, int H, int W, uint32_t* dpar, uint16_t* dlr, unsigned* derr)
{
    using namespace ccl;
    const int tiles_x = (W + TW - 1) / TW, tiles = tiles_x * ((H + TH - 1) / TH);
    const dim3 g(tiles, (unsigned)planes), blk(256);
    const hipStream_t s = h->stream;
    hipLaunchKernelGGL((k_ccl_local<CONN, LR, Set>), g, blk, 0, s, set, dpar, dlr, H, W, tiles_x, derr);
    HIPC(h, acc.clear(planes * H * W, s));
    hipLaunchKernelGGL(k_ccl_merge<CONN>, g, blk, 0, s, dpar, H, W, tiles_x, derr);
    hipLaunchKernelGGL(k_ccl_flatten<Acc>, g, blk, 0, s, dpar, dlr, acc, H, W, tiles_x);
    return TF_OK;
}

// The two labellings tf_clean_masks and tf_otsu_masks share, on planes whose background is `set`: fill holes (components of the
// background; those with a pixel on the border keep their flag in daux), then small objects (components of the filled mask, their
// sizes counted into daux).  Leaves each pixel's root in dpar and each root's component size in daux (10 B of scratch per pixel and plane).
template <typename Set>
int fill_and_size_planes(tf_handle* h, const Set& set, size_t planes, int H, int W, uint32_t* dpar, uint32_t* daux, uint16_t* dlr, unsigned* derr)
{
    int rc = label_planes<4, false>(h, set, msk::BorderFlag{daux}, planes, H, W, dpar, dlr, derr);
    if (rc) return rc;
    return label_planes<4, true>(h, msk::FilledByLabels{dpar, daux, (size_t)H * W}, msk::ComponentSize{daux}, planes, H, W, dpar, dlr, derr);
}

// the labelling's error word, read back behind what the caller has queued on the stream; waits for the stream
int label_errors(tf_handle* h, const unsigned* derr, const char* who)
{
    unsigned e = 0;
    HIPC(h, hipMemcpyAsync(&e, derr, sizeof e, hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (e) return fail(h, TF_ERR_HIP, "%s: a union-find loop ran out of its bound (code %u)", who, e);
    return TF_OK;
}

// tf_clean_masks: frames go through in chunks so that the per-chunk scratch (10 B per pixel and label, 2 B per pixel and label + 1 of
// output) stays within MASK_CHUNK_BYTES whatever the study's length; the class map itself (1 B per pixel) is uploaded whole.
int clean_masks(tf_handle* h, const uint8_t* cmap, int N, int H, int W, const uint8_t* ids, int L, long long min_size, uint8_t* out)
{
    using namespace msk;
    const size_t HW = (size_t)H * W;
    if (HW > 0x7fffffffu) return fail(h, TF_ERR_UNSUPPORTED, "tf_clean_masks: at most 2^31 - 1 pixels per frame");
    if (L > 65535) return fail(h, TF_ERR_UNSUPPORTED, "tf_clean_masks: at most 65535 labels");
    const int nf = chunk_frames(HW * (10 * (size_t)L + 2 * ((size_t)L + 1)), N, 65535 / L);   // planes of a chunk are grid.y
    HIPC(h, hipSetDevice(h->dev));
    Pre pre(h);
    auto* dcls = pre.get<uint8_t>(tf_handle::PRE_MK_CLS, (size_t)N * HW);
    auto* dpar = pre.get<uint32_t>(tf_handle::PRE_LB_PAR, (size_t)L * nf * HW);
    auto* daux = pre.get<uint32_t>(tf_handle::PRE_LB_AUX, (size_t)L * nf * HW);
    auto* dlr = pre.get<uint16_t>(tf_handle::PRE_LB_LR, (size_t)L * nf * HW);
    auto* dout = pre.get<uint16_t>(tf_handle::PRE_MK_OUT, (size_t)(L + 1) * nf * HW);
    auto* meta = pre.get<uint8_t>(tf_handle::PRE_MK_META, 64 + (size_t)L);   // [0, 4): error word, [64, 64 + L): class ids
    if (pre.rc) return pre.rc;
    unsigned* derr = (unsigned*)meta;
    const hipStream_t s = h->stream;
    HIPC(h, hipMemcpyAsync(dcls, cmap, (size_t)N * HW, hipMemcpyHostToDevice, s));
    HIPC(h, hipMemcpyAsync(meta + 64, ids, (size_t)L, hipMemcpyHostToDevice, s));
    HIPC(h, hipMemsetAsync(derr, 0, sizeof(unsigned), s));
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int n = std::min(nf, N - f0);
        int rc = fill_and_size_planes(h, ClassWindowBackground{dcls, meta + 64, N, f0, n, HW}, (size_t)L * n, H, W, dpar, daux, dlr, derr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mask_store, dim3((unsigned)((HW + 255) / 256), (unsigned)n), dim3(256), 0, s, dpar, daux, L, n, HW, min_size, dout);
        HIPC(h, hipGetLastError());
        for (int l = 0; l <= L; ++l)                           // label l's frames of this chunk are contiguous in masks_out
            HIPC(h, hipMemcpyAsync(out + ((size_t)l * N + f0) * HW * 2, dout + (size_t)l * n * HW, (size_t)n * HW * 2, hipMemcpyDeviceToHost, s));
        rc = label_errors(h, derr, "tf_clean_masks");
        if (rc) return rc;
    }
    return TF_OK;
}
}  // namespace

TF_API int tf_clean_masks(tf_handle* h, const uint8_t* class_map, int N, int H, int W, const uint8_t* class_ids, int n_labels, long long min_size,
                          uint8_t* masks_out)
{
    if (!h || !class_map || !class_ids || !masks_out || N < 1 || H < 1 || W < 1 || n_labels < 1) return TF_ERR_INVALID_ARG;
    return finish_host_call(h, clean_masks(h, class_map, N, H, W, class_ids, n_labels, min_size, masks_out));
}

namespace {
// The three launches tf_otsu_masks opens with (tf_dbg_luma_stats runs them alone and downloads what they leave): per-frame min / max of
// the luma, its 256-bin histogram, Otsu's threshold.  mm: [N][2], seeded by minmax_seed; dhist: [N][256], zeroed; dthr: [N].
void otsu_luma_stats(const uint8_t* drgb, int N, size_t HW, u64* mm, uint32_t* dhist, double* dthr, hipStream_t s)
{
    const dim3 blk(256);
    const unsigned gx = (unsigned)((HW + 255) / 256), gr = gx < 512 ? gx : 512;
    hipLaunchKernelGGL(k_cond_minmax, dim3(gr, N), blk, 0, s, drgb, HW, mm);
    hipLaunchKernelGGL(otsu::k_otsu_hist, dim3(gr, N), blk, 0, s, drgb, HW, mm, dhist);
    hipLaunchKernelGGL(otsu::k_otsu_thr, dim3(N), blk, 0, s, mm, dhist, dthr);
}

// tf_otsu_masks: the frames, one byte per pixel of the cleaned planes and the output stay on the device for the whole study (6 B per
// pixel and frame); the labelling scratch (10 B per pixel and frame: parents, flags / sizes, tile-local roots) is the PRE_LB_* slots
// that every labelling call uses, in chunks of as many frames as fit in MASK_CHUNK_BYTES.  The temporal window runs over all cleaned planes after the last chunk.
int otsu_masks(tf_handle* h, const Src& rgb, int N, int H, int W, long long min_size, uint8_t* out, double* thr_out)
{
    const size_t HW = (size_t)H * W;
    const int nf = chunk_frames(HW * 10, N);
    HIPC(h, hipSetDevice(h->dev));
    // meta: [0, 64) error word; then min / max [N][2] u64, thresholds [N] f64, histograms [N][256] u32
    const size_t off_mm = 64, off_thr = off_mm + (size_t)N * 16, off_hist = off_thr + (size_t)N * 8, meta_bytes = off_hist + (size_t)N * otsu::NBINS * 4;
    Pre pre(h);
    auto* urgb = rgb.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_OT_RGB, (size_t)N * HW * 3);
    auto* dclean = pre.get<uint8_t>(tf_handle::PRE_OT_CLEAN, (size_t)N * HW);
    auto* dout = pre.get<uint16_t>(tf_handle::PRE_OT_OUT, (size_t)N * HW);
    auto* meta = pre.get<uint8_t>(tf_handle::PRE_OT_META, meta_bytes);
    auto* dpar = pre.get<uint32_t>(tf_handle::PRE_LB_PAR, (size_t)nf * HW);
    auto* daux = pre.get<uint32_t>(tf_handle::PRE_LB_AUX, (size_t)nf * HW);
    auto* dlr = pre.get<uint16_t>(tf_handle::PRE_LB_LR, (size_t)nf * HW);
    if (pre.rc) return pre.rc;
    unsigned* derr = (unsigned*)meta;
    u64* mm = (u64*)(meta + off_mm);
    double* dthr = (double*)(meta + off_thr);
    uint32_t* dhist = (uint32_t*)(meta + off_hist);
    const hipStream_t s = h->stream;
    const std::vector<u64> init = minmax_seed((size_t)N);
    const uint8_t* drgb = nullptr;
    if (int rc = frames_to_device(h, rgb, 0, (size_t)N * HW * 3, urgb, &drgb)) return rc;
    HIPC(h, hipMemsetAsync(meta, 0, meta_bytes, s));
    HIPC(h, hipMemcpyAsync(mm, init.data(), init.size() * sizeof(u64), hipMemcpyHostToDevice, s));
    const dim3 blk(256);
    const unsigned gx = (unsigned)((HW + 255) / 256);
    otsu_luma_stats(drgb, N, HW, mm, dhist, dthr, s);
    for (int f0 = 0; f0 < N; f0 += nf) {                       // one plane per frame
        const int n = std::min(nf, N - f0);
        int rc = fill_and_size_planes(h, otsu::LumaNotAbove{drgb, dthr, f0, HW}, (size_t)n, H, W, dpar, daux, dlr, derr);
        if (rc) return rc;
        hipLaunchKernelGGL(otsu::k_otsu_keep, dim3(gx, (unsigned)n), blk, 0, s, dpar, daux, HW, min_size, dclean + (size_t)f0 * HW);
        HIPC(h, hipGetLastError());
    }
    hipLaunchKernelGGL(otsu::k_otsu_window, dim3(gx, N), blk, 0, s, dclean, N, HW, dout);
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(out, dout, (size_t)N * HW * 2, hipMemcpyDeviceToHost, s));
    if (thr_out) HIPC(h, hipMemcpyAsync(thr_out, dthr, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    return label_errors(h, derr, "tf_otsu_masks");
}
}  // namespace

TF_API int tf_otsu_masks(tf_handle* h, const uint8_t* rgb, int N, int H, int W, long long min_size, uint8_t* masks_out, double* thresholds_out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const ArmedFrames armed = spend_frames_next(h);
    if ((!rgb && !armed.on) || !masks_out || N < 2 || H < 2 || W < 2) return TF_ERR_INVALID_ARG;
    if ((size_t)H * W > 0x7fffffffu || N > 65535) return TF_ERR_UNSUPPORTED;   // (frames are a grid dimension)
    Src fr;
    if (int rc = take_frames(h, "tf_otsu_masks", armed, rgb, N, H, W, 3, &fr)) return rc;
    return finish_host_call(h, otsu_masks(h, fr, N, H, W, min_size, masks_out, thresholds_out));
}

namespace {
// tf_segmentor_input: tables, LUT and frames travel as ONE block -- written into pinned staging, copied to device scratch of the same
// layout, read by the kernel -- so the call returns with everything queued on `s`.  Layout, in 4-byte words: x bounds [ow][2], x
// coefficients [ow][kxs], y bounds [oh][2], y coefficients [oh][kys], LUT [3][256]; then, 256-byte aligned, the frames -- unless they are
// the held frames, which the kernel reads where they are: then the block is its head alone.
int segmentor_input(tf_handle* h, const Src& rgb, int N, int H, int W, int oh, int ow, const float* lut, float* d_out, hipStream_t s)
{
    HIPC(h, hipSetDevice(h->dev));
    int kxs = 0, kys = 0;
    std::vector<int> bx, cx, by, cy;
    pil_bilinear_tables(W, ow, kxs, bx, cx);
    pil_bilinear_tables(H, oh, kys, by, cy);
    const size_t off_cx = bx.size(), off_by = off_cx + cx.size(), off_cy = off_by + by.size(), off_lut = off_cy + cy.size();
    const size_t head = ((off_lut + 3 * 256) * 4 + 255) / 256 * 256, frames = rgb.dev ? 0 : (size_t)N * H * W * 3, total = head + frames;
    for (auto& ev : h->seg_ev) if (!ev) HIPC(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPC(h, hipEventSynchronize(h->seg_ev[0]));          // the last call's upload has left the staging
    if (h->seg_stage_cap < total) {
        if (h->seg_stage) (void)hipHostFree(h->seg_stage);
        h->seg_stage = nullptr; h->seg_stage_cap = 0;
        HIPC(h, hipHostMalloc(&h->seg_stage, total, hipHostMallocDefault));
        h->seg_stage_cap = total;
    }
    int* st = (int*)h->seg_stage;
    memcpy(st, bx.data(), bx.size() * 4);
    memcpy(st + off_cx, cx.data(), cx.size() * 4);
    memcpy(st + off_by, by.data(), by.size() * 4);
    memcpy(st + off_cy, cy.data(), cy.size() * 4);
    memcpy(st + off_lut, lut, 3 * 256 * 4);
    if (frames) memcpy((uint8_t*)h->seg_stage + head, rgb.host, frames);
    h->frames_upload_bytes += (long long)frames;
    if (h->pre[tf_handle::PRE_SG_IN].cap < total) HIPC(h, hipEventSynchronize(h->seg_ev[1]));   // (growing frees what the last kernel reads)
    Pre pre(h);
    auto* din = pre.get<uint8_t>(tf_handle::PRE_SG_IN, total);
    if (pre.rc) return pre.rc;
    HIPC(h, hipStreamWaitEvent(s, h->seg_ev[1], 0));     // the last call's kernel, on whichever stream it ran, is done with the scratch
    HIPC(h, hipMemcpyAsync(din, h->seg_stage, total, hipMemcpyHostToDevice, s));
    HIPC(h, hipEventRecord(h->seg_ev[0], s));
    const int* dt = (const int*)din;
    const seg::Axis ax{dt, dt + off_cx, kxs}, ay{dt + off_by, dt + off_cy, kys};
    const float* dlut = (const float*)(dt + off_lut);
    const unsigned gx = (unsigned)(((size_t)oh * ((ow + 3) / 4) + 255) / 256);
    const size_t fin = (size_t)H * W * 3, fout = (size_t)3 * oh * ow;
    const uint8_t* dfr = rgb.dev ? (const uint8_t*)rgb.dev : din + head;
    for (int f0 = 0; f0 < N; f0 += 65535) {              // frames are a grid dimension
        const dim3 g(gx, (unsigned)std::min(65535, N - f0)), blk(256);
        if (ow % 4 == 0) hipLaunchKernelGGL(seg::k_seg_input<true>, g, blk, 0, s, dfr + f0 * fin, H, W, oh, ow, ax, ay, dlut, d_out + f0 * fout);
        else hipLaunchKernelGGL(seg::k_seg_input<false>, g, blk, 0, s, dfr + f0 * fin, H, W, oh, ow, ax, ay, dlut, d_out + f0 * fout);
    }
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(h->seg_ev[1], s));
    return TF_OK;
}

int segmentor_classmap(tf_handle* h, const float* d_logits, int N, int C, int hh, int ww, int H, int W, uint8_t* out, hipStream_t s)
{
    HIPC(h, hipSetDevice(h->dev));
    std::vector<int> iy, ix;
    pil_nearest_table(hh, H, iy);
    pil_nearest_table(ww, W, ix);
    const size_t HW = (size_t)H * W;
    Pre pre(h);
    auto* didx = pre.get<int>(tf_handle::PRE_SG_IDX, (size_t)H + W);
    auto* dmap = pre.get<uint8_t>(tf_handle::PRE_SG_MAP, (size_t)N * HW);
    if (pre.rc) return pre.rc;
    HIPC(h, hipMemcpyAsync(didx, iy.data(), (size_t)H * 4, hipMemcpyHostToDevice, s));
    HIPC(h, hipMemcpyAsync(didx + H, ix.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
    for (int f0 = 0; f0 < N; f0 += 65535) {              // frames are a grid dimension
        const dim3 g((unsigned)((HW + 255) / 256), (unsigned)std::min(65535, N - f0)), blk(256);
        hipLaunchKernelGGL(seg::k_seg_classmap, g, blk, 0, s, d_logits + (size_t)f0 * C * hh * ww, C, hh, ww, H, W, didx, didx + H, dmap + f0 * HW);
    }
    HIPC(h, hipGetLastError());
    HIPC(h, hipMemcpyAsync(out, dmap, (size_t)N * HW, hipMemcpyDeviceToHost, s));
    HIPC(h, hipStreamSynchronize(s));                     // (iy, ix leave scope; the map is the caller's host memory)
    return TF_OK;
}

// a failed call leaves nothing of it running on the caller's stream either
int finish_stream_call(hipStream_t s, int rc)
{
    if (rc != TF_OK) {
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
    }
    return rc;
}
}  // namespace

TF_API int tf_segmentor_input(tf_handle* h, const uint8_t* rgb, int N, int H, int W, int out_h, int out_w, const float* lut, float* d_out,
                              void* hip_stream)
{
    if (!h) return TF_ERR_INVALID_ARG;
    const ArmedFrames armed = spend_frames_next(h);
    if ((!rgb && !armed.on) || !lut || !d_out || N < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) return TF_ERR_INVALID_ARG;
    if ((size_t)H * W > 0x7fffffffu || (size_t)out_h * out_w > 0x7fffffffu) return TF_ERR_UNSUPPORTED;
    Src fr;
    if (int rc = take_frames(h, "tf_segmentor_input", armed, rgb, N, H, W, 3, &fr)) return rc;
    const hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    return finish_stream_call(s, segmentor_input(h, fr, N, H, W, out_h, out_w, lut, d_out, s));
}

TF_API int tf_segmentor_classmap(tf_handle* h, const float* d_logits, int N, int C, int hh, int ww, int H, int W, uint8_t* class_map_out,
                                 void* hip_stream)
{
    if (!h || !d_logits || !class_map_out || N < 1 || C < 1 || hh < 1 || ww < 1 || H < 1 || W < 1) return TF_ERR_INVALID_ARG;
    if (C > 256 || (size_t)hh * ww > 0x7fffffffu || (size_t)H * W > 0x7fffffffu) return TF_ERR_UNSUPPORTED;
    const hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    return finish_stream_call(s, segmentor_classmap(h, d_logits, N, C, hh, ww, H, W, class_map_out, s));
}

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
// tf_av_centroids: frames go through in chunks so that the per-chunk scratch (26 B per pixel + the mask bytes: 10 B of them the
// PRE_LB_* slots every labelling call uses, the areas in the sizes' place) stays within MASK_CHUNK_BYTES whatever the study's length
int av_centroids(tf_handle* h, const Src& masks, int N, int H, int W, int C, double* cent_out, long long* area_out)
{
    using namespace cen;
    const size_t HW = (size_t)H * W;
    if (HW > 0x7fffffffu) return fail(h, TF_ERR_UNSUPPORTED, "tf_av_centroids: at most 2^31 - 1 pixels per frame");
    const int nf = chunk_frames(HW * (26 + (size_t)C), N);     // frames of a chunk are grid.y
    HIPC(h, hipSetDevice(h->dev));
    Pre pre(h);
    auto* um = masks.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_CT_MASK, (size_t)nf * HW * C);
    auto* dpar = pre.get<uint32_t>(tf_handle::PRE_LB_PAR, (size_t)nf * HW);
    auto* dlr = pre.get<uint16_t>(tf_handle::PRE_LB_LR, (size_t)nf * HW);
    auto* darea = pre.get<uint32_t>(tf_handle::PRE_LB_AUX, (size_t)nf * HW);
    auto* dsum = pre.get<unsigned long long>(tf_handle::PRE_CT_SUM, (size_t)nf * HW * 2);
    auto* out = pre.get<uint8_t>(tf_handle::PRE_CT_OUT, 64 + (size_t)N * 24);   // [0, 64): error word, then centroids [N][2] f64, then areas [N] i64
    if (pre.rc) return pre.rc;
    unsigned* derr = (unsigned*)out;
    double* dcent = (double*)(out + 64);
    long long* dar = (long long*)(out + 64 + (size_t)N * 16);
    const hipStream_t s = h->stream;
    HIPC(h, hipMemsetAsync(derr, 0, sizeof(unsigned), s));
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int n = std::min(nf, N - f0);
        const uint8_t* dm = nullptr;
        int rc = src_to_device(h, masks, (size_t)f0 * HW * C, (size_t)n * HW * C, um, &dm);
        if (rc) return rc;
        rc = label_planes<8, true>(h, ChannelZeroSet{dm, C, HW}, AreaAndSums{darea, dsum}, (size_t)n, H, W, dpar, dlr, derr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cent_pick, dim3((unsigned)n), dim3(256), 0, s, dpar, darea, dsum, HW, dcent + 2 * (size_t)f0, dar + f0);
        HIPC(h, hipGetLastError());
    }
    HIPC(h, hipMemcpyAsync(cent_out, dcent, (size_t)N * 16, hipMemcpyDeviceToHost, s));
    HIPC(h, hipMemcpyAsync(area_out, dar, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    return label_errors(h, derr, "tf_av_centroids");
}

// tf_first_region_areas: frames go through in chunks so that the per-chunk scratch (6 B per pixel, the parents and tile-local roots of
// the PRE_LB_* slots every labelling call uses, + the mask bytes) stays within MASK_CHUNK_BYTES (tests: the area_chunk_kib knob) whatever
// the study's length
int first_region_areas(tf_handle* h, const Src& masks, int N, int H, int W, int C, long long* area_out)
{
    using namespace fra;
    const size_t HW = (size_t)H * W;
    if (HW > 0x7fffffffu) return fail(h, TF_ERR_UNSUPPORTED, "tf_first_region_areas: at most 2^31 - 1 pixels per frame");
    const size_t budget = h->area_chunk_kib > 0 ? (size_t)h->area_chunk_kib << 10 : MASK_CHUNK_BYTES;
    const int nf = chunk_frames(HW * (6 + (size_t)C), N, 65535, budget);   // frames of a chunk are grid.y
    HIPC(h, hipSetDevice(h->dev));
    Pre pre(h);
    auto* um = masks.dev ? nullptr : pre.get<uint8_t>(tf_handle::PRE_CT_MASK, (size_t)nf * HW * C);
    auto* dpar = pre.get<uint32_t>(tf_handle::PRE_LB_PAR, (size_t)nf * HW);
    auto* dlr = pre.get<uint16_t>(tf_handle::PRE_LB_LR, (size_t)nf * HW);
    // [0, 64): error word, then areas [N] u64, then the chunk's seeds [nf] u32 and seed values [nf] u8
    auto* out = pre.get<uint8_t>(tf_handle::PRE_CT_OUT, 64 + (size_t)N * 8 + (size_t)nf * 5);
    if (pre.rc) return pre.rc;
    unsigned* derr = (unsigned*)out;
    unsigned long long* dar = (unsigned long long*)(out + 64);
    uint32_t* dseed = (uint32_t*)(out + 64 + (size_t)N * 8);
    uint8_t* dval = (uint8_t*)(dseed + nf);
    const hipStream_t s = h->stream;
    HIPC(h, hipMemsetAsync(derr, 0, sizeof(unsigned), s));
    for (int f0 = 0; f0 < N; f0 += nf) {
        const int n = std::min(nf, N - f0);
        const uint8_t* dm = nullptr;
        int rc = src_to_device(h, masks, (size_t)f0 * HW * C, (size_t)n * HW * C, um, &dm);
        if (rc) return rc;
        hipLaunchKernelGGL(k_area_seed, dim3((unsigned)n), dim3(256), 0, s, dm, C, HW, dseed, dval, dar + f0);
        rc = label_planes<8, true>(h, SeedValueSet{dm, dseed, dval, C, HW}, SeedArea{dseed, dar + f0}, (size_t)n, H, W, dpar, dlr, derr);
        if (rc) return rc;
        HIPC(h, hipGetLastError());
    }
    HIPC(h, hipMemcpyAsync(area_out, dar, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    return label_errors(h, derr, "tf_first_region_areas");
}

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

// Argument checks return before the handle is touched (no message: the Python layer checks the same first and says why).
TF_API int tf_av_centroids(tf_handle* h, const uint8_t* masks, int N, int H, int W, int C, double* centroids_out, long long* area_out)
{
    if (!h || !masks || !centroids_out || !area_out || N < 1 || H < 1 || W < 1 || (C != 1 && C != 2)) return TF_ERR_INVALID_ARG;
    return finish_host_call(h, av_centroids(h, Src::on_host(masks), N, H, W, C, centroids_out, area_out));
}

TF_API int tf_first_region_areas(tf_handle* h, const uint8_t* masks, int N, int H, int W, int C, long long* area_out)
{
    if (!h || !masks || !area_out || N < 1 || H < 1 || W < 1 || (C != 1 && C != 2)) return TF_ERR_INVALID_ARG;
    return finish_host_call(h, first_region_areas(h, Src::on_host(masks), N, H, W, C, area_out));
}

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

static_assert(TF_ECHO_F16 == ovl::ECHO_F16 && TF_ECHO_U8 == ovl::ECHO_U8, "echo kinds of the header and the kernel differ");

namespace {
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

TF_API int tf_radlong_shape(tf_handle* h, int* shape)
{
    if (!h || !shape) return TF_ERR_INVALID_ARG;
    const bool have = h->anN >= 1 && !h->an_polar;
    shape[0] = have ? h->anN : 0; shape[1] = have ? h->anH : 0; shape[2] = have ? h->anW : 0;
    return TF_OK;
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

// pinned host memory for results: a destination allocated here makes the host-pointer entry points copy out at PCIe
// speed, overlapped with the solve of the next sub-batch
TF_API void* tf_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
TF_API void tf_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

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

// ---- a study call: the frames of a study in, its `flow` array (and `echo`) out ---------------------------------------------------
namespace {
enum StudyFrames { FR_GRAY, FR_SAL_U8, FR_SAL_F32 };     // what the solver sees: the conditioned gray frames, or the saliency maps
// what every study entry point fills
struct Study {
    const uint8_t* frames; int N, H, W, channels;        // host, uint8 [N][H][W][channels]
    StudyFrames sees;
    float scale; bool out_f16;
    void* flow_out; uint16_t* echo16_out;                // host: [N-1][H][W][2] of the output type; [N][H][W] halves or null
    bool wase = false;                                   // (flow - background) * scale, from the bkgd mask [n_frames][H][W][2]
    const uint8_t* bkgd = nullptr; int n_frames = 0; float* background_out = nullptr;   // (host, [N-1] or null)
    bool held_only = false;                              // tf_calc_seq_rgb_held: the payload is left held and nothing is copied to the host
    bool held_echo = false;                              // (flow_out and echo16_out are null); held_echo: with the study's echo
};

// the solver's frames of study s on the device (`own`: a submitted job's buffer for them, see condition_to_device)
// (echo_keep: device memory that gets the study's echo too, or null)
// (fr: where the frames are, the study's host pointer or the held frames)
int study_frames_to_device(tf_handle* h, const Study& s, const Src& fr, uint8_t* own, const uint8_t** dfr, uint16_t* echo_keep)
{
    return s.sees == FR_GRAY ? condition_to_device(h, fr, s.N, s.H, s.W, dfr, own, s.echo16_out, echo_keep)
                             : saliency_to_device(h, fr, s.N, s.H, s.W, s.channels, s.sees == FR_SAL_F32, dfr, s.echo16_out, echo_keep);
}

// Buffers of the handle's own for a study of N flow frames, and n_echo echo frames, of H x W; whatever was held before goes.  The
// caller fills them.  A failure leaves no study held.
int held_alloc(tf_handle* h, int N, int H, int W, int n_echo)
{
    HIPC(h, hipSetDevice(h->dev));
    HIPC(h, hipStreamSynchronize(h->stream));                 // (the tail calls are host-synchronous: nothing reads the old buffers)
    tf_handle::Held& k = h->held;
    k.release();
    const size_t HW = (size_t)H * W;
    hipError_t e = hipMalloc(&k.flow, (size_t)N * HW * 2 * sizeof(uint16_t));
    if (e == hipSuccess && n_echo) e = hipMalloc(&k.echo, (size_t)n_echo * HW * sizeof(uint16_t));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        k.release();
        return fail(h, e == hipErrorOutOfMemory ? TF_ERR_NOMEM : TF_ERR_HIP, "holding a study of %d x %d x %d: hipMalloc failed: %s", N, H, W, hipGetErrorString(e));
    }
    k.N = N; k.H = H; k.W = W; k.n_echo = n_echo;
    ++k.gen;
    return TF_OK;
}

// the held flow's last frame: flow N - 2 repeated, as the study file holds it (queued on the handle's stream)
int held_repeat_last(tf_handle* h)
{
    const tf_handle::Held& k = h->held;
    const size_t hw2 = (size_t)k.H * k.W * 2;
    HIPC(h, hipMemcpyAsync(k.flow + (size_t)(k.N - 1) * hw2, k.flow + (size_t)(k.N - 2) * hw2, hw2 * sizeof(uint16_t), hipMemcpyDeviceToDevice, h->stream));
    return TF_OK;
}

// The tail of a WASE study.  The flows never leave the device between the solve and the compensation: the solver has written them,
// unscaled float32, into dflow (PRE_WS_FLOW); the reduction reads them there, and k_wase_out writes the compensated, scaled flows in
// the call's output type into PRE_WS_OUT, which is copied to the caller's buffer (and, `hold`, on the device into the held flow).
int wase_study_tail(tf_handle* h, const Study& s, const float* dflow, bool hold)
{
    const int P = s.N - 1, H = s.H, W = s.W;
    const size_t hw2 = (size_t)H * W * 2, elt = s.out_f16 ? sizeof(uint16_t) : sizeof(float);
    Pre pre(h);
    auto* dout = pre.get<uint8_t>(tf_handle::PRE_WS_OUT, (size_t)P * hw2 * elt);
    auto* dmask = pre.get<uint8_t>(tf_handle::PRE_AN_MASK, (size_t)s.n_frames * hw2);
    if (pre.rc) return pre.rc;
    const hipStream_t stream = h->stream;
    HIPC(h, hipMemcpyAsync(dmask, s.bkgd, (size_t)s.n_frames * hw2, hipMemcpyHostToDevice, stream));
    HIPC(h, hipEventRecord(h->ev[0], stream));                // the reduction and the output kernel, without the copies
    float* wbg = nullptr;
    const int rc = wase_backgrounds(h, dflow, dmask, P, s.n_frames, H, W, &wbg);
    if (rc) return rc;
    const Geom g = make_geom(W, H);
    if (s.out_f16) hipLaunchKernelGGL(k_wase_out<uint16_t>, out_grid<uint16_t>(g, P), dim3(256), 0, stream, dflow, wbg, H, W, s.scale, (uint16_t*)dout);
    else hipLaunchKernelGGL(k_wase_out<float>, out_grid<float>(g, P), dim3(256), 0, stream, dflow, wbg, H, W, s.scale, (float*)dout);
    HIPC(h, hipGetLastError());
    HIPC(h, hipEventRecord(h->ev[1], stream));
    HIPC(h, hipMemcpyAsync(s.flow_out, dout, (size_t)P * hw2 * elt, hipMemcpyDeviceToHost, stream));
    if (hold) {                                               // (a held study is float16: study_call has refused the others)
        HIPC(h, hipMemcpyAsync(h->held.flow, dout, (size_t)P * hw2 * elt, hipMemcpyDeviceToDevice, stream));
        if (int rc2 = held_repeat_last(h)) return rc2;
    }
    if (s.background_out) HIPC(h, hipMemcpyAsync(s.background_out, wbg, (size_t)P * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIPC(h, hipStreamSynchronize(stream));
    float t = 0;
    HIPC(h, hipEventElapsedTime(&t, h->ev[0], h->ev[1]));
    h->wase_kernel_ms = t;
    return TF_OK;
}

// Every study entry point: the study's own argument checks, check_call (on the host frames, before anything is uploaded), the ticket,
// the WASE kernels' grid limits -- the order every route had, so each refusal is the one it was (the saliency pass checks its own
// limits) -- then the frames to the device and the solve.  `submit` (a plain RGB study only): the frames are conditioned now, on the
// handle's stream, into a buffer the job owns; the solve is queued and *ticket is what tf_wait takes.
// Armed by tf_frames_next, the call reads the held frames in place of its host pointer (take_frames); a submitted study conditions
// them into its own buffer before it returns, so they may be replaced at once.
// Armed by tf_hold_next, a synchronous float16 call also leaves its payload held (teeflow_held.hip.h): N flow frames, the last one
// repeated, and the echo if the call makes one, copied on the device from what the call wrote there.  The flag is spent by the call,
// refused or not; the old held study goes once the call's arguments have passed, and a call that fails after that holds nothing.
// A held-only study (Study::held_only) is such a call without the host copies: the lanes' copy-out is skipped (Call::keep_only) and
// k_echo_f16 writes into the held echo itself.
int study_call(tf_handle* h, const Study& s, tf_stats* st, int* ticket = nullptr, bool submit = false)
{
    struct Owned { uint8_t* p = nullptr; ~Owned() { if (p) (void)hipFree(p); } } own;     // (freed after the failed call has been drained)
    const bool hold = h && (h->hold_next || s.held_only);
    if (h) h->hold_next = false;
    const bool chain = h && h->chain_next;                   // tf_chain_next: spent likewise
    if (h) h->chain_next = false;
    bool holding = false;                                    // held_alloc has run for this call
    Src fr;                                                  // tf_frames_next: spent likewise
    const int frames_rc = h ? take_frames(h, "a study call", spend_frames_next(h), s.frames, s.N, s.H, s.W, s.channels, &fr) : TF_OK;
    auto run = [&]() -> int {
        if (!h) return TF_ERR_INVALID_ARG;
        if (frames_rc) return frames_rc;
        if (hold && submit) return fail(h, TF_ERR_UNSUPPORTED, "a submitted study cannot be held: tf_hold_next arms a synchronous float16 study call");
        if (hold && !s.out_f16) return fail(h, TF_ERR_UNSUPPORTED, "only a float16 study call can leave its payload held");
        if (s.sees != FR_GRAY && s.channels != 1 && s.channels != 3) return fail(h, TF_ERR_INVALID_ARG, "saliency: frames must have 1 or 3 channels, got %d", s.channels);
        if (s.echo16_out && s.channels != 3) return fail(h, TF_ERR_INVALID_ARG, "the echo needs RGB frames (channels == 3), got %d", s.channels);
        if (s.wase && (!s.bkgd || s.n_frames < 1)) return fail(h, TF_ERR_INVALID_ARG, "a wase study needs a bkgd mask of at least 1 frame, got %d", s.n_frames);
        if (submit && (s.sees != FR_GRAY || s.wase)) return fail(h, TF_ERR_UNSUPPORTED, "only a plain RGB study can be submitted");
        // float maps reach the solver as CV_32F frames (DualTVL1: x 255; DeepFlow: as they are); a WASE study's scale is k_wase_out's
        Call c{MODE_SEQ, (const uint8_t*)(fr.dev ? fr.dev : fr.host), nullptr, s.N - 1, s.H, s.W, s.wase ? 1.0f : s.scale, s.flow_out, W_HOST, s.sees == FR_SAL_F32, s.out_f16};
        c.chain = chain;
        c.keep_only = s.held_only;
        int rc = check_call(h, c);
        if (rc) return rc;
        if (submit && !ticket) return TF_ERR_INVALID_ARG;
        if (s.wase && (s.N > 65535 || s.n_frames > 65535)) return fail(h, TF_ERR_UNSUPPORTED, "a wase study takes at most 65535 frames and mask frames");   // (grid dimensions)
        if (submit) {
            HIPC(h, hipSetDevice(h->dev));
            HIPC(h, hipMalloc(&own.p, (size_t)s.N * s.H * s.W));
        }
        if (hold) {
            if ((rc = held_alloc(h, s.N, s.H, s.W, s.echo16_out || s.held_echo ? s.N : 0))) return rc;
            holding = true;
        }
        rc = study_frames_to_device(h, s, fr, own.p, &c.in0, hold ? h->held.echo : nullptr);
        if (rc) return rc;
        c.where = W_IN_DEV;
        // frames on the device, flows to the caller's host buffer: sub-batch by sub-batch through the pinned, overlapped copy-out path
        if (submit) { uint8_t* p = own.p; own.p = nullptr; return submit_entry(h, c, ticket, p); }   // (the job's from here on)
        if (!s.wase) {
            if (hold) c.keep = h->held.flow;                  // each sub-batch's flows, copied on the device by the engine that solved them
            rc = calc_entry(h, c, st);
            if (!rc && !s.held_only)                          // what the call has copied to the caller's arrays
                h->study_download_bytes += (long long)(c.n_pairs * c.flow_bytes() + (s.echo16_out ? (size_t)s.N * s.H * s.W * sizeof(uint16_t) : 0));
            if (rc || !hold) return rc;
            if ((rc = held_repeat_last(h))) return rc;
            HIPC(h, hipStreamSynchronize(h->stream));
            return TF_OK;
        }
        Pre pre(h);
        auto* dflow = pre.get<float>(tf_handle::PRE_WS_FLOW, (size_t)c.n_pairs * s.H * s.W * 2);
        if (pre.rc) return pre.rc;
        c.out = dflow; c.where = W_DEV; c.out_f16 = false;
        rc = calc_entry(h, c, st);                            // (returns with every lane's stream drained: the flows are there)
        if (!rc) rc = wase_study_tail(h, s, dflow, hold);
        if (!rc) h->study_download_bytes += (long long)((size_t)c.n_pairs * s.H * s.W * 2 * (s.out_f16 ? sizeof(uint16_t) : sizeof(float))
                                                        + (s.echo16_out ? (size_t)s.N * s.H * s.W * sizeof(uint16_t) : 0));
        return rc;
    };
    const int rc = finish_host_call(h, run());
    if (rc && holding) h->held.release();
    return rc;
}
}  // namespace

TF_API int tf_calc_seq_rgb(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, float* flow_out, tf_stats* st)
{
    return study_call(h, {rgb, N, H, W, 3, FR_GRAY, scale, false, flow_out, nullptr}, st);
}
TF_API int tf_submit_seq_rgb(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, float* flow_out, int* ticket)
{
    return study_call(h, {rgb, N, H, W, 3, FR_GRAY, scale, false, flow_out, nullptr}, nullptr, ticket, true);
}
TF_API int tf_calc_seq_rgb_f16(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, uint16_t* flow16_out, uint16_t* echo16_out,
                               tf_stats* st)
{
    return study_call(h, {rgb, N, H, W, 3, FR_GRAY, scale, true, flow16_out, echo16_out}, st);
}
TF_API int tf_submit_seq_rgb_f16(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, uint16_t* flow16_out, uint16_t* echo16_out,
                                 int* ticket)
{
    return study_call(h, {rgb, N, H, W, 3, FR_GRAY, scale, true, flow16_out, echo16_out}, nullptr, ticket, true);
}
// tf_calc_seq_rgb_f16 after tf_hold_next without its host arrays: the study is solved into the held payload and nothing is downloaded
TF_API int tf_calc_seq_rgb_held(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, int with_echo, tf_stats* st)
{
    Study s{rgb, N, H, W, 3, FR_GRAY, scale, true, nullptr, nullptr};
    s.held_only = true; s.held_echo = with_echo != 0;
    return study_call(h, s, st);
}
// Several RGB studies of one frame size as chains in lock-step (teeflow.hip, check_chains): each study is conditioned as tf_calc_seq_rgb
// conditions it, one after the other into one scratch slot that holds all their gray frames; its echo, where asked for, comes from the same
// upload.  The flags are spent first, the arguments checked on the host pointers before anything is uploaded.
TF_API int tf_calc_chains_rgb(tf_handle* h, const uint8_t* const* rgb, const int* n_frames, int n_chains, int H, int W, float scale, int out_f16,
                              void* const* flows_out, uint16_t* const* echo16_out, tf_stats* st)
{
    const int armed = spend_flags(h);
    auto run = [&]() -> int {
        ChainSet cs; Call c;
        int rc = check_chains(h, (const void* const*)rgb, n_frames, n_chains, H, W, scale, flows_out, W_HOST, out_f16 != 0, armed, &cs, &c);
        if (rc) return rc;
        HIPC(h, hipSetDevice(h->dev));                        // (the scratch below is this handle's device's, whatever the thread's current one)
        const size_t npx = (size_t)H * W;
        Pre pre(h);
        uint8_t* at = pre.get<uint8_t>(tf_handle::PRE_CH_GRAY, ((size_t)c.n_pairs + (size_t)n_chains) * npx);
        if (pre.rc) return pre.rc;
        for (int s = 0; s < cs.count(); ++s) {
            const int N = cs.pairs[s] + 1;
            const uint8_t* dgray = nullptr;
            rc = condition_to_device(h, Src::on_host(cs.in[s]), N, H, W, &dgray, at, echo16_out ? echo16_out[cs.order[s]] : nullptr);
            if (rc) return rc;
            cs.in[s] = dgray; at += (size_t)N * npx;
        }
        c.in0 = cs.in[0]; c.where = W_IN_DEV;
        return run_chains(h, c, st);
    };
    return finish_host_call(h, run());
}
TF_API int tf_calc_seq_saliency(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, float scale, float* flow_out, tf_stats* st)
{
    return study_call(h, {frames, N, H, W, channels, FR_SAL_U8, scale, false, flow_out, nullptr}, st);
}
TF_API int tf_calc_seq_saliency_f32(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, float scale, float* flow_out, tf_stats* st)
{
    return study_call(h, {frames, N, H, W, channels, FR_SAL_F32, scale, false, flow_out, nullptr}, st);
}
TF_API int tf_calc_seq_saliency_f16(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, int map_f32, float scale,
                                    uint16_t* flow16_out, uint16_t* echo16_out, tf_stats* st)
{
    return study_call(h, {frames, N, H, W, channels, map_f32 ? FR_SAL_F32 : FR_SAL_U8, scale, true, flow16_out, echo16_out}, st);
}
TF_API int tf_calc_seq_rgb_wase(tf_handle* h, const uint8_t* rgb, int N, int H, int W, const uint8_t* bkgd, int n_frames, float scale, int out_f16,
                                void* flow_out, uint16_t* echo16_out, float* background_out, tf_stats* st)
{
    return study_call(h, {rgb, N, H, W, 3, FR_GRAY, scale, out_f16 != 0, flow_out, echo16_out, true, bkgd, n_frames, background_out}, st);
}
TF_API int tf_calc_seq_saliency_wase(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, int map_f32, const uint8_t* bkgd,
                                     int n_frames, float scale, int out_f16, void* flow_out, uint16_t* echo16_out, float* background_out, tf_stats* st)
{
    return study_call(h, {frames, N, H, W, channels, map_f32 ? FR_SAL_F32 : FR_SAL_U8, scale, out_f16 != 0, flow_out, echo16_out, true, bkgd,
                          n_frames, background_out}, st);
}
