// A study held on the device: the study file's payload -- float16 flow, optional float16 echo, up to TF_HELD_SLOTS masks -- in buffers of
// the handle's own (tf_handle::Held), put there once from host arrays (tf_hold_study, tf_hold_mask) or by the solve that made it
// (tf_hold_next; study_call in teeflow_study_host.hip.h, which is included after this), and the tail calls that read it there: every
// tf_held_* call is its original's internal function with device sources (Src) in the place of host ones, so there is one copy of every
// kernel and launch rule.  Nothing else writes the held buffers: the PRE_* scratch and the resident analysis planes stay what they
// were.  Relies on teeflow_masks_host / _analysis_host / _overlay_host.hip.h.

namespace {
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

// the held study, for a call named `who` that reads it: TF_ERR_INVALID_ARG and why when there is none
int held_study(tf_handle* h, const char* who)
{
    if (h->held.N < 1) return fail(h, TF_ERR_INVALID_ARG, "%s: no study is held (tf_hold_study, or tf_hold_next before a float16 study call)", who);
    return TF_OK;
}

// ... and its mask slot, of which the call reads n frames
int held_mask(tf_handle* h, const char* who, int slot, int n, const tf_handle::Held::Mask** out)
{
    if (int rc = held_study(h, who)) return rc;
    if (slot < 0 || slot >= TF_HELD_SLOTS) return fail(h, TF_ERR_INVALID_ARG, "%s: mask slot %d is out of range [0, %d)", who, slot, TF_HELD_SLOTS);
    const tf_handle::Held::Mask& m = h->held.mask[slot];
    if (!m.p) return fail(h, TF_ERR_INVALID_ARG, "%s: mask slot %d is empty", who, slot);
    if (n < 1) return fail(h, TF_ERR_INVALID_ARG, "%s: %d frames asked for, need at least 1", who, n);
    if (n > m.n_frames) return fail(h, TF_ERR_INVALID_ARG, "%s: the mask in slot %d has %d frames, fewer than the %d asked for", who, slot, m.n_frames, n);
    *out = &m;
    return TF_OK;
}

// what the two held projections check alike (check_project_param's rules, on the held study's sizes, with their cause)
int held_project_check(tf_handle* h, const char* who, int n_used, int slot, int param, double spacing, const tf_handle::Held::Mask** m)
{
    if (int rc = held_study(h, who)) return rc;
    const int N = h->held.N;
    if (n_used < 1 || n_used > N) return fail(h, TF_ERR_INVALID_ARG, "%s: n_used %d is outside [1, %d], the held study's frames", who, n_used, N);
    if (int rc = held_mask(h, who, slot, n_used, m)) return rc;
    if (param < TF_PARAM_VELOCITY || param > TF_PARAM_PWR) return fail(h, TF_ERR_INVALID_ARG, "%s: param %d is none of velocity (0), acceleration (1), PWR (2)", who, param);
    if (param != TF_PARAM_VELOCITY && N < 2) return fail(h, TF_ERR_INVALID_ARG, "%s: acceleration and PWR need at least 2 held frames, the study has %d", who, N);
    if (param != TF_PARAM_VELOCITY && (!std::isfinite(spacing) || spacing == 0.0))
        return fail(h, TF_ERR_INVALID_ARG, "%s: acceleration and PWR need a finite, non-zero spacing, got %g", who, spacing);
    if (n_used > 65535) return fail(h, TF_ERR_UNSUPPORTED, "%s: at most 65535 frames", who);              // frames are grid.y
    return TF_OK;
}

// bytes host -> a fresh device buffer, on the handle's stream, waited for; counted as a tail upload
int held_upload(tf_handle* h, const void* src, size_t bytes, void** out)
{
    void* p = nullptr;
    HIPC(h, hipMalloc(&p, bytes));
    const hipError_t e = hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, h->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(h->stream) : e;
    if (e2 != hipSuccess) {
        (void)hipGetLastError(); (void)hipFree(p);
        return fail(h, TF_ERR_HIP, "uploading %zu held bytes failed: %s", bytes, hipGetErrorString(e2));
    }
    h->tail_upload_bytes += (long long)bytes;
    *out = p;
    return TF_OK;
}
}  // namespace

TF_API int tf_hold_study(tf_handle* h, const uint16_t* flow16, int N, int H, int W, const uint16_t* echo16, int n_echo)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!flow16 || N < 1 || H < 1 || W < 1) return fail(h, TF_ERR_INVALID_ARG, "tf_hold_study: null flow or bad sizes: N=%d H=%d W=%d", N, H, W);
    if (echo16 ? n_echo < 1 : n_echo != 0) return fail(h, TF_ERR_INVALID_ARG, "tf_hold_study: %d echo frames with %s echo", n_echo, echo16 ? "an" : "no");
    auto run = [&]() -> int {
        int rc = held_alloc(h, N, H, W, n_echo);
        if (rc) return rc;
        const size_t HW = (size_t)H * W, fb = (size_t)N * HW * 2 * sizeof(uint16_t), eb = (size_t)n_echo * HW * sizeof(uint16_t);
        HIPC(h, hipMemcpyAsync(h->held.flow, flow16, fb, hipMemcpyHostToDevice, h->stream));
        if (n_echo) HIPC(h, hipMemcpyAsync(h->held.echo, echo16, eb, hipMemcpyHostToDevice, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        h->tail_upload_bytes += (long long)(fb + eb);
        return TF_OK;
    };
    const int rc = finish_host_call(h, run());
    if (rc) h->held.release();
    return rc;
}

TF_API int tf_hold_mask(tf_handle* h, int slot, const uint8_t* mask, int n_frames, int C)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (int rc = held_study(h, "tf_hold_mask")) return rc;
    if (slot < 0 || slot >= TF_HELD_SLOTS) return fail(h, TF_ERR_INVALID_ARG, "tf_hold_mask: mask slot %d is out of range [0, %d)", slot, TF_HELD_SLOTS);
    if (!mask || n_frames < 1 || (C != 1 && C != 2)) return fail(h, TF_ERR_INVALID_ARG, "tf_hold_mask: null mask, or bad sizes: n_frames=%d C=%d", n_frames, C);
    auto run = [&]() -> int {
        HIPC(h, hipSetDevice(h->dev));
        void* p = nullptr;
        const int rc = held_upload(h, mask, (size_t)n_frames * h->held.H * h->held.W * C, &p);
        if (rc) return rc;
        tf_handle::Held::Mask& m = h->held.mask[slot];
        (void)hipFree(m.p);                                   // (the tail calls are host-synchronous: nothing reads the old mask)
        m.p = (uint8_t*)p; m.n_frames = n_frames; m.C = C;
        return TF_OK;
    };
    return finish_host_call(h, run());
}

TF_API int tf_hold_next(tf_handle* h, int on)
{
    if (!h) return TF_ERR_INVALID_ARG;
    h->armed.hold = on != 0;
    return TF_OK;
}

TF_API int tf_held_shape(tf_handle* h, long long* out)
{
    if (!h || !out) return TF_ERR_INVALID_ARG;
    const tf_handle::Held& k = h->held;
    out[0] = k.N; out[1] = k.H; out[2] = k.W; out[3] = k.n_echo; out[4] = k.gen;
    for (int s = 0; s < TF_HELD_SLOTS; ++s) { out[5 + 2 * s] = k.mask[s].n_frames; out[6 + 2 * s] = k.mask[s].C; }
    return TF_OK;
}

TF_API int tf_release_study(tf_handle* h)
{
    if (!h) return TF_ERR_INVALID_ARG;
    HIPC(h, hipSetDevice(h->dev));
    HIPC(h, hipStreamSynchronize(h->stream));
    h->held.release();
    return TF_OK;
}

TF_API int tf_held_av_centroids(tf_handle* h, int slot, int N, double* centroids_out, long long* area_out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!centroids_out || !area_out) return fail(h, TF_ERR_INVALID_ARG, "tf_held_av_centroids: null output pointer");
    const tf_handle::Held::Mask* m = nullptr;
    if (int rc = held_mask(h, "tf_held_av_centroids", slot, N, &m)) return rc;
    return finish_host_call(h, av_centroids(h, Src::on_device(m->p), N, h->held.H, h->held.W, m->C, centroids_out, area_out));
}

TF_API int tf_held_first_region_areas(tf_handle* h, int slot, int N, long long* area_out)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!area_out) return fail(h, TF_ERR_INVALID_ARG, "tf_held_first_region_areas: null output pointer");
    const tf_handle::Held::Mask* m = nullptr;
    if (int rc = held_mask(h, "tf_held_first_region_areas", slot, N, &m)) return rc;
    return finish_host_call(h, first_region_areas(h, Src::on_device(m->p), N, h->held.H, h->held.W, m->C, area_out));
}

TF_API int tf_held_radlong_project_param(tf_handle* h, int n_used, int slot, int param, double spacing, int grad_f64, const double* centroids,
                                         double* rad_out, double* long_out, double* minmax, long long* nonzero)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!centroids || !minmax || !nonzero) return fail(h, TF_ERR_INVALID_ARG, "tf_held_radlong_project_param: null centroids, minmax or nonzero");
    const tf_handle::Held::Mask* m = nullptr;
    if (int rc = held_project_check(h, "tf_held_radlong_project_param", n_used, slot, param, spacing, &m)) return rc;
    const tf_handle::Held& k = h->held;
    return finish_host_call(h, radlong_project_param(h, Src::on_device(k.flow), 1, k.N, n_used, k.H, k.W, Src::on_device(m->p), m->C, param, spacing,
                                                     grad_f64 ? 1 : 0, centroids, rad_out, long_out, minmax, nonzero));
}

TF_API int tf_held_polar_project_param(tf_handle* h, int n_used, int slot, int param, double spacing, int grad_f64, float* mag_out, float* ang_out,
                                       float* minmax, long long* nonzero, float* ang_mode)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!minmax || !nonzero || !ang_mode) return fail(h, TF_ERR_INVALID_ARG, "tf_held_polar_project_param: null minmax, nonzero or ang_mode");
    const tf_handle::Held::Mask* m = nullptr;
    if (int rc = held_project_check(h, "tf_held_polar_project_param", n_used, slot, param, spacing, &m)) return rc;
    const tf_handle::Held& k = h->held;
    if ((size_t)k.H * k.W > 0xFFFFFFFFu) return fail(h, TF_ERR_UNSUPPORTED, "tf_held_polar_project_param: a frame's counts are 32-bit");
    return finish_host_call(h, polar_project_param(h, Src::on_device(k.flow), 1, k.N, n_used, k.H, k.W, Src::on_device(m->p), m->C, param, spacing,
                                                   grad_f64 ? 1 : 0, mag_out, ang_out, minmax, nonzero, ang_mode));
}

TF_API int tf_held_radlong_overlay(tf_handle* h, const double* lut_rad, const double* lut_long, uint8_t* out, double* info)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (!lut_rad || !lut_long || !out || !info) return fail(h, TF_ERR_INVALID_ARG, "tf_held_radlong_overlay: null table or output pointer");
    if (int rc = held_study(h, "tf_held_radlong_overlay")) return rc;
    const tf_handle::Held& k = h->held;
    if (!k.echo) return fail(h, TF_ERR_INVALID_ARG, "tf_held_radlong_overlay: the held study has no echo");
    if (int rc = check_overlay(h, lut_rad, lut_long)) return rc;
    if (h->anH != k.H || h->anW != k.W)
        return fail(h, TF_ERR_INVALID_ARG, "tf_held_radlong_overlay: the planes are %d x %d, the held echo %d x %d", h->anH, h->anW, k.H, k.W);
    if (k.n_echo < h->anN) return fail(h, TF_ERR_INVALID_ARG, "tf_held_radlong_overlay: the held echo has %d frames, fewer than the planes' %d", k.n_echo, h->anN);
    return finish_host_call(h, radlong_overlay<ovl::ECHO_F16>(h, Src::on_device(k.echo), lut_rad, lut_long, out, info));
}

// (the field and the norm's range are over all N held frames, so the mask in `slot` must cover them all; n_used frames are rendered)
TF_API int tf_held_magnitude_overlay(tf_handle* h, int n_used, int slot, int param, double spacing, int grad_f64, int norm_f64, const double* lut,
                                     uint8_t* out, double* info, double* frame_info)
{
    const char* who = "tf_held_magnitude_overlay";
    if (!h) return TF_ERR_INVALID_ARG;
    if (!lut || !out || !info || !frame_info) return fail(h, TF_ERR_INVALID_ARG, "%s: null table or output pointer", who);
    const tf_handle::Held::Mask* m = nullptr;
    if (int rc = held_project_check(h, who, n_used, slot, param, spacing, &m)) return rc;
    const tf_handle::Held& k = h->held;
    if (m->n_frames < k.N)
        return fail(h, TF_ERR_INVALID_ARG, "%s: the mask in slot %d has %d frames, fewer than the study's %d (the norm's range is over all of them)", who, slot, m->n_frames, k.N);
    if (!k.echo) return fail(h, TF_ERR_INVALID_ARG, "%s: the held study has no echo", who);
    if (k.n_echo < n_used) return fail(h, TF_ERR_INVALID_ARG, "%s: the held echo has %d frames, fewer than the %d asked for", who, k.n_echo, n_used);
    if (int rc = check_magnitude_overlay(h, who, k.N, k.H, k.W, lut)) return rc;
    return finish_host_call(h, magnitude_overlay<ovl::ECHO_F16>(h, Src::on_device(k.flow), 1, k.N, n_used, k.H, k.W, Src::on_device(m->p), m->C, param, spacing,
                                                                grad_f64 ? 1 : 0, norm_f64 ? 1 : 0, Src::on_device(k.echo), lut, out, info, frame_info));
}
