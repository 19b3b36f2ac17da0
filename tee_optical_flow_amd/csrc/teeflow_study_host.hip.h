// The study calls, a study's frames in, its `flow` array (and `echo`) out: Study, study_call and the tf_calc_seq_rgb* / tf_calc_seq_saliency* / *_wase / tf_submit_seq_rgb*
// entry points.  Relies on teeflow_queue.hip.h (calc_entry, submit_entry), teeflow_frames_host.hip.h, teeflow_wase_host.hip.h and teeflow_held.hip.h (held_alloc, held_repeat_last).

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
int study_frames_on_device(tf_handle* h, const Study& s, const Src& fr, uint8_t* own, const uint8_t** dfr, uint16_t* echo_keep)
{
    return s.sees == FR_GRAY ? condition_to_device(h, fr, s.N, s.H, s.W, dfr, own, s.echo16_out, echo_keep)
                             : saliency_to_device(h, fr, s.N, s.H, s.W, s.channels, s.sees == FR_SAL_F32, dfr, s.echo16_out, echo_keep);
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
    HIPC(h, dev_time(h, 0, 1, tf_handle::DT_WASE, false));
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
    const tf_handle::Armed armed = spend(h, SPEND_ALL);       // all three flags, refused or not (nothing on a null handle)
    const bool hold = h && (armed.hold || s.held_only);
    bool holding = false;                                    // held_alloc has run for this call
    Src fr;
    const int frames_rc = h ? take_frames(h, "a study call", armed, s.frames, s.N, s.H, s.W, s.channels, &fr) : TF_OK;
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
        c.chain = armed.chain;
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
        rc = study_frames_on_device(h, s, fr, own.p, &c.in0, hold ? h->held.echo : nullptr);
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
