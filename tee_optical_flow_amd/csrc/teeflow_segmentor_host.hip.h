// The SAM segmentor's frame glue, on the caller's stream: tf_segmentor_input (PIL's bilinear resize and the LUT, into the model's input tensor) and tf_segmentor_classmap.
// Relies on teeflow_scratch.hip.h, on call_frames of teeflow_frames_host.hip.h, on pil_resample_tables.h and on the kernels of teeflow_segmentor.hip.h.

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
    Src fr;
    const int args_rc = !lut || !d_out || N < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1 ? TF_ERR_INVALID_ARG
                        : (size_t)H * W > 0x7fffffffu || (size_t)out_h * out_w > 0x7fffffffu ? TF_ERR_UNSUPPORTED : TF_OK;
    if (int rc = call_frames(h, "tf_segmentor_input", rgb, N, H, W, 3, args_rc, &fr)) return rc;
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
