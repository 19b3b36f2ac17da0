// The calls that label connected components (teeflow_ccl.hip.h) on the PRE_LB_* slots: tf_clean_masks, tf_otsu_masks, tf_av_centroids, tf_first_region_areas.
// Relies on teeflow_scratch.hip.h, on call_frames of teeflow_frames_host.hip.h (Otsu takes frames) and on the kernels of teeflow_masks / _otsu / _centroid / _area.hip.h.

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
    if (int rc = src_to_device(h, rgb, 0, (size_t)N * HW * 3, urgb, &drgb, &tf_handle::frames_upload_bytes)) return rc;
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
}  // namespace

TF_API int tf_otsu_masks(tf_handle* h, const uint8_t* rgb, int N, int H, int W, long long min_size, uint8_t* masks_out, double* thresholds_out)
{
    Src fr;
    const int args_rc = !masks_out || N < 2 || H < 2 || W < 2 ? TF_ERR_INVALID_ARG
                        : (size_t)H * W > 0x7fffffffu || N > 65535 ? TF_ERR_UNSUPPORTED : TF_OK;   // (frames are a grid dimension)
    if (int rc = call_frames(h, "tf_otsu_masks", rgb, N, H, W, 3, args_rc, &fr)) return rc;
    return finish_host_call(h, otsu_masks(h, fr, N, H, W, min_size, masks_out, thresholds_out));
}

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
