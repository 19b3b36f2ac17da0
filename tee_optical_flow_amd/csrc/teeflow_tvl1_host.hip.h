// teeflow_tvl1_host.hip.h -- DualTVL1's host side: parameters, pyramid geometry, Tvl1State's buffers, the launch rules of its
// kernels, the stage loop and a solve's byte accounting; included by teeflow.hip after teeflow_engine.hip.h (one translation unit)
namespace {
int validate_params(Engine* h, const tf_params& p)
{
    if (p.algo != TF_ALGO_TVL1) return fail(h, TF_ERR_UNSUPPORTED, "algo %d not implemented (only TF_ALGO_TVL1)", p.algo);
    if (p.nscales < 1 || p.nscales > MAXLEV) return fail(h, TF_ERR_INVALID_ARG, "nscales must be in [1,%d], got %d", MAXLEV, p.nscales);
    if (p.warps < 1) return fail(h, TF_ERR_INVALID_ARG, "warps must be >= 1, got %d", p.warps);
    if (p.inner_iterations < 1 || p.outer_iterations < 1)
        return fail(h, TF_ERR_INVALID_ARG, "inner/outer iterations must be >= 1, got %d/%d", p.inner_iterations, p.outer_iterations);
    if ((long long)p.inner_iterations * p.outer_iterations > 100000)
        return fail(h, TF_ERR_INVALID_ARG, "inner*outer iterations too large");
    if (p.median_filtering != 1 && p.median_filtering != 3 && p.median_filtering != 5)
        return fail(h, TF_ERR_UNSUPPORTED, "medianFiltering must be 1, 3 or 5 (cv::medianBlur on CV_32F), got %d", p.median_filtering);
    if (p.gamma != 0.0) return fail(h, TF_ERR_UNSUPPORTED, "gamma != 0 (illumination term u3) is not implemented");
    if (p.variant != TF_VARIANT_CPU && p.variant != TF_VARIANT_CUDA) return fail(h, TF_ERR_INVALID_ARG, "variant must be TF_VARIANT_CPU or TF_VARIANT_CUDA, got %d", p.variant);
    if (p.variant == TF_VARIANT_CUDA && (p.inner_iterations * p.outer_iterations) % 2 != 0)
        return fail(h, TF_ERR_UNSUPPORTED, "TF_VARIANT_CUDA needs an even iteration count (inner*outer), got %d", p.inner_iterations * p.outer_iterations);
    if (p.use_initial_flow && p.variant == TF_VARIANT_CUDA)
        return fail(h, TF_ERR_UNSUPPORTED, "useInitialFlow is not implemented for TF_VARIANT_CUDA (nothing checks that form bit for bit)");
    if (!(p.scale_step > 0.0 && p.scale_step < 1.0)) return fail(h, TF_ERR_INVALID_ARG, "scaleStep must be in (0,1), got %g", p.scale_step);
    // cv::resize silently runs INTER_AREA instead of INTER_LINEAR when both scale factors are exactly 2 (imgproc/resize.cpp, "in
    // case of scale_x && scale_y is equal to 2"): same value mathematically, not the same float as the bilinear form k_pyr_down
    // computes.  That branch is not restated, so the one scaleStep that takes it is refused rather than silently different.
    if (p.scale_step == 0.5) return fail(h, TF_ERR_UNSUPPORTED, "scaleStep == 0.5 makes cv::resize take its INTER_AREA fast path for the pyramid, which is not implemented");
    if (!(p.theta > 0.0) || !(p.tau > 0.0) || !(p.lambda > 0.0) || !(p.epsilon >= 0.0))
        return fail(h, TF_ERR_INVALID_ARG, "tau, lambda, theta must be > 0 and epsilon >= 0");
    return TF_OK;
}

// pyramid geometry of DualTVL1::calc: dsize = cvRound(size*scaleStep); stop before a level < 16 px
int compute_levels(const tf_params& P, int H, int W, Geom* lv)
{
    int n = 1;
    lv[0] = make_geom(W, H);
    for (int s = 1; s < P.nscales; ++s) {
        const int w = cv_round_d(lv[s - 1].w * P.scale_step), hh = cv_round_d(lv[s - 1].h * P.scale_step);
        if (w < 16 || hh < 16) break;
        lv[s] = make_geom(w, hh);
        lv[s].splane = lv[0].plane;
        n = s + 1;
    }
    return n;
}

void Tvl1State::release()
{
    for (int l = 0; l < MAXLEV; ++l) { dev_free(pyr[l]); dev_free(gxl[l]); dev_free(gyl[l]); }
    dev_free(cwx); dev_free(cwy); dev_free(crho);
    for (int k = 0; k < 2; ++k) { dev_free(sb.u1[k]); dev_free(sb.u2[k]); dev_free(sb.p11[k]); dev_free(sb.p12[k]); dev_free(sb.p21[k]); dev_free(sb.p22[k]); }
    dev_free(ctl); dev_free(errs); dev_free(iters_dev); dev_free(chain_src);
    H = W = cap = nlev = 0; iters_cap = 0; chain_src_cap = 0;
}

// buffers for B pairs (at most a sub-batch) of H x W frames under the engine's current parameters; kept while they fit
int Tvl1State::ensure(Engine* e, int H_, int W_, int B)
{
    const tf_params& P = e->P;
    const int mb = P.max_batch > 0 ? P.max_batch : DEFAULT_MAX_BATCH;
    const int want_cap = B < mb ? B : mb;
    const int total = P.inner_iterations * P.outer_iterations;
    if (H == H_ && W == W_ && cap >= want_cap && scale_step == P.scale_step && nscales == P.nscales && errstride >= total &&
        variant == P.variant && iters_cap >= (size_t)cap * (size_t)nlev * (size_t)P.warps * 2)
        return TF_OK;
    HIPC(e, hipStreamSynchronize(e->stream));
    release(); release_staging(e);
    nlev = compute_levels(P, H_, W_, lv);
    const size_t ncap = (size_t)want_cap, fcap = 2 * ncap;
    for (int l = 0; l < nlev; ++l) HIPC(e, hipMalloc(&pyr[l], fcap * lv[l].plane * sizeof(float)));
    if (P.variant == TF_VARIANT_CUDA)
        for (int l = 0; l < nlev; ++l) {
            HIPC(e, hipMalloc(&gxl[l], fcap * lv[l].plane * sizeof(float)));
            HIPC(e, hipMalloc(&gyl[l], fcap * lv[l].plane * sizeof(float)));
        }
    variant = P.variant;
    const size_t pl = (size_t)lv[0].plane * ncap * sizeof(float);
    HIPC(e, hipMalloc(&cwx, pl)); HIPC(e, hipMalloc(&cwy, pl)); HIPC(e, hipMalloc(&crho, pl));
    for (int k = 0; k < 2; ++k) {
        HIPC(e, hipMalloc(&sb.u1[k], pl)); HIPC(e, hipMalloc(&sb.u2[k], pl));
        HIPC(e, hipMalloc(&sb.p11[k], pl)); HIPC(e, hipMalloc(&sb.p12[k], pl));
        HIPC(e, hipMalloc(&sb.p21[k], pl)); HIPC(e, hipMalloc(&sb.p22[k], pl));
    }
    HIPC(e, hipMalloc(&ctl, ncap * sizeof(PairCtl)));
    errstride = total;
    HIPC(e, hipMalloc(&errs, ncap * (size_t)errstride * sizeof(u64)));
    iters_cap = ncap * (size_t)nlev * (size_t)P.warps * 2;
    HIPC(e, hipMalloc(&iters_dev, iters_cap * sizeof(int)));
    H = H_; W = W_; cap = want_cap;
    scale_step = P.scale_step; nscales = P.nscales;
    return TF_OK;
}

inline dim3 grid64x4(const Geom& g, int z) { return dim3((g.w + 63) / 64, (g.h + 3) / 4, z); }

// full-width strips need W <= max_strip_width (at most 2048: one quad per thread, 512 threads) and enough rows*pairs to fill 256 CUs; tiny launches (single-pair latency mode) keep the tiles
bool rows_ok(const Engine* h, const Geom& g, int B)
{
    return h->iter_variant >= 1 && g.w <= h->max_strip_width && (long long)g.h * B >= h->min_rows_work;
}

// tvl1_iter iterations per launch for a stage whose medians come every `inner` iterations: 2 (k_iter2_rows / k_iter2_tile) or 1.
// TF_VARIANT_CUDA always runs the two-iteration form (it has no median, and its iteration count is even)
int iter_step(const Engine* h, bool cuda_variant, int inner)
{
    return (cuda_variant || (h->iter_variant >= 2 && inner % 2 == 0)) ? 2 : 1;
}

// Block shape of the row-strip kernels: QX quads per row, RY = floor(256/QX) rows per step, 256 threads.
// (Measured on MI355X: shapes that fill more lanes with 320-512-thread blocks, or 1-row/128-thread blocks, are 10-35 %
// SLOWER -- more waves per barrier domain / fewer blocks per CU cost more than idle lanes.)
void strip_shape(const Engine* h, const Geom& g, int B, int* R, int* QX, int* RY, int* threads)
{
    const int qx = (g.w + 3) / 4;
    int ry = 256 / qx;
    if (ry < 1) ry = 1;
    *QX = qx; *RY = ry;
    *threads = qx * ry <= 256 ? 256 : (qx * ry + 63) / 64 * 64;
    long long n = (long long)g.h * B / ((long long)h->strip_blocks * ry);
    if (n < 2) n = 2;
    if (n > 16) n = 16;
    *R = ry * (int)n;
}

// launch `step` (1 or 2) tvl1_iter iterations for pairs [0,B): strips or tiles by rows_ok; the one-iteration kernels take A.a alone
void launch_iter(Engine* h, const Iter2Args& A, int step, int B, hipStream_t s)
{
    const Geom& g = A.a.g;
    if (!rows_ok(h, g, B)) {      // small launches and very wide levels: tiles
        if (step == 2) hipLaunchKernelGGL(k_iter2_tile, dim3((g.w + T2_OW - 1) / T2_OW, (g.h + T2_OH - 1) / T2_OH, B), dim3(256), 0, s, A);
        else hipLaunchKernelGGL(k_iter, dim3((g.w + IT_OW - 1) / IT_OW, (g.h + IT_OH - 1) / IT_OH, B), dim3(256), 0, s, A.a);
        return;
    }
    int R, QX, RY, threads;
    strip_shape(h, g, B, &R, &QX, &RY, &threads);
    const int LW = QX * 4 + 4;
    if (step == 1) {
        const size_t shmem1 = (size_t)(32 + 8 * RY * LW + 2 * RY * QX) * sizeof(float);
        hipLaunchKernelGGL(k_iter_rows, dim3((g.h + R - 1) / R, 1, B), dim3(threads), shmem1, s, A.a, R, QX, RY);
        return;
    }
    const size_t shmem = (size_t)(32 + 8 * RY * LW + 2 * (RY + 1) * LW + 2 * RY * QX) * sizeof(float);
    if (B <= 1024) {
        // strips sized on the device from the exact number of pairs still iterating (one round of resident blocks); the grid covers
        // the largest item count
        auto f = h->tv.slots_cache.find(shmem * 1024 + (size_t)threads / 64);
        if (f == h->tv.slots_cache.end()) {
            int per_cu = 0;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_iter2_rows, threads, shmem);
            if (per_cu < 1) per_cu = 1;
            f = h->tv.slots_cache.emplace(shmem * 1024 + (size_t)threads / 64, per_cu * h->num_cus).first;
        }
        int slots = f->second;
        if (h->slots_pct > 0 && h->slots_pct < 100) slots = slots * h->slots_pct / 100;
        if (h->strip_test_slots >= 1) slots = h->strip_test_slots;
        int items = 1;
        for (int n = 1; n <= B; ++n) {
            int r, sn;
            strip_rule(n, g.h, RY, slots, &r, &sn);
            if (n * sn > items) items = n * sn;
        }
        hipLaunchKernelGGL(k_iter2_rows, dim3(items, 1, 1), dim3(threads), shmem, s, A, 0, QX, RY, slots);
        return;
    }
    // a sub-batch above 1024 pairs (max_batch > 1024): fixed strips of R rows per pair
    hipLaunchKernelGGL(k_iter2_rows, dim3((g.h + R - 1) / R, 1, B), dim3(threads), shmem, s, A, R, QX, RY, 0);
}

// k_warp_lds is instantiated for a few margins (the staged width is a compile-time constant)
inline int warp_margin_class(int m) { return m <= 0 ? 0 : (m <= 4 ? 4 : (m <= 8 ? 8 : 16)); }
void launch_warp(Engine* h, const WarpArgs& wa, int B, hipStream_t s, const float* gx = nullptr, const float* gy = nullptr)
{
    const Geom& g = wa.g;
    if (h->P.variant == TF_VARIANT_CUDA) {
        WarpCudaArgs ca; ca.w = wa; ca.gx = gx; ca.gy = gy;
        hipLaunchKernelGGL(k_warp_cuda, dim3((g.w + 63) / 64, (g.h + 3) / 4, B), dim3(256), 0, s, ca);
        return;
    }
    const int M = warp_margin_class(h->warp_margin);
    const dim3 grid((g.w + WL_TW - 1) / WL_TW, (g.h + WL_TH - 1) / WL_TH, B);
    const size_t shm = (size_t)(128 + (WL_TW + 2 * (M + 4)) * (WL_TH + 2 * M + 7)) * sizeof(float);
    switch (M) {
        case 4: hipLaunchKernelGGL(k_warp_lds<4>, grid, dim3(256), shm, s, wa); break;
        case 8: hipLaunchKernelGGL(k_warp_lds<8>, grid, dim3(256), shm, s, wa); break;
        case 16: hipLaunchKernelGGL(k_warp_lds<16>, grid, dim3(256), shm, s, wa); break;
        default: hipLaunchKernelGGL(k_warp, dim3((g.w + 63) / 64, (g.h + 3) / 4, B), dim3(256), 0, s, wa); break;
    }
}

// Read back the active-pair reports of this stage's launches [*checked, q] (a launch publishes its report when it starts): never more than
// DEFAULT_LAG launches unread.  *stop: a launch that no pair entered active -- the rest of the stage would be no-ops.
int read_reports(Engine* h, hipStream_t s, unsigned q, unsigned* checked, bool* stop)
{
    while (*checked <= q) {
        int v = h->tv.slots_host[*checked % SLOT_RING];
        if (v < 0) {
            if (q - *checked < (unsigned)DEFAULT_LAG) break;        // not there yet, and we may still run ahead
            const double t0 = now_ms();
            while ((v = h->tv.slots_host[*checked % SLOT_RING]) < 0) {
                if (now_ms() - t0 > 20000.0) return fail(h, TF_ERR_HIP, "tvl1_iter launch %u never reported (GPU hang?)", *checked);
                if (hipStreamQuery(s) == hipSuccess && h->tv.slots_host[*checked % SLOT_RING] < 0)
                    return fail(h, TF_ERR_HIP, "stream drained but launch %u did not report", *checked);
            }
        }
        ++*checked;
        if (v == 0) { *stop = true; break; }
    }
    return TF_OK;
}

// What the iteration loop of one (level, warp) stage works on and is told: run_stage fills it from the engine's buffers and parameters,
// tf_dbg_stage (teeflow_dbg.hip.h) from a caller's planes, so that the hook runs the loop a solve runs.
struct StageRun {
    const float *wx, *wy, *rho;          // the stage's warp constants, pair b at b * g.splane
    StateBufs sb; PairCtl* ctl;          // the ping-pong state and which half of it holds pair b
    u64* errs; int errstride;            // error slots, errstride >= inner * outer per pair; the loop clears them
    int* iters_dev;                      // k_stage_end files (n_it, n_out) of pair b at [b][nlev][warps][2], entry (l, wi)
    Geom g;
    int inner, total;                    // iterations between two medians; inner * outer
    int ksize;                           // medianFiltering: 3 or 5, anything else = none
    int variant;
    float thr_f; double thr_d;           // the stage's threshold as the CPU class keeps it (float) and as the CUDA class does (double)
    float l_t, theta, taut;
    int pzero;                           // the stage starts from p == 0: its first launch does not read the dual planes
    int l, wi, nlev, warps;
};

// the iteration loop of one stage for pairs [0,B): medians, tvl1_iter launches, the active-pair reports that end it early, k_stage_end
int run_stage_loop(Engine* h, const StageRun& r, int B)
{
    const Geom g = r.g;
    const int inner = r.inner, total = r.total;
    const double thr_q = (double)r.thr_f * 1073741824.0;
    hipStream_t s = h->stream;
    HIPC(h, hipMemsetAsync(r.errs, 0, (size_t)B * r.errstride * sizeof(u64), s));

    Iter2Args A;
    IterArgs& ia = A.a;
    ia.wx = r.wx; ia.wy = r.wy; ia.rho = r.rho; ia.sb = r.sb; ia.ctl = r.ctl; ia.err = r.errs;
    ia.errstride = r.errstride; ia.thr_q = thr_q; ia.g = g;
    ia.l_t = r.l_t; ia.theta = r.theta; ia.taut = r.taut;
    ia.variant = r.variant; ia.thr_d = r.thr_d;
    const bool cuda_variant = r.variant == TF_VARIANT_CUDA;      // one loop, no median, stops only after odd iterations
    const bool median = r.ksize > 1 && !cuda_variant;
    MedArgs ma;
    ma.sb = r.sb; ma.ctl = r.ctl; ma.err = r.errs; ma.errstride = r.errstride; ma.thr_q = thr_q; ma.g = g;

    const dim3 gm((g.w + 63) / 64, (g.h + 15) / 16, 2 * B);
    ia.B = B;
    // `step` iterations per launch.  Two: launch index it = 0,2,..,total (the last one can only hold REPLAY blocks), and each launch
    // is also told the ping-pong state of the one before it (the one-iteration kernels do not read it).
    const int step = iter_step(h, cuda_variant, inner);
    ma.total = A.total = total; ma.step = step;
    A.utog_prev = A.ptog_prev = A.pzero_prev = 0;
    int utog = 0, ptog = 0;
    bool stop = false;
    unsigned checked = h->tv.launch_seq;          // this stage's launches before `checked` have been read back
    for (int it = 0; it < total + step - 1 && !stop; it += step) {
        if (it < total && it % inner == 0 && median) {
            ma.it = it; ma.utog = utog;
            int rc = profiled(h, s, -5, 0, 0, [&] {
                if (r.ksize == 5) hipLaunchKernelGGL(k_median<5>, gm, dim3(256), 0, s, ma);
                else hipLaunchKernelGGL(k_median<3>, gm, dim3(256), 0, s, ma);
            });
            if (rc) return rc;
            ++utog;
        }
        const unsigned q = h->tv.launch_seq++;
        h->tv.slots_host[q % SLOT_RING] = -1;
        ia.host_slot = h->tv.slots_dev + q % SLOT_RING;
        ia.it = it; ia.utog = utog; ia.ptog = ptog; ia.pzero = (r.pzero && it == 0) ? 1 : 0;
        int rc = profiled(h, s, r.l, r.wi, it, [&] { launch_iter(h, A, step, B, s); });
        if (rc) return rc;
        ++h->tally.iter_launches;
        A.utog_prev = utog; A.ptog_prev = ptog; A.pzero_prev = ia.pzero;
        ++utog; ++ptog;
        rc = read_reports(h, s, q, &checked, &stop);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_stage_end, dim3((B + 255) / 256), dim3(256), 0, s, r.errs, r.errstride, r.ctl, r.iters_dev, B,
                       total, inner, median ? 1 : 0, thr_q, r.l, r.wi, r.nlev, r.warps, r.variant, r.thr_d, step);
    return TF_OK;
}

// one (level, warp) stage for pairs [0,B): the warp, then the loop; pair b's executed iteration counts go to iters_dev[b] (a chain
// step's pair: its own slice)
int run_stage(Engine* h, int l, int wi, int B, int off0, int off1, int* iters_dev)
{
    const tf_params& P = h->P;
    const Geom g = h->tv.lv[l];
    hipStream_t s = h->stream;

    WarpArgs wa;
    wa.pyr = h->tv.pyr[l]; wa.off0 = off0; wa.off1 = off1; wa.sb = h->tv.sb; wa.ctl = h->tv.ctl; wa.tab = h->tv.tab;
    wa.wx = h->tv.cwx; wa.wy = h->tv.cwy; wa.rho = h->tv.crho; wa.g = g;
    int rc = profiled(h, s, -4, 0, 0, [&] { launch_warp(h, wa, B, s, h->tv.gxl[l], h->tv.gyl[l]); });
    if (rc) return rc;

    StageRun r;
    r.wx = h->tv.cwx; r.wy = h->tv.cwy; r.rho = h->tv.crho; r.sb = h->tv.sb; r.ctl = h->tv.ctl;
    r.errs = h->tv.errs; r.errstride = h->tv.errstride; r.iters_dev = iters_dev; r.g = g;
    r.inner = P.inner_iterations; r.total = P.inner_iterations * P.outer_iterations;
    r.ksize = P.median_filtering; r.variant = P.variant;
    r.thr_f = (float)(P.epsilon * P.epsilon * (double)(g.w * g.h));
    r.thr_d = P.epsilon * P.epsilon * (double)(g.w * g.h);     // TF_VARIANT_CUDA compares in double
    r.l_t = (float)(P.lambda * P.theta); r.theta = (float)P.theta; r.taut = (float)(P.tau / P.theta);
    r.pzero = wi == 0 ? 1 : 0;
    r.l = l; r.wi = wi; r.nlev = h->tv.nlev; r.warps = P.warps;
    return run_stage_loop(h, r, B);
}

// level 0 of F frame slots -> the levels below it (and, TF_VARIANT_CUDA, the gradients)
void pyramids_below_level0(Engine* h, int F)
{
    const tf_params& P = h->P;
    hipStream_t s = h->stream;
    for (int l = 1; l < h->tv.nlev; ++l) {
        const double sc = 1.0 / P.scale_step;   // resize(src, Size(), fx, fy): scale = 1/fx
        hipLaunchKernelGGL(k_pyr_down, grid64x4(h->tv.lv[l], F), dim3(256), 0, s, h->tv.pyr[l - 1], h->tv.lv[l - 1], h->tv.pyr[l], h->tv.lv[l], sc, sc,
                           P.variant == TF_VARIANT_CUDA ? 1 : 0);
    }
    if (P.variant == TF_VARIANT_CUDA)
        for (int l = 0; l < h->tv.nlev; ++l)
            hipLaunchKernelGGL(k_grad, grid64x4(h->tv.lv[l], F), dim3(256), 0, s, h->tv.pyr[l], h->tv.gxl[l], h->tv.gyl[l], h->tv.lv[l]);
}

// frames[F][H][W] in device memory (uint8, or float32 in [0,1] when f32) -> their pyramids
void build_pyramids(Engine* h, const uint8_t* dframes, bool f32, int F)
{
    hipStream_t s = h->stream;
    const Geom g0 = h->tv.lv[0];
    if (f32) hipLaunchKernelGGL(k_f32_to_level0, dim3((g0.w + 255) / 256, g0.h, F), dim3(256), 0, s, (const float*)dframes, h->tv.pyr[0], g0, 1);
    else hipLaunchKernelGGL(k_u8_to_f32, dim3((g0.w + 255) / 256, g0.h, F), dim3(256), 0, s, dframes, h->tv.pyr[0], g0);
    pyramids_below_level0(h, F);
}

// Where a solve's level-0 initial flow comes from (useInitialFlow): nowhere (start from zero), the caller's interleaved flows, or -- a
// chain step -- the state planes of the pair's own slot as the pair solved there before has left them (a single chain: slot 0; chains in
// lock-step: slot s is chain s for the whole call).
enum Seed { SEED_ZERO, SEED_FLOWS, SEED_STATE };

// Solve B pairs of the pyramids build_pyramids has made, pair b = frames (off0+b, off1+b), in state slots [0,B): the seed, the level /
// warp stages, the output.  dinit (SEED_FLOWS): device float32 [B][H][W][2] in pixels per frame.  SEED_STATE: every slot of [0,B) holds
// the pair solved there before, untouched since; slots >= B are neither read nor written.  The executed
// iteration counts go to iters_dev[b], the flows, times `scale`, to dflow[b].
int solve_pairs(Engine* h, int B, int off0, int off1, Seed seed, const float* dinit, int* iters_dev, float scale, void* dflow, bool out_f16)
{
    const tf_params& P = h->P;
    hipStream_t s = h->stream;
    const Geom g0 = h->tv.lv[0];
    const int L = h->tv.nlev - 1;
    // useInitialFlow: u?s[0] = split(flow), u?s[l] = resize(u?s[l-1], Size(), scaleStep, scaleStep) * scaleStep, every level rounded to
    // float32 before the next is taken from it.  Level l lives in u buffer (L - l) & 1, so the coarsest one ends in buffer 0, which the
    // first stage reads (ubase = 0); the levels in between are scratch.  All but the last step run BEFORE the two memsets: a level in
    // between that sits in buffer 0 would otherwise write into the row padding they clear.
    const auto seed_step = [&](int l) {         // level l of the chain, from the caller's flow or the state (l == 0) or from level l - 1
        if (l > 0) hipLaunchKernelGGL(k_init_down, grid64x4(h->tv.lv[l], B), dim3(256), 0, s, h->tv.sb, (L - l + 1) & 1, h->tv.lv[l - 1], h->tv.lv[l],
                                      1.0 / P.scale_step, (float)P.scale_step);
        else if (seed == SEED_FLOWS) hipLaunchKernelGGL(k_init_split, grid64x4(g0, B), dim3(256), 0, s, dinit, h->tv.sb, L & 1, g0);
    };
    // A chain step's level 0 is the slot's last pair's flow, in the buffer that pair's ctl names (slot by slot: it depends on the
    // iterations the pair executed): k_chain_seed reads ctl before k_ctl_set resets it.  With one level that flow is itself what the first
    // stage reads, in buffer 0: the memsets, which would clear it, are left out, and the kernel clears the row padding in their place.
    if (seed == SEED_STATE)
        hipLaunchKernelGGL(k_chain_seed, dim3((g0.pitch + 63) / 64, (g0.h + 3) / 4, B), dim3(256), 0, s, h->tv.sb, h->tv.ctl, L & 1, g0, L == 0 ? 1 : 0);
    hipLaunchKernelGGL(k_ctl_set, dim3((B + 255) / 256), dim3(256), 0, s, h->tv.ctl, B, 0);
    if (seed != SEED_ZERO) for (int l = 0; l < L; ++l) seed_step(l);
    if (!(seed == SEED_STATE && L == 0)) {
        HIPC(h, hipMemset2DAsync(h->tv.sb.u1[0], (size_t)h->tv.lv[L].splane * sizeof(float), 0, (size_t)h->tv.lv[L].plane * sizeof(float), B, s));
        HIPC(h, hipMemset2DAsync(h->tv.sb.u2[0], (size_t)h->tv.lv[L].splane * sizeof(float), 0, (size_t)h->tv.lv[L].plane * sizeof(float), B, s));
    }
    if (seed != SEED_ZERO) seed_step(L);
    for (int l = L; l >= 0; --l) {
        for (int wi = 0; wi < P.warps; ++wi) {
            int rc = run_stage(h, l, wi, B, off0, off1, iters_dev);
            if (rc) return rc;
        }
        if (l == 0) break;
        const Geom gs = h->tv.lv[l], gd = h->tv.lv[l - 1];
        // resize(u, size(I0s[s-1])): inv_scale = dsize/ssize, scale = 1/inv_scale
        const double sx = 1.0 / ((double)gd.w / gs.w), sy = 1.0 / ((double)gd.h / gs.h);
        hipLaunchKernelGGL(k_flow_up, grid64x4(gd, B), dim3(256), 0, s, h->tv.sb, h->tv.ctl, gs, gd, sx, sy, (float)(1 / P.scale_step),
                           P.variant == TF_VARIANT_CUDA ? 1 : 0);
        hipLaunchKernelGGL(k_ctl_set, dim3((B + 255) / 256), dim3(256), 0, s, h->tv.ctl, B, 1);
    }
    if (out_f16) hipLaunchKernelGGL(k_output<uint16_t>, out_grid<uint16_t>(g0, B), dim3(256), 0, s, h->tv.sb, h->tv.ctl, g0, scale, (uint16_t*)dflow);
    else hipLaunchKernelGGL(k_output<float>, out_grid<float>(g0, B), dim3(256), 0, s, h->tv.sb, h->tv.ctl, g0, scale, (float*)dflow);
    HIPC(h, hipGetLastError());
    return TF_OK;
}

// Solve B pairs whose frames are in device memory: frames[F][H][W] (uint8, or float32 in [0,1] when f32), pair b = (off0+b, off1+b).
// dinit (useInitialFlow): the pairs' initial flows in device memory, float32 [B][H][W][2] in pixels per frame, or null = start from zero.
int solve_resident(Engine* h, const uint8_t* dframes, bool f32, int F, int B, int off0, int off1, float scale, void* dflow, bool out_f16,
                   const float* dinit = nullptr)
{
    build_pyramids(h, dframes, f32, F);
    return solve_pairs(h, B, off0, off1, dinit ? SEED_FLOWS : SEED_ZERO, dinit, h->tv.iters_dev, scale, dflow, out_f16);
}

// A chained sequence's sub-batch (useInitialFlow, tf_chain_next): the B pairs (k, k+1) of frames[B+1], solved one after the other in
// state slot 0, each seeded by the flow the pair before it has left there -- float32, in pixels per frame, before `scale` and before any
// float16 rounding: never read back from dflow.  The first pair starts from zero, or (`carry`: the call's later sub-batches) from what
// the sub-batch before has left: nothing between the two writes slot 0's planes or ctl.  Every frame's pyramid is built once; nothing
// here waits for the stream beyond what a stage's read_reports does.
int solve_chain_resident(Engine* h, const uint8_t* dframes, bool f32, int B, float scale, void* dflow, bool out_f16, bool carry)
{
    build_pyramids(h, dframes, f32, B + 1);
    const size_t per_pair = (size_t)h->tv.nlev * h->P.warps * 2;
    const size_t flb = (size_t)h->tv.H * h->tv.W * 2 * (out_f16 ? sizeof(uint16_t) : sizeof(float));
    for (int k = 0; k < B; ++k) {
        const int rc = solve_pairs(h, 1, k, k + 1, k > 0 || carry ? SEED_STATE : SEED_ZERO, nullptr, h->tv.iters_dev + (size_t)k * per_pair, scale,
                                   (uint8_t*)dflow + (size_t)k * flb, out_f16);
        if (rc) return rc;
        ++h->tally.chain_steps;
    }
    return TF_OK;
}

// Chains in lock-step (tf_calc_chains*): a sub-batch of T steps of up to S chains of one frame size.  dsrc: device table of (T+1) * S
// frame sources, time-major -- row t holds frame t of every chain, null where a chain has ended (k_chain_gather).  Step k solves the
// pairs (k * S + s, (k+1) * S + s) of the chains still running, s in [0, Bk[k]) -- the chains are ordered longest first, so those are a
// prefix and Bk never grows -- as one batch through solve_pairs, every pair seeded by the flow its own slot holds (step 0 of the call:
// from zero; `carry`: this sub-batch continues the one before, whose state nothing has written since).  A pair's solve does not depend
// on the batch it is in, so chain s gets what a chain of its own would.  Iteration counts go to iters_dev, flows to dflow, both
// time-major with S slots per step; the slots of ended chains stay unwritten.
int solve_chains_resident(Engine* h, const void* const* dsrc, bool f32, int S, int T, const int* Bk, float scale, void* dflow, bool out_f16, bool carry)
{
    const Geom g0 = h->tv.lv[0];
    const int F = (T + 1) * S;
    hipLaunchKernelGGL(k_chain_gather, dim3((g0.w + 255) / 256, g0.h, F), dim3(256), 0, h->stream, dsrc, f32 ? 1 : 0, h->tv.pyr[0], g0);
    pyramids_below_level0(h, F);
    const size_t per_pair = (size_t)h->tv.nlev * h->P.warps * 2;
    const size_t flb = (size_t)h->tv.H * h->tv.W * 2 * (out_f16 ? sizeof(uint16_t) : sizeof(float));
    for (int k = 0; k < T; ++k) {
        const int rc = solve_pairs(h, Bk[k], k * S, (k + 1) * S, k > 0 || carry ? SEED_STATE : SEED_ZERO, nullptr,
                                   h->tv.iters_dev + (size_t)k * S * per_pair, scale, (uint8_t*)dflow + (size_t)k * S * flb, out_f16);
        if (rc) return rc;
        h->tally.chain_steps += Bk[k];
    }
    return TF_OK;
}

// algorithmic (compulsory) HBM bytes of one solved pair from its executed iteration counts
// seeded: the pair started from a caller's flow (useInitialFlow)
void account_bytes(const Engine* h, const int* it /* [nlev][warps][2] */, bool seeded, double* iter_bytes, double* total_bytes,
                   unsigned long long* n_in, unsigned long long* n_out)
{
    const int warps = h->P.warps;
    double ib = 0, tb = 0;
    for (int l = 0; l < h->tv.nlev; ++l) {
        const double px = (double)h->tv.lv[l].w * h->tv.lv[l].h;
        for (int w = 0; w < warps; ++w) {
            const int ni = it[(l * warps + w) * 2], no = it[(l * warps + w) * 2 + 1];
            *n_in += ni; *n_out += no;
            ib += px * 60.0 * ni;                                   // tvl1_iter: 9 reads + 6 writes
            tb += px * (16.0 * (h->P.median_filtering > 1 ? no : 0)  // median: read+write u1,u2
                        + 28.0);                                    // warp: read I0,I1,u1,u2; write I1wx,I1wy,rho_c
        }
        if (l > 0) tb += px * 8.0 + (double)h->tv.lv[l - 1].w * h->tv.lv[l - 1].h * 8.0;          // flow upsample
        if (l > 0) tb += 2.0 * (px * 4.0 + (double)h->tv.lv[l - 1].w * h->tv.lv[l - 1].h * 4.0);  // pyramid level (2 frames)
        if (seeded) tb += l > 0 ? px * 8.0 + (double)h->tv.lv[l - 1].w * h->tv.lv[l - 1].h * 8.0  // initial flow: one level down,
                                : px * 16.0;                                                    //   or the split of the caller's
    }
    tb += (double)h->tv.lv[0].w * h->tv.lv[0].h * (2.0 * (1 + 4) + 8.0 + 8.0);  // u8->f32 of 2 frames, output interleave
    *iter_bytes += ib; *total_bytes += tb + ib;
}
}  // namespace
