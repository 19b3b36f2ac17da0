// teeflow_deepflow_host.hip.h -- DeepFlow's host side: parameters, pyramid geometry, DfState's buffers, the co-resident SOR form's
// state (Coop) and launch rules, the refinement of a level and a solve's byte accounting; included by teeflow.hip after
// teeflow_tvl1_host.hip.h (one translation unit)
namespace {
int df_levels(const tf_deepflow_params& P, int H, int W, Geom* lv)
{
    int n = 1;
    lv[0] = make_geom(W, H);
    while (n < DF_MAXLEV) {
        // Size((int)(cols*downscaleFactor + 0.5f), (int)(rows*downscaleFactor + 0.5f)), float arithmetic
        const int nw = (int)(lv[n - 1].w * P.downscale_factor + 0.5f), nh = (int)(lv[n - 1].h * P.downscale_factor + 0.5f);
        if (nh <= P.min_size || nw <= P.min_size) break;
        lv[n] = make_geom(nw, nh);
        lv[n].splane = lv[0].plane;
        ++n;
    }
    return n;
}

int df_validate(Engine* h, const tf_deepflow_params& p)
{
    if (!(p.sigma > 0.f) || (int)floorf(3 * p.sigma) * 2 + 1 != 3)
        return fail(h, TF_ERR_UNSUPPORTED, "DeepFlow pre-blur: only the 3x3 kernel (1/3 <= sigma < 2/3) is implemented, sigma=%g", p.sigma);
    if (!(p.downscale_factor > 0.1f && p.downscale_factor < 1.f)) return fail(h, TF_ERR_INVALID_ARG, "downscaleFactor must be in (0.1,1)");
    if (p.min_size < 1 || p.fixed_point_iterations < 0 || p.sor_iterations < 0 || p.fixed_point_iterations > 1000 || p.sor_iterations > 10000)
        return fail(h, TF_ERR_INVALID_ARG, "bad DeepFlow iteration/size parameters");
    return TF_OK;
}

// one sub-batch solved: an engine that is sitting out an abort comes one step closer to trying the co-resident form again
void Coop::tick()
{
    if (disabled && cooldown > 0 && --cooldown == 0) { disabled = false; ++rearms; }
}
// The co-resident form counts on ONE 1024-thread block (128 x 64 regions) or TWO 512-thread blocks (128 x 32) per CU.  Ask the runtime
// instead of assuming it: a build whose register or LDS use has grown past that is refused the form (the tiled one does the same work).
void Coop::query_occupancy(const TfKnobs& k)
{
    if (occ16 >= 0 && asked16 == k.coop_test_occ16 && asked8 == k.coop_test_occ8) return;
    asked16 = k.coop_test_occ16; asked8 = k.coop_test_occ8;
    int a = 0, b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_df_sor_rt_coop<4, 16>, 1024, 0) != hipSuccess) a = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_df_sor_rt_coop<4, 8>, 512, 0) != hipSuccess) b = 0;
    (void)hipGetLastError();
    occ16 = k.coop_test_occ16 >= 0 ? k.coop_test_occ16 : a;
    occ8 = k.coop_test_occ8 >= 0 ? k.coop_test_occ8 : b;
}
// k_df_sor_rt_coop's meeting place: a flag line per block that can be resident (one per CU) + the abort word behind them
int Coop::ensure(Engine* e)
{
    if (flags) return TF_OK;
    flag_lines = 2 * e->num_cus;          // 128 x 32 regions: two 512-thread blocks per CU
    HIPC(e, hipMalloc(&flags, ((size_t)flag_lines + 1) * 128));
    HIPC(e, hipMemsetAsync(flags, 0, ((size_t)flag_lines + 1) * 128, e->stream));
    epoch = 0;
    query_occupancy(*e);
    return TF_OK;
}
void Coop::release() { dev_free(flags); flag_lines = 0; }
// after the stream has drained: did a launch of this call give up waiting?  Then the results are void: the tiled form from now on.
int Coop::aborted(Engine* e, bool* aborted)
{
    *aborted = false;
    if (!used || !flags) return TF_OK;
    used = false;
    unsigned word = 0;
    HIPC(e, hipMemcpy(&word, flags + (size_t)flag_lines * 32, sizeof word, hipMemcpyDeviceToHost));
    if (!word) return TF_OK;
    // Back-off, not a verdict: whatever held the CUs (another process, another stream) is usually gone a few solves later.  Sit out
    // 16 tiled sub-batches, twice as many after every further abort (capped), then try the form again (tick).
    disabled = true;
    ++aborts;
    backoff = backoff ? (backoff < 4096 ? 2 * backoff : 4096) : 16;
    cooldown = backoff;
    e->err = "co-resident SOR launch gave up waiting (foreign work on the GPU?): sub-batch repeated with the tiled form";   // readable through tf_last_error
    HIPC(e, hipMemset(flags, 0, ((size_t)flag_lines + 1) * 128));
    *aborted = true;
    return TF_OK;
}
// Two launches of co-resident regions that each count on the same CUs can wait for each other for ever (each holds CUs the other's
// last blocks need), so at most one call (or one lane pool with jobs outstanding) per device and process may use the form at a time;
// a pool's lanes split the CUs between them.
static std::atomic<int> g_coop_busy[64];
bool coop_claim(int dev) { int z = 0; return dev >= 0 && dev < 64 && g_coop_busy[dev].compare_exchange_strong(z, 1); }
void coop_release(int dev) { g_coop_busy[dev].store(0); }
struct CoopClaim {
    int dev; bool ok;
    explicit CoopClaim(int dev_) : dev(dev_), ok(coop_claim(dev_)) {}
    ~CoopClaim() { if (ok) coop_release(dev); }
};

// the state planes of a refinement, `stride` floats apart from `base` on
constexpr int DF_PLANES = 23;
void df_carve(DfBufs& d, float* base, size_t stride)
{
    float** slots[] = {&d.avg, &d.Iz, &d.Ix, &d.Iy, &d.Ixx, &d.Ixy, &d.Iyy, &d.Ixz, &d.Iyz, &d.A11, &d.A12, &d.A22, &d.b1, &d.b2, &d.wg,
                       &d.du, &d.dv, &d.du2, &d.dv2, &d.Wu[0], &d.Wu[1], &d.Wv[0], &d.Wv[1]};
    for (auto s_ : slots) { *s_ = base; base += stride; }
}

void DfState::release()
{
    dev_free(pyr_base); dev_free(tmp); dev_free(planes);
    nlev = H = W = cap = 0;
}

// buffers for B pairs (at most a sub-batch) of H x W frames, kept while they fit; the co-resident form's flags start over with them
int DfState::ensure(Engine* e, int H_, int W_, int B)
{
    const int mb = e->DP.max_batch > 0 ? e->DP.max_batch : DEFAULT_MAX_BATCH;
    const int want = B < mb ? B : mb;
    if (H == H_ && W == W_ && cap >= want) return TF_OK;
    HIPC(e, hipStreamSynchronize(e->stream));
    release(); e->coop.release(); release_staging(e);
    nlev = df_levels(e->DP, H_, W_, lv);
    const size_t ncap = (size_t)want, F = 2 * ncap;
    size_t total = 0;
    for (int l = 0; l < nlev; ++l) { pyr_off[l] = total; total += F * (size_t)lv[l].plane; }
    HIPC(e, hipMalloc(&pyr_base, total * sizeof(float)));
    HIPC(e, hipMalloc(&tmp, F * (size_t)lv[0].plane * sizeof(float)));
    const size_t pl = (size_t)lv[0].plane * ncap;
    HIPC(e, hipMalloc(&planes, DF_PLANES * pl * sizeof(float)));
    df_carve(bufs, planes, pl);
    const int rc = e->coop.ensure(e);
    if (rc) return rc;
    H = H_; W = W_; cap = want;
    return TF_OK;
}

DfConst df_consts(const tf_deepflow_params& P)
{
    // OpticalFlowDeepFlow::calc: var->setAlpha(4*alpha); setDelta(delta/3); setGamma(gamma/3)
    const float alpha = 4 * P.alpha, delta = P.delta / 3, gamma = P.gamma / 3;
    DfConst c;
    c.zeta2 = P.zeta * P.zeta; c.eps2 = P.epsilon * P.epsilon;
    c.delta2 = delta / 2; c.gamma2 = gamma / 2; c.alpha2 = alpha / 2; c.omega = P.omega;
    return c;
}

void df_gauss3(float sigma, float* k0, float* k1)
{
    // getGaussianKernel(3, sigma, CV_32F): normalised in double, cast to float
    const double s2 = -0.5 / ((double)sigma * (double)sigma);
    const double t0 = exp(s2 * 1.0), t1 = exp(0.0);
    const double inv = 1.0 / (t0 + t1 + t0);
    *k0 = (float)(t1 * inv); *k1 = (float)(t0 * inv);
}

// regions of `size` px along one axis that cover `extent` px when neighbours overlap by a halo of hl on each side (the first region
// holds `size` px, every further one adds size - 2 hl)
inline int sor_regions(int extent, int size, int hl)
{
    return extent <= size ? 1 : 1 + (extent - size + (size - 2 * hl) - 1) / (size - 2 * hl);
}

// register-tile SOR (teeflow_sor_rt.hip.h): `sweeps` sweeps per launch on 128 x (R*NB) regions with a halo of hl = 2 * sweeps
// (hl = 0: the region holds the whole level)
template <int R, int NB>
void launch_sor_rt_t(const DfBufs& d, const Geom& g, int B, float omega, int sweeps, int hl, hipStream_t s, int plain_div)
{
    const int nx = sor_regions(g.w, 128, hl), ny = sor_regions(g.h, R * NB, hl);
    hipLaunchKernelGGL((k_df_sor_rt<R, NB>), dim3(nx, ny, B), dim3(64 * NB), 0, s, d, g, omega, sweeps, hl, plain_div);
}
// returns the number of sweeps it ran (all of `left` when the level fits one region).
// Region shapes: 128 x 64 held by 16 bands x 4 rows (1024 threads, one block per CU) is the throughput shape -- least halo.  When it
// would leave most of the chip idle (a single pair, or the small levels of a batch: fewer blocks than CUs) the same 4-row bands are
// stacked only 8 high: 128 x 32 regions, 512 threads, two blocks per CU, ~2.5x the blocks and half the sweep time per block -- as
// long as they all fit one round of resident blocks.  (64 pairs @512^2 are unaffected; single pair 27.3 -> see DESIGN.md.)
int launch_sor_rt(Engine* h, const DfBufs& d, const Geom& g, int B, float omega, int left, int fuse, hipStream_t s)
{
    auto tiles = [&](int RH, int hl) { return sor_regions(g.w, 128, hl) * sor_regions(g.h, RH, hl); };
    int shape = h->sor_rt_shape;
    if (shape == 3 && g.w <= 62 && g.h <= 128) {
        // a level this narrow fills at most half a wave: two bands per wave (k_df_sor_rt<.., HALF>), all sweeps in one launch
        if (g.h <= 64) hipLaunchKernelGGL((k_df_sor_rt<4, 8, true>), dim3(1, 1, B), dim3(512), 0, s, d, g, omega, left, 0, h->sor_plain_div);
        else hipLaunchKernelGGL((k_df_sor_rt<4, 16, true>), dim3(1, 1, B), dim3(1024), 0, s, d, g, omega, left, 0, h->sor_plain_div);
        return left;
    }
    const bool whole64 = g.w <= 128 && g.h <= 64, whole32 = g.w <= 128 && g.h <= 32;
    if (shape == 3) {
        shape = 1;
        const int n5 = left < fuse ? left : fuse;
        if (whole32) shape = 2;                                            // fits 8 bands: half the waves, same sweeps
        else if (!whole64 && 32 - 4 * n5 >= 8 && tiles(64, 2 * n5) * B < h->num_cus && tiles(32, 2 * n5) * B <= 2 * h->num_cus) shape = 2;
    }
    const bool whole = shape == 2 ? whole32 : whole64;
    int n = whole ? left : (left < fuse ? left : fuse);
    if (!whole && shape == 2 && 32 - 4 * n < 4) n = 6;                     // 128 x 32 regions: at most 6 sweeps per launch (core of 8 rows)
    if (n > left) n = left;
    const int hl = whole ? 0 : 2 * n;
    if (shape == 2) launch_sor_rt_t<4, 8>(d, g, B, omega, n, hl, s, h->sor_plain_div);
    else launch_sor_rt_t<4, 16>(d, g, B, omega, n, hl, s, h->sor_plain_div);
    return n;
}

// Co-resident form (k_df_sor_rt_coop): regions of a level and how many pairs' worth of them this handle may keep resident at once
// (0: the level is one region, or its regions do not fit -- tiled / whole-level form)
int sor_coop_pairs(const Engine* h, const Geom& g, int B, int S, int* nx_, int* ny_, int* rows_)
{
    const int hl = 2 * S;
    *rows_ = 64;
    if (!h->sor_coop || h->coop.disabled || !h->coop.flags || h->sor_rt_shape != 3 || 64 - 2 * hl < 8 || 3 * hl > 64) return 0;
    if (h->coop.occ16 < 1) return 0;                        // the runtime does not promise a resident 1024-thread block per CU: no co-resident form
    const int nx = sor_regions(g.w, 128, hl), ny = sor_regions(g.h, 64, hl);
    const int share = h->coop.share < h->coop.flag_lines / 2 ? h->coop.share : h->coop.flag_lines / 2;
    if (nx * ny < 2 || nx * ny > share) return 0;
    // few pairs: 128 x 64 regions would leave most CUs idle for the whole fixed-point iteration.  Like the tiled form (launch_sor_rt) the
    // co-resident one then takes 128 x 32 regions: 512-thread blocks, two per CU, ~2.5 x the blocks and half the sweep time per block
    const int ny32 = sor_regions(g.h, 32, hl);
    // (a region waits for the 8 regions around it, so its halo must not reach past their cores: hl <= core, i.e. 3 hl <= 32 -- S <= 5;
    // the 64-row regions satisfy 3 hl <= 64 for every S the knob allows)
    if (h->sor_coop != 2 && 32 - 2 * hl >= 8 && 3 * hl <= 32 && nx * ny * B < h->num_cus && nx * ny32 * B <= 2 * h->num_cus) {
        if (h->sor_coop != 3 && !h->sor_coop_small) return 0;
        if (h->coop.occ8 < 2) return 0;                     // two resident 512-thread blocks per CU are what this form counts on
        if (nx * ny32 < 2 || nx * ny32 * B > 2 * share) return 0;
        *nx_ = nx; *ny_ = ny32; *rows_ = 32;
        return B;                                                       // all of them in one launch
    }
    // Whole pairs only: a batch goes through in ceil(B / cp) launches that each hold `share` CUs, the tiled form needs
    // ceil(B * regions / share) rounds of blocks.  Where whole pairs leave much of the share empty (one pair of 66 regions on 128 CUs)
    // the tiled form is quicker although it loads the system five times: co-resident only if its launches are nearly as full.
    const int cp = share / (nx * ny);
    const long long groups = (B + cp - 1) / cp, rounds_t = ((long long)B * nx * ny + share - 1) / share;
    if (h->sor_coop == 1 && rounds_t * 100 < (long long)h->sor_coop_min_util * groups) return 0;
    *nx_ = nx; *ny_ = ny;
    return cp;
}

// one cv::VariationalRefinement::calcUV for pairs [0,B) on level geometry g: W[cur] -> (avg, Iz) = W + dW
int df_refine_level(Engine* h, const float* pyr_l, int off0, int off1, const Geom& g, int cur, int B, hipStream_t s)
{
    DfBufs d = h->df.bufs;
    const DfConst c = df_consts(h->DP);
    const dim3 gr = grid64x4(g, B), bl(256);
    const dim3 gsor(((g.w + 1) / 2 + 63) / 64, (g.h + 3) / 4, B);
    hipLaunchKernelGGL(k_df_warp, gr, bl, 0, s, pyr_l, off0, off1, d, cur, g);
    hipLaunchKernelGGL(k_df_grad1, gr, bl, 0, s, d, g);
    hipLaunchKernelGGL(k_df_grad2, gr, bl, 0, s, d, g);
    const int fuse = h->sor_fuse < 0 ? 0 : h->sor_fuse;
    for (int fp = 0; fp < h->DP.fixed_point_iterations; ++fp) {
        if (h->df_fuse_ds) hipLaunchKernelGGL(k_df_data_smooth4, dim3((g.w + 255) / 256, (g.h + 3) / 4, B), bl, 0, s, d, cur, g, c);
        else {
            hipLaunchKernelGGL(k_df_data, gr, bl, 0, s, d, cur, g, c);
            hipLaunchKernelGGL(k_df_smooth, gr, bl, 0, s, d, cur, g);
        }
        int left = h->DP.sor_iterations;
        int cnx = 0, cny = 0, crows = 64;
        const int S = h->sor_coop_s < 1 ? 1 : (h->sor_coop_s > 8 ? 8 : h->sor_coop_s);
        const int cpairs = h->sor_rt && fuse > 0 && left > S ? sor_coop_pairs(h, g, B, S, &cnx, &cny, &crows) : 0;
        if (cpairs > 0) {
            // all `left` sweeps in one launch per group of pairs; the result is in (du2, dv2) after an odd number of phases
            const int phases = (left + S - 1) / S;
            if (h->coop.epoch > (1u << 30)) {            // flags are compared as signed differences: start over long before a stale line could look ahead
                (void)hipMemsetAsync(h->coop.flags, 0, (size_t)h->coop.flag_lines * 128, s);
                h->coop.epoch = 0;
            }
            for (int b0 = 0; b0 < B; b0 += cpairs) {
                const int nb = B - b0 < cpairs ? B - b0 : cpairs;
                const int rc = profiled(h, s, 0, 0, 0, [&] {
                    if (crows == 32)
                        hipLaunchKernelGGL((k_df_sor_rt_coop<4, 8>), dim3(cnx, cny, nb), dim3(512), 0, s, d, g, c.omega, left, S, h->sor_plain_div | (h->coop_test_mute ? 2 : 0), b0,
                                           h->coop.flags, h->coop.epoch, h->coop.flags + (size_t)h->coop.flag_lines * 32);
                    else
                        hipLaunchKernelGGL((k_df_sor_rt_coop<4, 16>), dim3(cnx, cny, nb), dim3(1024), 0, s, d, g, c.omega, left, S, h->sor_plain_div | (h->coop_test_mute ? 2 : 0), b0,
                                           h->coop.flags, h->coop.epoch, h->coop.flags + (size_t)h->coop.flag_lines * 32);
                });
                if (rc) return rc;
                ++h->tally.iter_launches;
                h->coop.epoch += (unsigned)phases;
                ++h->coop.launches;
                h->tally.df_sor_bytes += (double)left * g.w * g.h * nb * 40.0;
                h->tally.df_sor_px += (double)g.w * g.h * nb;
            }
            h->coop.used = true;
            if (phases & 1) { std::swap(d.du, d.du2); std::swap(d.dv, d.dv2); }
            left = 0;
        }
        while (h->sor_rt && fuse > 0 && left > 0) {
            int n = 0;
            const int rc = profiled(h, s, 0, 0, 0, [&] { n = launch_sor_rt(h, d, g, B, c.omega, left, fuse > 8 ? 8 : fuse, s); });
            if (rc) return rc;
            ++h->tally.iter_launches;
            h->tally.df_sor_bytes += (double)n * g.w * g.h * B * 40.0;
            h->tally.df_sor_px += (double)g.w * g.h * B;
            std::swap(d.du, d.du2); std::swap(d.dv, d.dv2);
            left -= n;
        }
        while (left > 0) {     // sor_fuse = 0 (or sor_rt = 0): one colour per launch, in place -- the plain form the others are tested against
            hipLaunchKernelGGL(k_df_sor, gsor, bl, 0, s, d, g, 0, c.omega);
            hipLaunchKernelGGL(k_df_sor, gsor, bl, 0, s, d, g, 1, c.omega);
            h->tally.df_sor_bytes += (double)g.w * g.h * B * 40.0;
            --left;
        }
    }
    hipLaunchKernelGGL(k_df_sum, gr, bl, 0, s, d, cur, g);
    return TF_OK;
}

int df_solve_resident(Engine* h, const uint8_t* dframes, bool f32, int F, int B, int off0, int off1, float scale, void* dflow, bool out_f16)
{
    hipStream_t s = h->stream;
    const Geom g0 = h->df.lv[0];
    float k0, k1;
    df_gauss3(h->DP.sigma, &k0, &k1);
    // convertTo(CV_32F) without a factor: uint8 frames keep 0..255, float frames (a saliency map in [0,1]) are taken as they are
    if (f32) hipLaunchKernelGGL(k_f32_to_level0, dim3((g0.w + 255) / 256, g0.h, F), dim3(256), 0, s, (const float*)dframes, h->df.tmp, g0, 0);
    else hipLaunchKernelGGL(k_u8_to_f32, dim3((g0.w + 255) / 256, g0.h, F), dim3(256), 0, s, dframes, h->df.tmp, g0);
    hipLaunchKernelGGL(k_df_blur, grid64x4(g0, F), dim3(256), 0, s, h->df.tmp, h->df.pyr_base + h->df.pyr_off[0], g0, k0, k1);
    for (int l = 1; l < h->df.nlev; ++l) {
        const Geom gs = h->df.lv[l - 1], gd = h->df.lv[l];
        const double sx = 1.0 / ((double)gd.w / gs.w), sy = 1.0 / ((double)gd.h / gs.h);
        hipLaunchKernelGGL(k_pyr_down, grid64x4(gd, F), dim3(256), 0, s, h->df.pyr_base + h->df.pyr_off[l - 1], gs, h->df.pyr_base + h->df.pyr_off[l], gd, sx, sy);
    }
    const int L = h->df.nlev - 1;
    int cur = 0;
    HIPC(h, hipMemset2DAsync(h->df.bufs.Wu[0], (size_t)g0.plane * sizeof(float), 0, (size_t)h->df.lv[L].plane * sizeof(float), B, s));
    HIPC(h, hipMemset2DAsync(h->df.bufs.Wv[0], (size_t)g0.plane * sizeof(float), 0, (size_t)h->df.lv[L].plane * sizeof(float), B, s));
    const float mul = 1.0f / h->DP.downscale_factor;
    for (int l = L; l >= 0; --l) {
        const Geom g = h->df.lv[l];
        const int rc = df_refine_level(h, h->df.pyr_base + h->df.pyr_off[l], off0, off1, g, cur, B, s);
        if (rc) return rc;
        if (l == 0) break;
        const Geom gd = h->df.lv[l - 1];
        const double sx = 1.0 / ((double)gd.w / g.w), sy = 1.0 / ((double)gd.h / g.h);
        hipLaunchKernelGGL(k_df_up, grid64x4(gd, B), dim3(256), 0, s, h->df.bufs, cur, g, gd, sx, sy, mul);
        cur ^= 1;
    }
    if (out_f16) hipLaunchKernelGGL(k_df_out<uint16_t>, out_grid<uint16_t>(g0, B), dim3(256), 0, s, h->df.bufs, g0, scale, (uint16_t*)dflow);
    else hipLaunchKernelGGL(k_df_out<float>, out_grid<float>(g0, B), dim3(256), 0, s, h->df.bufs, g0, scale, (float*)dflow);
    HIPC(h, hipGetLastError());
    return TF_OK;
}

// algorithmic bytes of one DeepFlow pair (fp32 planes touched once per kernel)
double df_account_bytes(const Engine* h)
{
    double tb = 0;
    for (int l = 0; l < h->df.nlev; ++l) {
        const double px = (double)h->df.lv[l].w * h->df.lv[l].h;
        const double per_fp = (10 + 3 + 6) * 4.0 /*data*/ + (4 + 3 + 4) * 4.0 /*smooth*/ + h->DP.sor_iterations * 2 * 10 * 4.0 /*SOR colour passes*/;
        tb += px * ((4 + 4) * 4.0 /*warp*/ + (2 + 4 + 2 + 3) * 4.0 /*grads*/ + h->DP.fixed_point_iterations * per_fp + 6 * 4.0 /*sum*/ + 4 * 4.0 /*up*/);
    }
    return tb;
}
}  // namespace
