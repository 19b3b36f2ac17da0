// teeflow.hip -- host driver + C ABI (include/teeflow.h) of the MI355X DualTVL1 engine.
//
// Replaces, for the reference's hot path only, what cv2's DenseOpticalFlow object does behind
// the reference's optical_flow/calculate_optical_flow.py:564-600, 627-642.  No CPU fallback: without a
// gfx950 device tf_create fails with TF_ERR_NO_DEVICE.
//
// Execution model: a batch of B frame pairs advances in lock-step through
//   pyramid -> for level (coarse..fine): for warp: k_warp, then [median every `inner` iterations,
//   tvl1_iter] until each pair's own convergence test stops it.
// The stop decision lives on the device (per-pair error slots, blocks of stopped pairs exit at once);
// each tvl1_iter launch publishes "pairs still iterating" to a host-mapped word, which the host reads a few
// launches later to stop enqueuing a stage -- it never stalls the stream inside the iteration budget.
// The host side is cut by what it serves, all of it one translation unit: teeflow_engine.hip.h (Engine, tf_handle, the one-shot flags), the solvers'
// teeflow_tvl1_host.hip.h and teeflow_deepflow_host.hip.h, teeflow_queue.hip.h (a call's way to an engine or to the lanes), this file's C ABI entry points, then
// the study tail, a host header per topic beside its kernel header (listed where they are included; teeflow_scratch.hip.h and teeflow_streams_host.hip.h, what
// the topics share, come first), teeflow_comm.hip.h (RCCL) and teeflow_dbg.hip.h (test hooks).
// The device side is one header per kernel family; teeflow_kernels.hip.h holds what the solvers share and includes DualTVL1's
// stages (teeflow_tvl1_warp / _iter / _median.hip.h) and the tail's frame conditioning (teeflow_cond.hip.h); teeflow_wave_stage.hip.h is
// the staged reader that teeflow_inflate.hip.h, teeflow_rle.hip.h, teeflow_jpeg.hip.h and teeflow_jpegll.hip.h share.
#include "teeflow_kernels.hip.h"
#include "teeflow_deepflow.hip.h"
#include "teeflow_sor_rt.hip.h"
#include "teeflow_analysis.hip.h"
#include "teeflow_wase.hip.h"
#include "teeflow_saliency.hip.h"
#include "teeflow_ccl.hip.h"
#include "teeflow_masks.hip.h"
#include "teeflow_otsu.hip.h"
#include "teeflow_centroid.hip.h"
#include "teeflow_area.hip.h"
#include "teeflow_polar.hip.h"
#include "teeflow_overlay.hip.h"
#include "teeflow_magoverlay.hip.h"
#include "teeflow_segmentor.hip.h"
#include "teeflow_inflate.hip.h"
#include "teeflow_deflate.hip.h"
#include "teeflow_ingest.hip.h"
#include "teeflow_rle.hip.h"
#include "teeflow_jpeg.hip.h"
#include "teeflow_jpegll.hip.h"
#include "pil_resample_tables.h"
#include "../../include/teeflow.h"
#include "teeflow_engine.hip.h"
#include "teeflow_tvl1_host.hip.h"
#include "teeflow_deepflow_host.hip.h"
#include "teeflow_queue.hip.h"

// =================================================================================================
// C ABI
// =================================================================================================
TF_API int tf_abi_version(void) { return TF_ABI_VERSION; }

TF_API int tf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

TF_API int tf_default_params(tf_params* p)
{
    if (!p) return TF_ERR_INVALID_ARG;
    p->tau = 0.25; p->lambda = 0.15; p->theta = 0.3; p->epsilon = 0.01; p->scale_step = 0.8; p->gamma = 0.0;
    p->nscales = 5; p->warps = 5; p->inner_iterations = 30; p->outer_iterations = 10; p->median_filtering = 5;
    p->use_initial_flow = 0; p->algo = TF_ALGO_TVL1; p->max_batch = 0; p->variant = TF_VARIANT_CPU;
    return TF_OK;
}

TF_API int tf_default_deepflow_params(tf_deepflow_params* p)
{
    if (!p) return TF_ERR_INVALID_ARG;
    p->sigma = 0.6f; p->min_size = 25; p->downscale_factor = 0.95f; p->fixed_point_iterations = 5; p->sor_iterations = 25;
    p->alpha = 1.0f; p->delta = 0.5f; p->gamma = 5.0f; p->omega = 1.6f; p->zeta = 0.1f; p->epsilon = 0.001f; p->max_batch = 0;
    return TF_OK;
}

TF_API int tf_create_deepflow(const tf_deepflow_params* p, int device_id, tf_handle** out)
{
    tf_deepflow_params dp;
    if (p) dp = *p; else tf_default_deepflow_params(&dp);
    int rc = df_validate(nullptr, dp);
    if (rc) return rc;
    rc = tf_create(nullptr, device_id, out);
    if (rc) return rc;
    (*out)->P.algo = TF_ALGO_DEEPFLOW;
    (*out)->DP = dp;
    return TF_OK;
}

TF_API const char* tf_last_error(tf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

TF_API int tf_create(const tf_params* p, int device_id, tf_handle** out)
{
    if (!out) return fail(nullptr, TF_ERR_INVALID_ARG, "out == NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return fail(nullptr, TF_ERR_NO_DEVICE, "no HIP device visible: libteeflow_hip has no CPU fallback");
    if (device_id < 0 || device_id >= n) return fail(nullptr, TF_ERR_INVALID_ARG, "device_id %d out of range [0,%d)", device_id, n);
    tf_handle* h = new tf_handle();
    if (p) h->P = *p; else tf_default_params(&h->P);
    int rc = validate_params(h, h->P);
    if (rc) { g_create_error = h->err; delete h; return rc; }
    rc = engine_init(h, device_id);
    if (rc) { tf_destroy(h); return rc; }
    *out = h;
    return TF_OK;
}

TF_API void tf_destroy(tf_handle* h)
{
    if (!h) return;
    pool_destroy(h);                                     // the lanes finish what is queued, then go
    for (auto& kv : h->tickets) delete kv.second;
    h->tickets.clear();
    engine_destroy(h);                                   // drains the solve stream, which the tail's work ran on too
    (void)tf_comm_destroy(h);
    for (auto& ev : h->seg_ev) if (ev) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
    if (h->seg_stage) (void)hipHostFree(h->seg_stage);
    for (auto& b : h->pre) if (b.p) (void)hipFree(b.p);
    dev_free(h->an_rad); dev_free(h->an_lon);
    h->held.release();
    h->frames.release();
    (void)spend(h, SPEND_FRAMES);                        // (the address may be the next handle's)
    delete h;
}

// the tf_params field a TF_PARAM_* key names: a double (*d) or an int (*i); false = no such key
static bool param_field(tf_params& p, int key, double** d, int** i)
{
    *d = nullptr; *i = nullptr;
    switch (key) {
        case TF_PARAM_TAU: *d = &p.tau; break;
        case TF_PARAM_LAMBDA: *d = &p.lambda; break;
        case TF_PARAM_THETA: *d = &p.theta; break;
        case TF_PARAM_NSCALES: *i = &p.nscales; break;
        case TF_PARAM_WARPS: *i = &p.warps; break;
        case TF_PARAM_EPSILON: *d = &p.epsilon; break;
        case TF_PARAM_INNER_ITERATIONS: *i = &p.inner_iterations; break;
        case TF_PARAM_OUTER_ITERATIONS: *i = &p.outer_iterations; break;
        case TF_PARAM_SCALE_STEP: *d = &p.scale_step; break;
        case TF_PARAM_GAMMA: *d = &p.gamma; break;
        case TF_PARAM_MEDIAN_FILTERING: *i = &p.median_filtering; break;
        case TF_PARAM_USE_INITIAL_FLOW: *i = &p.use_initial_flow; break;
        default: return false;
    }
    return true;
}

TF_API int tf_set_param(tf_handle* h, int key, double v)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (h->P.algo == TF_ALGO_DEEPFLOW) return fail(h, TF_ERR_UNSUPPORTED, "DeepFlow handles have creation-time parameters only (as cv2's object)");
    tf_params p = h->P;
    double* d; int* i;
    if (!param_field(p, key, &d, &i)) return fail(h, TF_ERR_INVALID_ARG, "unknown parameter key %d", key);
    if (d) *d = v; else *i = key == TF_PARAM_USE_INITIAL_FLOW ? v != 0.0 : (int)v;
    int rc = validate_params(h, p);
    if (rc) return rc;
    h->P = p;
    return TF_OK;
}

TF_API int tf_get_param(tf_handle* h, int key, double* v)
{
    if (!h || !v) return TF_ERR_INVALID_ARG;
    double* d; int* i;
    if (!param_field(h->P, key, &d, &i)) return fail(h, TF_ERR_INVALID_ARG, "unknown parameter key %d", key);
    *v = d ? *d : *i;
    return TF_OK;
}

TF_API int tf_set_stream(tf_handle* h, void* hip_stream, int use_external)
{
    if (!h) return TF_ERR_INVALID_ARG;
    HIPC(h, hipStreamSynchronize(h->stream));
    h->stream = use_external ? (hipStream_t)hip_stream : h->own_stream;
    return TF_OK;
}

TF_API int tf_set_tuning(tf_handle* h, const char* name, int value)
{
    if (!h || !name) return TF_ERR_INVALID_ARG;
    const std::string n(name);
    if (n == "iter_variant") {                      // 0 / 1 / 2 name a form of tvl1_iter (the one-wave-per-strip experiments 4 / 5 / 6 of round 4 are gone: DESIGN.md section 4c)
        if (value < 0 || value > 2) return fail(h, TF_ERR_UNSUPPORTED, "iter_variant must be 0 (64x16 tiles), 1 (row strips) or 2 (row strips, two iterations per launch), got %d", value);
        h->iter_variant = value;
    }
    else if (n == "strip_blocks") h->strip_blocks = value > 0 ? value : 2048;
    else if (n == "min_rows_work") h->min_rows_work = value;
    else if (n == "lane_slots_pct") h->lane_slots_pct = value;
    else if (n == "strip_test_slots") h->strip_test_slots = value < 0 ? 0 : (value > (1 << 20) ? (1 << 20) : value);
    else if (n == "sor_rt") h->sor_rt = value ? 1 : 0;
    else if (n == "sor_rt_shape") h->sor_rt_shape = value;
    else if (n == "sor_plain_div") h->sor_plain_div = value ? 1 : 0;
    else if (n == "max_strip_width") h->max_strip_width = value < 4 ? 4 : (value > 2048 ? 2048 : value);
    else if (n == "lanes") h->lanes = value < 1 ? 1 : (value > 8 ? 8 : value);
    else if (n == "queue_lanes") h->queue_lanes = value;          // -1 = per algorithm (3 DualTVL1, `lanes` DeepFlow), 0 = no lanes: the handle alone
    else if (n == "queue_unit") h->queue_unit = value < 0 ? 0 : value;
    else if (n == "queue_test_fail_unit") h->queue_test_fail_unit = value;
    else if (n == "sor_fuse") h->sor_fuse = value;
    else if (n == "sor_coop") {                       // setting the knob re-arms the form and forgets the back-off: at once, and on a lane when it takes its next job
        h->sor_coop = value;
        if (value) { h->coop.rearm(); ++h->sor_coop_arm; }
    }
    else if (n == "sor_coop_s") h->sor_coop_s = value;
    else if (n == "sor_coop_small") h->sor_coop_small = value ? 1 : 0;
    else if (n == "sor_coop_min_util") h->sor_coop_min_util = value;
    else if (n == "coop_test_mute") h->coop_test_mute = value ? 1 : 0;
    else if (n == "coop_test_occ16") { h->coop_test_occ16 = value; h->coop.occ16 = -1; if (h->coop.flags) h->coop.query_occupancy(*h); }
    else if (n == "coop_test_occ8") { h->coop_test_occ8 = value; h->coop.occ16 = -1; if (h->coop.flags) h->coop.query_occupancy(*h); }
    else if (n == "coop_backoff") { h->coop.backoff = value < 0 ? 0 : value; }        // tests: next abort sits out 2 x this (0: the default 16)
    else if (n == "df_fuse_ds") h->df_fuse_ds = value < 0 ? 0 : (value > 2 ? 2 : value);
    else if (n == "warp_margin") h->warp_margin = value < 0 ? 0 : (value > 40 ? 40 : value);
    else if (n == "overlay_chunk_kib") h->overlay_chunk_kib = value < 0 ? 0 : (value > (512 << 10) ? (512 << 10) : value);   // never above the 512 MiB rule
    else if (n == "area_chunk_kib") h->area_chunk_kib = value < 0 ? 0 : (value > (512 << 10) ? (512 << 10) : value);         // the same
    else if (n == "jpeg_batch_kib") h->jpeg_batch_kib = value < 0 ? 0 : (value > (256 << 10) ? (256 << 10) : value);           // never above the 256 MiB rule
    else if (n == "jpegll_split") {
        if (value < 0 || value > 2) return fail(h, TF_ERR_INVALID_ARG, "jpegll_split must be 0 (automatic), 1 (the serial kernel only) or 2 (the split decode for every interval), got %d", value);
        h->jpegll_split = value;
    }
    else if (n == "jpegll_sync_rounds") h->jpegll_sync_rounds = value < 0 ? 0 : (value > 64 ? 64 : value);
    else return fail(h, TF_ERR_INVALID_ARG, "unknown tuning knob %s", name);
    return TF_OK;
}

#ifdef TF_COOP_TIMING
extern "C" __attribute__((visibility("default"))) int tf_dbg_coop_times(unsigned long long* out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_coop_t), sizeof(unsigned long long) * 4 * 64);
}
#endif
TF_API long long tf_dbg_counter(tf_handle* h, const char* name)
{
    if (!h || !name) return -1;
    const std::string n(name);
    long long v = -1;
    for (int i = 0; i < tf_handle::DT_COUNT; ++i)
        if (n == DEV_TIME_NAMES[i]) return (long long)(h->dev_ms[i] * 1000.0);
    std::vector<CoopCounters> all{h->coop.counters()};            // this handle and what its lanes published at the end of their last unit
    if (h->pool) { std::lock_guard<std::mutex> lk(h->pool->m); all.insert(all.end(), h->pool->coop.begin(), h->pool->coop.end()); }
    if (n == "coop_launches") { v = 0; for (auto& c : all) v += c.launches; }
    else if (n == "coop_aborts") { v = 0; for (auto& c : all) v += c.aborts; }
    else if (n == "coop_disabled") { v = 0; for (auto& c : all) v |= (long long)c.disabled; }
    else if (n == "coop_rearms") { v = 0; for (auto& c : all) v += c.rearms; }
    else if (n == "coop_cooldown") { v = 0; for (auto& c : all) v = v > c.cooldown ? v : c.cooldown; }
    else if (n == "deflate_batches") v = h->deflate_batches;
    else if (n == "queue_jobs") v = h->q_jobs;
    else if (n == "stream_retries") v = h->stream_retries;
    else if (n == "tail_upload_bytes") v = h->tail_upload_bytes;
    else if (n == "frames_upload_bytes") v = h->frames_upload_bytes;
    else if (n == "frames_held_reads") v = h->frames_held_reads;
    else if (n == "ingest_bytes") v = h->ingest_bytes;
    else if (n == "rle_bytes") v = h->rle_bytes;
    else if (n == "jpeg_bytes") v = h->jpeg_bytes;
    else if (n == "jpeg_batches") v = h->jpeg_batches;
    else if (n == "jpegll_bytes") v = h->jpegll_bytes;
    else if (n == "jpegll_batches") v = h->jpegll_batches;
    else if (n == "jpegll_split_intervals") v = h->jpegll_split_intervals;
    else if (n == "jpegll_serial_fallbacks") v = h->jpegll_serial_fallbacks;
    else if (n == "jpegll_sync_rounds") v = h->jpegll_rounds_launched;
    else if (n == "study_download_bytes") v = h->study_download_bytes;
    else if (n == "streams_serialised") v = h->streams_serialised;
    else if (n == "queue_units_done" || n == "queue_units_skipped" || n == "queue_units_failed" || n == "queue_outstanding" || n == "queue_lanes") {
        v = 0;
        if (h->pool) {
            std::lock_guard<std::mutex> lk(h->pool->m);
            v = n == "queue_units_done" ? h->q_units_done : n == "queue_units_skipped" ? h->q_units_skipped : n == "queue_units_failed" ? h->q_units_failed : n == "queue_outstanding" ? h->pool->outstanding : (long long)h->pool->lanes.size();
        }
    }
    else if (n == "chain_steps") {
        if (h->pool) { std::lock_guard<std::mutex> lk(h->pool->m); v = h->chain_steps; }
        else v = h->chain_steps;
    }
    else if (n == "coop_occ16") v = h->coop.occ16;
    else if (n == "coop_occ8") v = h->coop.occ8;
    return v;
}

// the strip rule of k_iter2_rows (pure host arithmetic, no device call): rows per strip and strip count for n active pairs
TF_API void tf_dbg_strip_rule(int n_active, int H, int RY, int slots, int* R, int* S)
{
    int r = 0, sn = 0;
    strip_rule(n_active, H, RY, slots, &r, &sn);
    if (R) *R = r;
    if (S) *S = sn;
}

// per-launch record of the last profiled solve (tvl1_iter launches in issue order): level, warp, first iteration, ms
TF_API int tf_dbg_launch_profile(tf_handle* h, int* level, int* warp, int* it, float* ms, int max_n)
{
    if (!h) return -1;
    int n = 0;
    for (size_t i = 0; i < h->tally.prof_used; ++i) {
        const ProfEv& pe = h->prof_pool[i];
        if (pe.level < 0) continue;                        // warp / median records
        if (n < max_n) {
            if (level) level[n] = pe.level;
            if (warp) warp[n] = pe.warp;
            if (it) it[n] = pe.it;
            if (ms) ms[n] = pe.ms;
        }
        ++n;
    }
    return n;
}

TF_API int tf_set_profile(tf_handle* h, int level)
{
    if (!h) return TF_ERR_INVALID_ARG;
    h->profile = level;
    return TF_OK;
}

TF_API int tf_calc_pair(tf_handle* h, const uint8_t* I0, const uint8_t* I1, int H, int W, float* flow_out, tf_stats* st)
{
    return calc_entry(h, {MODE_PAIRS, I0, I1, 1, H, W, 1.0f, flow_out, W_HOST}, st);
}
TF_API int tf_calc_pairs(tf_handle* h, const uint8_t* I0s, const uint8_t* I1s, int B, int H, int W, float* flow_out, tf_stats* st)
{
    return calc_entry(h, {MODE_PAIRS, I0s, I1s, B, H, W, 1.0f, flow_out, W_HOST}, st);
}
// CV_32FC1 frames (values in [0,1]; cv2 multiplies them by 255 when it builds level 0)
TF_API int tf_calc_pairs_f32(tf_handle* h, const float* I0s, const float* I1s, int B, int H, int W, float* flow_out, tf_stats* st)
{
    return calc_entry(h, {MODE_PAIRS, (const uint8_t*)I0s, (const uint8_t*)I1s, B, H, W, 1.0f, flow_out, W_HOST, true}, st);
}
TF_API int tf_calc_pair_f32(tf_handle* h, const float* I0, const float* I1, int H, int W, float* flow_out, tf_stats* st)
{
    return tf_calc_pairs_f32(h, I0, I1, 1, H, W, flow_out, st);
}
TF_API int tf_calc_seq(tf_handle* h, const uint8_t* frames, int N, int H, int W, float scale, float* flow_out, tf_stats* st)
{
    return calc_entry(h, {MODE_SEQ, frames, nullptr, N - 1, H, W, scale, flow_out, W_HOST}, st);
}
TF_API int tf_calc_pairs_device(tf_handle* h, const uint8_t* dI0s, const uint8_t* dI1s, int B, int H, int W, float scale,
                                float* dflow_out, tf_stats* st)
{
    return calc_entry(h, {MODE_PAIRS, dI0s, dI1s, B, H, W, scale, dflow_out, W_DEV}, st);
}
TF_API int tf_calc_seq_device(tf_handle* h, const uint8_t* dframes, int N, int H, int W, float scale, float* dflow_out, tf_stats* st)
{
    return calc_entry(h, {MODE_SEQ, dframes, nullptr, N - 1, H, W, scale, dflow_out, W_DEV}, st);
}

// ---- OF_model.calc(I0, I1, flow) under useInitialFlow: the pairs calls with an initial flow per pair.  The flag decides, as in cv2:
// off, `init` is not looked at; on, check_call refuses a call without one ----------------------------------------------------------------
static int calc_init_entry(tf_handle* h, Call c, const float* init, tf_stats* st)
{
    if (h && h->P.algo == TF_ALGO_TVL1 && h->P.use_initial_flow) c.init = init;
    return calc_entry(h, c, st);
}
TF_API int tf_calc_pairs_init(tf_handle* h, const void* I0s, const void* I1s, int frames_f32, const float* init_flows, int B, int H, int W,
                              float* flow_out, tf_stats* st)
{
    return calc_init_entry(h, {MODE_PAIRS, (const uint8_t*)I0s, (const uint8_t*)I1s, B, H, W, 1.0f, flow_out, W_HOST, frames_f32 != 0}, init_flows, st);
}
TF_API int tf_calc_pairs_init_device(tf_handle* h, const uint8_t* dI0s, const uint8_t* dI1s, const float* d_init, int B, int H, int W, float scale,
                                     float* dflow_out, tf_stats* st)
{
    return calc_init_entry(h, {MODE_PAIRS, dI0s, dI1s, B, H, W, scale, dflow_out, W_DEV}, d_init, st);
}

// ---- a chained sequence (the video idiom `flow = calc(frames[k], frames[k+1], flow)`): armed for the handle's next solve call --------
// (Call::chain; spend() in teeflow_engine.hip.h says which calls take the flag)
TF_API int tf_chain_next(tf_handle* h, int on)
{
    if (!h) return TF_ERR_INVALID_ARG;
    h->armed.chain = false;
    if (!on) return TF_OK;
    if (h->P.algo == TF_ALGO_DEEPFLOW) return fail(h, TF_ERR_UNSUPPORTED, "a chained sequence is DualTVL1's (useInitialFlow): DeepFlow takes no initial flow");
    if (h->P.variant == TF_VARIANT_CUDA) return fail(h, TF_ERR_UNSUPPORTED, "a chained sequence needs useInitialFlow, which TF_VARIANT_CUDA does not implement");
    if (!h->P.use_initial_flow)
        return fail(h, TF_ERR_UNSUPPORTED, "useInitialFlow is clear: cv2 then ignores a passed flow, so a chain would be the plain solve at the cost of "
                                            "N-1 serial steps; set TF_PARAM_USE_INITIAL_FLOW first, or make the plain call");
    h->armed.chain = true;
    return TF_OK;
}

// ---- asynchronous forms: the job is queued on the handle's lanes and the call returns; tf_wait collects it ----------------------
TF_API int tf_submit_pairs_device(tf_handle* h, const uint8_t* dI0s, const uint8_t* dI1s, int B, int H, int W, float scale, float* dflow_out, int* ticket)
{
    return submit_entry(h, {MODE_PAIRS, dI0s, dI1s, B, H, W, scale, dflow_out, W_DEV}, ticket);
}
TF_API int tf_submit_seq_device(tf_handle* h, const uint8_t* dframes, int N, int H, int W, float scale, float* dflow_out, int* ticket)
{
    return submit_entry(h, {MODE_SEQ, dframes, nullptr, N - 1, H, W, scale, dflow_out, W_DEV}, ticket);
}
TF_API int tf_submit_pairs(tf_handle* h, const uint8_t* I0s, const uint8_t* I1s, int B, int H, int W, float* flow_out, int* ticket)
{
    return submit_entry(h, {MODE_PAIRS, I0s, I1s, B, H, W, 1.0f, flow_out, W_HOST}, ticket);
}
TF_API int tf_submit_seq(tf_handle* h, const uint8_t* frames, int N, int H, int W, float scale, float* flow_out, int* ticket)
{
    return submit_entry(h, {MODE_SEQ, frames, nullptr, N - 1, H, W, scale, flow_out, W_HOST}, ticket);
}

TF_API int tf_wait(tf_handle* h, int ticket, tf_stats* st)
{
    if (!h) return TF_ERR_INVALID_ARG;
    if (ticket < 0) {                                        // every job not yet waited for, oldest first; the first failure is returned
        int rc_all = TF_OK; std::string err_all;
        while (!h->tickets.empty()) {
            const int rc = tf_wait(h, h->tickets.begin()->first, st);
            if (rc && !rc_all) { rc_all = rc; err_all = h->err; }
        }
        if (rc_all) h->err = err_all;
        return rc_all;
    }
    auto f = h->tickets.find(ticket);
    if (f == h->tickets.end()) return fail(h, TF_ERR_INVALID_ARG, "unknown ticket %d (already waited for?)", ticket);
    QJob* j = f->second;
    h->tickets.erase(f);
    const int rc = queue_finish(h, j, st);
    delete j;
    return rc;
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

// ---- the study tail: everything around the solver, from frame conditioning to WASE; host code, a header per topic in the order they build on each other ----
#include "teeflow_scratch.hip.h"          // the handle's grow-only scratch, chunking, Src: what every tail call shares
#include "teeflow_streams_host.hip.h"     // a batch of byte streams: check, upload, verdict (inflate's and RLE's)
#include "teeflow_frames_host.hip.h"      // a call's frames (tf_frames_next), conditioning, echo, saliency, the held frames
#include "teeflow_jpeg_host.hip.h"        // frames held from JPEG Baseline pixel data
#include "teeflow_jpegll_host.hip.h"      // frames held from JPEG Lossless pixel data (SOF3, predictor 1)
#include "teeflow_masks_host.hip.h"       // labelling: clean masks, Otsu, AV centroids, first-region areas
#include "teeflow_segmentor_host.hip.h"
#include "teeflow_analysis_host.hip.h"    // rad/long and polar projections, histogram, select
#include "teeflow_overlay_host.hip.h"
#include "teeflow_wase_host.hip.h"
#include "teeflow_held.hip.h"             // a study held on the device and the tail calls that read it there
#include "teeflow_study_host.hip.h"       // the study calls
#include "teeflow_chains_host.hip.h"      // several chains in lock-step
#include "teeflow_inflate_host.hip.h"     // tf_inflate, and a study held from the gzip chunks of its file
#include "teeflow_deflate_host.hip.h"

TF_API int tf_get_iters(tf_handle* h, int* out, size_t capacity_ints, size_t* written)
{
    if (!h || !out) return TF_ERR_INVALID_ARG;
    const size_t n = h->last_iters.size() < capacity_ints ? h->last_iters.size() : capacity_ints;
    memcpy(out, h->last_iters.data(), n * sizeof(int));
    if (written) *written = n;
    return TF_OK;
}
#include "teeflow_comm.hip.h"
#include "teeflow_dbg.hip.h"
