// teeflow_engine.hip.h -- what solves a sub-batch (Engine) and what a caller holds (tf_handle : Engine); included by teeflow.hip
// after the kernel headers (one translation unit).  A queue lane is an Engine with a host thread (teeflow_queue.hip.h); the handle
// adds everything around the solver: the study tail's scratch, the analysis session, RCCL, the lane queue and its tickets.
// The records an engine is made of are declared here; their functions are next to their solver (teeflow_*_host.hip.h).
#include <rccl/rccl.h>      // types and prototypes only: librccl is loaded with dlopen when a communicator is first asked for
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <deque>
#include <string>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <map>
#include <vector>

#define TF_API extern "C" __attribute__((visibility("default")))

namespace {
constexpr int MAXLEV = 64;
// DeepFlow pyramid depth: at most 200 downscales (201 levels), upstream OpticalFlowDeepFlow's `maxLayers` (200) as recalled, not pinned
// against OpenCV.  oracle/deepflow_oracle.c stops at the same depth (DFO_MAX_LEVELS).  Default x0.95 pyramids never reach it: 60 levels
// at 512^2, 87 at 2048^2; a size rule with a fixed point above min_size (64^2, min_size 5: 10 x 10 for ever) does.
constexpr int DF_MAXLEV = 201;
constexpr int SLOT_RING = 1024;       // host-mapped words the tvl1_iter launches publish their active-pair count to
constexpr int DEFAULT_LAG = 1;        // the host enqueues at most this many launches beyond the last answer it has read
constexpr int DEFAULT_MAX_BATCH = 128;

thread_local std::string g_create_error;

struct ProfEv { hipEvent_t a, b; int level = 0, warp = 0, it = 0; float ms = 0.f; double work = 0.0; };
}  // namespace

// Implementation knobs (tf_set_tuning; results never depend on them).  One struct, so that a lane gets its engine's settings with ONE
// assignment (a knob missed in a field-by-field copy would silently make the lanes differ).
namespace { struct Engine; }
struct LanePool;
struct QJob;
struct CoopCounters { long long launches = 0; int aborts = 0, rearms = 0, cooldown = 0; bool disabled = false; };
struct TfKnobs {
    int iter_variant = 2;        // 0 = 64x16 tiles (k_iter), 1 = full-width row strips (k_iter_rows), 2 = row strips with TWO
                                 // iterations per launch (k_iter2_rows); 1 and 2 need W <= max_strip_width (2048) and enough rows*pairs
    int max_strip_width = 2048;  // widest level the full-width strip kernels take (one quad per thread: 2048 px = 512-thread blocks).
                                 // 8 pairs: 1080x1920 57.7 vs 32.6 pairs/s with the tile kernel, 768x1100 184 vs 131, 720x1280 137 vs 148
    int sor_rt = 1;              // DeepFlow SOR: 1 = register-tile kernel k_df_sor_rt (teeflow_sor_rt.hip.h), 0 = one colour per launch (k_df_sor)
    int sor_plain_div = 0;       // tests: k_df_sor_rt takes its plain-IEEE-division path (what a block with out-of-range diagonals does)
    int sor_rt_shape = 3;        // k_df_sor_rt: 1 = 16 bands x 4 rows (1024 threads), 2 = 8 bands x 4 rows (128 x 32
                                 // regions, 512 threads), 3 = 1 or 2 per launch (launch_sor_rt)
    int df_fuse_ds = 2;          // DeepFlow: data term + smoothness contributions in one kernel (non-zero: k_df_data_smooth4, four pixels per thread,
                                 // 16-byte loads; 0: k_df_data then k_df_smooth, the plain form it is tested against)
    int sor_coop = 1;            // DeepFlow: all sweeps of a fixed-point iteration in one launch of co-resident regions (k_df_sor_rt_coop) where a
                                 // level needs more than one region and its regions fit the CUs this engine may use; 0 = always the tiled form,
                                 // 2 = 128 x 64 regions whatever the batch size and however full the launches (tests), 3 = the small-batch form
                                 // (128 x 32 regions) whenever the batch is small, sor_coop_small or not (tests)
    int sor_coop_min_util = 85;  // co-resident launches must be at least this full (per cent) RELATIVE to the tiled form's rounds, else the level runs
                                 // tiled (600x800 studies: 324 pairs/s always co-resident, 357 tiled, 359 with the rule)
    int sor_coop_small = 1;      // few pairs: co-resident 128 x 32 regions (0: the tiled form, as before)
    int sor_coop_s = 5;          // sweeps between two exchanges of (du, dv) in that kernel (the halo is 2 x this)
    int sor_fuse = 5;            // DeepFlow: complete red-black SOR sweeps per launch of k_df_sor_rt (0 = one colour per launch, in place).
                                 // 64 pairs @512^2: 466 / 534 / 562 / 548 / 567 pairs/s for 3 / 4 / 5 / 6 / 7; 5 divides the 25 sweeps evenly
    int warp_margin = 8;         // > 0: k_warp_lds<M> stages the I1 tile + margin in LDS (0: k_warp, 36 global gathers per pixel).  k_warp is
                                 // bound by the texture path (~7-10 cycles per scattered dword load and wave); from LDS the same taps cost
                                 // ~2.  128 pairs @512^2, warp stage per step: 5.0 ms gathers, 3.35 / 3.5 / 3.55 / 3.8 ms for M = 4 / 8 / 12 /
                                 // 16 (+3.4 % pairs/s).  A pixel displaced by more than M falls back to the gathers, so M only moves time.
    int min_rows_work = 8192;    // rows*pairs of a level below which the tile kernels are used (measured at 512^2 with k_iter2_tile: 16 pairs
                                 // 12.5 ms on tiles vs 13.9 ms on strips, 24 pairs 17.1 vs 17.3, 64 pairs 34.1 vs 29.5)
    int strip_blocks = 2048;     // target number of strip blocks per launch of a sub-batch above 1024 pairs (sets rows per strip; smaller
                                 // sub-batches have their strips sized on the device)
    int lane_slots_pct = 67;     // queue units (not a split call's): per cent of the resident blocks a lane sizes their strips for.  Three lanes share the GPU, so a
                                 // lane that cuts its level into one round of ALL resident blocks pays the 3 halo + 2 RY fill rows of short strips for
                                 // parallelism the other lanes already provide (queue form, 384 pairs per call: 100 % 2728-2745, 67 % 2769-2772,
                                 // 50 % 2767-2769, 33 % 2706-2711 pairs/s on one box)
    int strip_test_slots = 0;    // tests: >= 1 = pretend the resident-block count k_iter2_rows sizes its strips for is this (after lane_slots_pct's
                                 // scaling), so that a test chooses the strip layout (R, S); 0 = the occupancy query's answer
    int coop_test_occ16 = -1, coop_test_occ8 = -1;   // tests: pretend the occupancy query answered this
    int coop_test_mute = 0;      // tests: block 0 of every co-resident launch never raises its flag -> its neighbours give up -> the call is repeated tiled
    int profile = 0;
    int overlay_chunk_kib = 0;   // tests: tf_radlong_overlay's and tf_magnitude_overlay's chunk of frames holds at most this many KiB instead of MASK_CHUNK_BYTES (0: that)
    int area_chunk_kib = 0;      // tests: tf_first_region_areas' chunk of frames likewise
    unsigned sor_coop_arm = 0;   // bumped by tf_set_tuning("sor_coop", non-zero): a lane that sees a new value in a job's knobs re-arms the form
};

namespace {
// ---- DualTVL1: the buffers of one geometry (ensure / release, teeflow_tvl1_host.hip.h) and what its launches are sized with ----
struct Tvl1State {
    // geometry the buffers are allocated for
    int H = 0, W = 0, cap = 0, nlev = 0;
    double scale_step = 0; int nscales = 0, variant = 0;
    Geom lv[MAXLEV];
    float* pyr[MAXLEV] = {};
    float* gxl[MAXLEV] = {}; float* gyl[MAXLEV] = {};   // TF_VARIANT_CUDA: centred gradient of every frame, per level
    float *cwx = nullptr, *cwy = nullptr, *crho = nullptr;
    StateBufs sb = {};
    PairCtl* ctl = nullptr;
    u64* errs = nullptr; int errstride = 0;
    int* iters_dev = nullptr; size_t iters_cap = 0;
    const void** chain_src = nullptr; size_t chain_src_cap = 0;     // chains in lock-step: a sub-batch's frame sources (k_chain_gather), grown on demand
    // made with the engine, whatever the geometry (engine_init)
    volatile int* slots_host = nullptr; int* slots_dev = nullptr;   // fine-grained pinned ring (SLOT_RING ints)
    unsigned launch_seq = 0;
    float* tab = nullptr;
    std::map<size_t, int> slots_cache;      // resident k_iter2_rows blocks on the device, by (LDS bytes, waves per block)
    int ensure(Engine* e, int H, int W, int B);
    void release();
};

// ---- DeepFlow (algo == TF_ALGO_DEEPFLOW): the buffers of one geometry (ensure / release, teeflow_deepflow_host.hip.h) ----
struct DfState {
    int nlev = 0, H = 0, W = 0, cap = 0;
    Geom lv[DF_MAXLEV];
    float* pyr_base = nullptr; size_t pyr_off[DF_MAXLEV] = {};   // one allocation: level l of frame f at pyr_base + off[l] + f*plane_l
    float* tmp = nullptr;                                         // unblurred level-0 frames
    float* planes = nullptr;                                      // 23 state planes x cap pairs (df_carve)
    DfBufs bufs = {};
    int ensure(Engine* e, int H, int W, int B);
    void release();
};

// ---- the co-resident SOR form's state: what an engine may fill, its back-off after an abort, its meeting place on the device ----
struct Coop {
    int share = 0;               // CUs (= resident 1024-thread blocks) this engine may fill with such a launch; set per call (start_call, lane_worker)
    bool disabled = false;       // a launch of this engine gave up waiting (foreign work on the GPU): tiled form until the back-off has run out
    int backoff = 0;             // tiled solves (sub-batches) to sit out before the co-resident form is tried again; doubles with every abort
    int cooldown = 0;            // ... of which this many are left
    int rearms = 0;              // times the form was re-armed after a back-off
    int occ16 = -1, occ8 = -1;   // resident blocks per CU of k_df_sor_rt_coop<4,16> / <4,8> (hipOccupancyMaxActiveBlocksPerMultiprocessor), -1 = not asked yet
    int asked16 = -2, asked8 = -2;   // the test overrides (knobs) that answer was made with
    bool used = false;           // this call launched k_df_sor_rt_coop
    int aborts = 0;
    long long launches = 0;
    unsigned epoch = 0;          // flag value base of the next launch
    unsigned* flags = nullptr;   // one 128-byte line per resident block + the abort word behind them
    int flag_lines = 0;
    void tick();
    void query_occupancy(const TfKnobs& k);
    int ensure(Engine* e);
    int aborted(Engine* e, bool* aborted);
    void rearm() { disabled = false; backoff = cooldown = 0; }      // the form is tried again at once and the back-off is forgotten
    CoopCounters counters() const { return {launches, aborts, rearms, cooldown, disabled}; }
    void release();
};

struct Engine : TfKnobs {
    tf_params P;
    tf_deepflow_params DP = {};
    int dev = 0;
    int num_cus = 256;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
    // staging for the host-pointer API
    hipStream_t copy_stream = nullptr;           // D2H of finished sub-batches overlaps the next solve (pinned destinations)
    hipEvent_t cev[4] = {nullptr, nullptr, nullptr, nullptr};   // solve done [2], copy done [2]
    uint8_t* st_u8 = nullptr; size_t st_u8_bytes = 0;
    uint8_t* st_flow = nullptr; size_t st_flow_bytes = 0;     // flow staging, in the call's output element type
    uint8_t* st_init = nullptr; size_t st_init_bytes = 0;     // a sub-batch's initial flows (useInitialFlow, host callers), float32
    hipEvent_t ev[5] = {};
    // profiling of tvl1_iter launches
    std::deque<ProfEv> prof_pool;                            // deque: records keep their address while the pool grows
    // per-call tallies (calc_common starts them at zero; the repeat of an aborted sub-batch restores them)
    struct Tally {
        unsigned long long iter_launches = 0;
        double df_sor_bytes = 0;     // DeepFlow: algorithmic bytes of the SOR launches of the current call (40 B per pixel-sweep)
        double df_sor_px = 0;        // DeepFlow: pixels x pairs summed over the SOR launches (a launch's compulsory traffic is 40 B per pixel: 8 planes in, 2 out)
        size_t prof_used = 0;        // records of prof_pool in use
        long long chain_steps = 0;   // DualTVL1: pairs solved as steps of a chained sequence
    } tally;
    int slots_pct = 100;         // per cent of the resident blocks this engine sizes its strips for (a lane: what its current job says)
    Tvl1State tv;
    DfState df;
    Coop coop;
};
}  // namespace

struct tf_handle : Engine {
    std::vector<int> last_iters;                             // tf_get_iters: the last call's iteration counts
    // ---- study tail (conditioning, saliency, masks, centroids, projections, statistics, overlay, WASE): every piece of its device
    // scratch is one of these grow-only slots, freed with the handle (teeflow_scratch.hip.h) ----
    struct GrowBuf { void* p = nullptr; size_t cap = 0; };
    enum { PRE_SRC, PRE_G0, PRE_G1, PRE_ION, PRE_IOFF, PRE_P, PRE_I, PRE_MON, PRE_MOFF, PRE_MX, PRE_OUT,
           PRE_LB_PAR, PRE_LB_AUX, PRE_LB_LR,                                     // the labelling's parents, per-root flags / sizes / areas and
                                                                                  //   tile-local roots: tf_clean_masks, tf_otsu_masks, tf_av_centroids, tf_first_region_areas
           PRE_MK_CLS, PRE_MK_OUT, PRE_MK_META,                                   // tf_clean_masks
           PRE_OT_RGB, PRE_OT_CLEAN, PRE_OT_OUT, PRE_OT_META,                     // tf_otsu_masks
           PRE_CT_MASK, PRE_CT_SUM, PRE_CT_OUT,                                   // tf_av_centroids; tf_first_region_areas (mask, out)
           PRE_AN_FLOW, PRE_AN_MASK, PRE_AN_META,                                 // the projections' uploads (also tf_wase_compensate's) and
           PRE_PO_META, PRE_PO_OUT,                                               //   meta words: rad/long's, polar's
           PRE_AN_HIST, PRE_AN_SEL,                                               // tf_radlong_hist, tf_radlong_select
           PRE_OV_IDX, PRE_OV_ECHO, PRE_OV_OUT, PRE_OV_META,                      // tf_radlong_overlay
           PRE_MO_IDX, PRE_MO_ECHO, PRE_MO_OUT, PRE_MO_META,                      // tf_magnitude_overlay
           PRE_WA_VALS, PRE_WA_CNT, PRE_WA_OFF, PRE_WA_SUM, PRE_WA_BG,            // WASE: compacted products, block counts / offsets, piece
                                                                                  //   sums, per-flow backgrounds
           PRE_WS_FLOW, PRE_WS_OUT,                                               // a WASE study call (tf_calc_seq_*_wase): the solver's resident
                                                                                  //   float32 flows, the compensated output in the call's type
           PRE_SG_IN, PRE_SG_IDX, PRE_SG_MAP,                                     // tf_segmentor_input (tables, LUT, frames), tf_segmentor_classmap
           PRE_ECHO,                                                              // the study's float16 `echo` (tf_echo_frames, the *_f16 calls)
           PRE_CH_GRAY,                                                           // tf_calc_chains_rgb: the conditioned frames of all its studies
           PRE_INF_BLOB, PRE_INF_TABLE, PRE_INF_OUT,                              // tf_inflate, tf_hold_*_chunks: compressed bytes, per-stream table, inflated chunks
           PRE_DF_WORK, PRE_DF_TABLE, PRE_DF_BLOB, PRE_DF_SRC,                    // tf_deflate, tf_deflate_array, tf_held_deflate: a batch's scratch, per-chunk table,
                                                                                  //   the streams end to end, an uploaded array
           PRE_FR_SRC,                                                            // tf_hold_frames: the source bytes as the file stores them, before k_ingest
           PRE_RLE_BLOB, PRE_RLE_TABLE, PRE_RLE_PLANES, PRE_RLE_OUT,              // tf_rle_decode, tf_hold_frames_rle: compressed bytes, per-frame table, the decoded
                                                                                  //   sample planes; tf_rle_decode's interleaved frames
           PRE_JPEG_BLOB, PRE_JPEG_TABLE, PRE_JPEG_RST, PRE_JPEG_COEF, PRE_JPEG_PLANES, PRE_JPEG_OUT, PRE_JPEG_SYNC,   // tf_jpeg_decode, tf_hold_frames_jpeg: compressed bytes, per-frame
                                                                                  //   table, RSTn positions, a batch's coefficients and component planes; the frames.
                                                                                  //   tf_jpegll_decode, tf_hold_frames_jpegll use the same slots (COEF: a batch's differences;
                                                                                  //   SYNC: the split entropy decode's per-piece and per-interval scratch of a batch)
           PRE_COUNT };
    GrowBuf pre[PRE_COUNT];
    // Device time of the tail's kernels in ms, read from the handle's event pairs (dev_time, below); tf_dbg_counter reports slot i in
    // microseconds under DEV_TIME_NAMES[i].  Of the last call: the saliency kernels, a WASE study call's reduction and output kernels,
    // k_ingest (tf_hold_frames, tf_hold_frames_rle), k_rle_decode (tf_rle_decode, tf_hold_frames_rle).  Since the handle was made:
    // k_inflate, k_unchunk, deflate's links + search, its emit + offsets + pack, and k_chunk.  Of the last tf_jpeg_decode /
    // tf_hold_frames_jpeg: the four k_jpeg_* kernels.  Of the last tf_jpegll_decode / tf_hold_frames_jpegll: k_jpeg_marks + k_jpegll_entropy,
    // and k_jpegll_col + k_jpegll_rows.
    enum { DT_SALIENCY, DT_WASE, DT_INGEST, DT_RLE, DT_INFLATE, DT_UNCHUNK, DT_DEFLATE_MATCH, DT_DEFLATE_EMIT, DT_CHUNK,
           DT_JPEG_MARKS, DT_JPEG_ENTROPY, DT_JPEG_IDCT, DT_JPEG_FINISH, DT_JPEGLL_ENTROPY, DT_JPEGLL_RESTORE, DT_COUNT };
    double dev_ms[DT_COUNT] = {};
    long long deflate_batches = 0;                                           // passes of deflate_run's batch loop since the handle was made
    // tf_segmentor_input does not wait for its work: pinned staging its upload reads from, and the events that say when the staging
    // ([0]: upload done) and the device scratch ([1]: kernel done) of the last call may be written again
    void* seg_stage = nullptr; size_t seg_stage_cap = 0; hipEvent_t seg_ev[2] = {};
    // ---- analysis session (row f1): lives until the next projection or the handle's end, whatever the solver allocates meanwhile ----
    double* an_rad = nullptr; double* an_lon = nullptr; int anN = 0, anH = 0, anW = 0;
    size_t an_cap = 0;           // doubles an_rad and an_lon each hold (grow_an_planes grows them, never shrinks)
    bool an_polar = false;       // the resident planes are tf_polar_project_param's magnitude / angle, not rad / long
    bool an_finite = false;      // ... and hold no NaN or inf (their min / max are finite)
    // ---- the held study (teeflow_held.hip.h): a study file's payload in device buffers of its own, which no other call writes; lives
    // until the next tf_hold_study / armed study call, tf_release_study or the handle's end ----
    struct Held {
        uint16_t* flow = nullptr; uint16_t* echo = nullptr;  // float16 [N][H][W][2]; float16 [n_echo][H][W] or null
        int N = 0, H = 0, W = 0, n_echo = 0;                 // N == 0: no study is held
        long long gen = 0;                                   // grows with every replacement and release
        struct Mask { uint8_t* p = nullptr; int n_frames = 0, C = 0; } mask[TF_HELD_SLOTS];   // uint8 [n_frames][H][W][C]
        // frees everything (the caller has drained the streams that read it); the generation moves on if a study was held
        void release()
        {
            if (N) ++gen;
            (void)hipFree(flow); (void)hipFree(echo);
            for (auto& m : mask) { (void)hipFree(m.p); m = Mask(); }
            flow = echo = nullptr; N = H = W = n_echo = 0;
        }
    } held;
    // ---- the held frames (teeflow_frames_host.hip.h): a study's uint8 RGB [N][H][W][3] in a device buffer of the handle's own, ingested once
    // (k_ingest) and read in place by every frames-taking call armed with tf_frames_next; separate from the held study ----
    struct Frames {
        uint8_t* rgb = nullptr; size_t cap = 0;              // the buffer only grows; it goes with tf_release_frames or the handle
        int N = 0, H = 0, W = 0;                             // N == 0: no frames are held
        long long gen = 0;                                   // grows with every replacement and release
        void drop() { if (N) ++gen; N = H = W = 0; }         // nothing is held any more (the buffer stays)
        void release() { drop(); (void)hipFree(rgb); rgb = nullptr; cap = 0; }   // (the caller has drained the streams that read it)
    } frames;
    long long frames_upload_bytes = 0;   // bytes of frames that tf_hold_frames and the frames-taking calls have copied host -> device
    long long frames_held_reads = 0;     // frames-taking calls that read the held frames in place
    long long ingest_bytes = 0;          // the last tf_hold_frames: the bytes k_ingest read and wrote
    long long rle_bytes = 0;             // the last tf_rle_decode / tf_hold_frames_rle: compressed bytes read + plane bytes written
    long long jpeg_bytes = 0;            // the last tf_jpeg_decode / tf_hold_frames_jpeg: compressed bytes read + sample bytes written
    long long jpeg_batches = 0;          // the batches of frames the JPEG decoder has worked through since the handle was made
    long long jpegll_bytes = 0;          // the last tf_jpegll_decode / tf_hold_frames_jpegll: compressed bytes read + sample bytes written
    long long jpegll_batches = 0;        // the batches of frames the JPEG Lossless decoder has worked through since the handle was made
    long long jpegll_split_intervals = 0;   // restart intervals sent down the split entropy decode since the handle was made
    long long jpegll_serial_fallbacks = 0;  // ... of which did not converge within the rounds and were decoded serially
    long long jpegll_rounds_launched = 0;   // the last tf_jpegll_decode / tf_hold_frames_jpegll: synchronisation rounds launched, all batches
    int jpegll_split = 0;                // tuning: 0 the split decode where the host's rule picks it, 1 the serial kernel only, 2 the split decode for every interval
    int jpegll_sync_rounds = 8;          // tuning: synchronisation rounds a batch launches (0: speculation only)
    int jpeg_batch_kib = 0;              // tuning: the coefficient scratch of a batch in KiB (0: 256 MiB), the lossless decoder's difference scratch too; the tests cut a call into batches with it
    // ---- the one-shot flags of the handle's next call, taken with spend(), below: tf_chain_next (a sequence is solved as a chain),
    // tf_hold_next (a study call leaves its payload held), tf_frames_next (the call reads held frames [first, first + count)).
    // `armed` holds the first two; tf_frames_next's part of the record is kept beside the handles (g_frames_next says why) ----
    struct Armed { bool chain = false, hold = false, frames = false; int first = 0, count = 0; } armed;
    long long chain_steps = 0;   // pairs this handle and its lanes have solved as chain steps ("chain_steps" counter; the pool's lock where there is a pool)
    long long study_download_bytes = 0;   // bytes of flow and echo the synchronous study calls have copied device -> host
    long long tail_upload_bytes = 0;   // bytes of flow, mask and echo the tail calls (and tf_hold_*) have copied host -> device
    // RCCL: one communicator rank per handle, its own stream, a small ring of completion events
    ncclComm_t comm = nullptr; int comm_rank = 0, comm_size = 0;
    hipStream_t comm_stream = nullptr; hipEvent_t comm_ev[8] = {}; hipEvent_t comm_ready = nullptr; unsigned comm_tickets = 0;
    // ---- engine lanes that pull whole sub-batches from a queue (calc_entry, tf_submit_*) ----
    int lanes = 2;               // an idle call of one sub-batch, >= 32 pairs, is split in this many contiguous units solved side by side on the
                                 // queue lanes: while one runs the thin tail of a stage, the other fills the GPU.  Measured at 128 pairs
                                 // @512^2: 1 lane 2180, 2 lanes 2470, 3 lanes 2415, 4 lanes 2165 pairs/s (DeepFlow 377 vs 309)
    int queue_lanes = -1;        // -1 = per algorithm (3 DualTVL1, `lanes` DeepFlow); 0 = never: the handle solves every call alone, sub-batch after sub-batch
    int queue_unit = 0;          // pairs per queue unit (0 = equal units of at most max_batch pairs, a multiple of the lane count of them)
    int queue_test_fail_unit = -1;   // tests: the lane that takes this unit of the next queued job reports a failure instead of solving it
    LanePool* pool = nullptr;
    long long q_jobs = 0, q_units_done = 0, q_units_skipped = 0, q_units_failed = 0;
    std::map<int, QJob*> tickets; int next_ticket = 1;      // tf_submit_* jobs not yet waited for
    int stream_retries = 0;      // streams made and dropped while looking for lane streams that run beside each other (pool_ensure)
    int streams_serialised = 0;  // bit 0: a lane had to keep a solve stream that shares a hardware queue with a sibling's; bit 1: a lane's copy stream shares one with a solve stream
};

TF_API int tf_create(const tf_params* p, int device_id, tf_handle** out);
TF_API int tf_create_deepflow(const tf_deepflow_params* p, int device_id, tf_handle** out);
TF_API const char* tf_last_error(tf_handle* h);
TF_API int tf_comm_destroy(tf_handle* h);

namespace {
// What of the flags `which` names was armed on h, and exactly those cleared: nothing on a null handle.  A call spends its family's
// flags once, at its start, whatever becomes of it (tests/test_gpu_armed_matrix.py pins the table; a handle is not re-entrant):
//   family                                                                spends               an armed flag it spends is
//   pairs and sequence calls (calc_entry, submit_entry)                   chain                honoured by a sequence call, refused by a pairs call (check_call)
//   study calls (study_call), before any argument check                   chain, hold, frames  honoured, or refused with the call
//   lock-step calls (check_chains), before any argument check             chain, hold, frames  refused, frames first, then hold; the chain flag changes nothing
//   frames-taking tail calls (call_frames), before their argument checks  frames               honoured (the handle itself is read only once the checks have passed)
//   everything else: tf_held_*, tf_hold_*, tf_release_*, tf_set_*, ...    nothing              (a refused tf_chain_next(h, 1) has disarmed the chain itself)
constexpr tf_handle::Armed SPEND_CHAIN{true, false, false}, SPEND_FRAMES{false, false, true}, SPEND_ALL{true, true, true};

// tf_frames_next's flag and range, by handle.  They are kept beside the handles, not in them, because the frames-taking tail calls
// spend the flag before their argument checks and must not read the handle before those have passed: a call refused for a null
// pointer or a bad size touches nothing of it (the CPU tests hand such calls a stand-in for the handle that cannot be read), and
// whether a null frame pointer is a mistake or the armed call's is part of that check.  spend(h, SPEND_FRAMES) never reads *h.
std::mutex g_frames_next_m;
std::map<const tf_handle*, tf_handle::Armed> g_frames_next;

tf_handle::Armed spend(tf_handle* h, const tf_handle::Armed& which)
{
    tf_handle::Armed got;
    if (!h) return got;
    if (which.frames) {
        std::lock_guard<std::mutex> lk(g_frames_next_m);
        const auto f = g_frames_next.find(h);
        if (f != g_frames_next.end()) { got = f->second; g_frames_next.erase(f); }
    }
    if (which.chain) { got.chain = h->armed.chain; h->armed.chain = false; }
    if (which.hold) { got.hold = h->armed.hold; h->armed.hold = false; }
    return got;
}

int fail(Engine* e, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (e) e->err = buf; else g_create_error = buf;
    return code;
}

#define HIPC(h, call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(h, e_ == hipErrorOutOfMemory ? TF_ERR_NOMEM : TF_ERR_HIP, "%s failed: %s (%s:%d)", #call, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                \
    } while (0)

constexpr const char* DEV_TIME_NAMES[tf_handle::DT_COUNT] = {"saliency_kernel_us", "wase_study_kernel_us", "ingest_kernel_us", "rle_kernel_us", "inflate_kernel_us",
                                                             "unchunk_kernel_us", "deflate_match_us", "deflate_emit_us", "chunk_kernel_us",
                                                             "jpeg_marks_us", "jpeg_entropy_us", "jpeg_idct_us", "jpeg_finish_us",
                                                             "jpegll_entropy_us", "jpegll_restore_us"};

// The device time from ev[a] to ev[b] of the handle, both recorded on a stream that has been waited for, into dev_ms[slot]: added to
// it, or put in its place.  A read-back that fails leaves the slot and is the caller's to judge: HIPC(h, dev_time(...)) fails the
// call (saliency, a WASE study, a hold's ingest), (void)dev_time(...) drops it where a counter alone depends on it (inflate, deflate, RLE).
inline hipError_t dev_time(tf_handle* h, int a, int b, int slot, bool add)
{
    float t = 0;
    const hipError_t e = hipEventElapsedTime(&t, h->ev[a], h->ev[b]);
    if (e == hipSuccess) h->dev_ms[slot] = (add ? h->dev_ms[slot] : 0.0) + t;
    else (void)hipGetLastError();
    return e;
}

inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int cv_round_d(double v) { return (int)lrint(v); }   // saturate_cast<int>(double): nearest-even

Geom make_geom(int w, int h)
{
    Geom g; g.w = w; g.h = h; g.pitch = round_up(w, 32); g.plane = (long long)g.pitch * h; g.splane = g.plane;
    return g;
}

template <class T> void dev_free(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }
// the staging is sized by the solver's capacity: a solver that re-allocates gives it back, and ensure_staging regrows it
void release_staging(Engine* e)
{
    dev_free(e->st_u8); dev_free(e->st_flow); dev_free(e->st_init);
    e->st_u8_bytes = e->st_flow_bytes = e->st_init_bytes = 0;
}

int grow_staging(Engine* h, uint8_t*& p, size_t& have, size_t want)
{
    if (have >= want) return TF_OK;
    dev_free(p); have = 0;
    HIPC(h, hipMalloc(&p, want)); have = want;
    return TF_OK;
}
int ensure_staging(Engine* h, size_t u8_bytes, size_t flow_bytes, size_t init_bytes = 0)
{
    int rc = grow_staging(h, h->st_u8, h->st_u8_bytes, u8_bytes);
    if (!rc) rc = grow_staging(h, h->st_flow, h->st_flow_bytes, flow_bytes);
    return rc ? rc : grow_staging(h, h->st_init, h->st_init_bytes, init_bytes);
}

// The device side of an engine whose P / DP the caller has set and checked: stream, events, the report ring, the bicubic table.  A
// failure leaves its text where tf_last_error(NULL) reads it and a half-made engine that engine_destroy takes.
int engine_init(Engine* h, int device_id)
{
    h->dev = device_id;
    auto bail = [&](hipError_t e, const char* what) { return fail(nullptr, TF_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    h->stream = h->own_stream;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) h->num_cus = cus;
    for (const void* k : {reinterpret_cast<const void*>(k_iter2_rows), reinterpret_cast<const void*>(k_iter_rows)})
        if ((e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)) != hipSuccess) return bail(e, "hipFuncSetAttribute");
    for (auto& ev : h->ev) if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e, "hipEventCreate");
    void* hp = nullptr; void* dp = nullptr;
    if ((e = hipHostMalloc(&hp, SLOT_RING * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return bail(e, "hipHostMalloc");
    h->tv.slots_host = (volatile int*)hp;
    if ((e = hipHostGetDevicePointer(&dp, hp, 0)) != hipSuccess) return bail(e, "hipHostGetDevicePointer");
    h->tv.slots_dev = (int*)dp;
    for (int i = 0; i < SLOT_RING; ++i) h->tv.slots_host[i] = -1;
    // bicubic coefficient table of cv::remap (interpolateCubic, A = -0.75, 1/32-px steps), float arithmetic
    float tab[128];
    const float A = -0.75f, scale = 1.f / 32;
    for (int i = 0; i < 32; ++i) {
        const float x = i * scale;
        float* c = tab + i * 4;
        c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
        c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
        c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
        c[3] = 1.f - c[0] - c[1] - c[2];
    }
    if ((e = hipMalloc(&h->tv.tab, sizeof tab)) != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemcpyAsync(h->tv.tab, tab, sizeof tab, hipMemcpyHostToDevice, h->stream)) != hipSuccess) return bail(e, "hipMemcpy");
    if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    return TF_OK;
}

// drains the engine's stream and gives back everything engine_init and the solvers made (the Engine object itself is the caller's)
void engine_destroy(Engine* h)
{
    (void)hipSetDevice(h->dev);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->tv.release(); h->df.release(); h->coop.release(); release_staging(h);
    dev_free(h->tv.tab);
    if (h->tv.slots_host) (void)hipHostFree((void*)h->tv.slots_host);
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& pe : h->prof_pool) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    for (auto& e : h->cev) if (e) (void)hipEventDestroy(e);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
}

// One profiled launch (tf_set_profile): `launch` between the two events of a record.  level -4 = warp, -5 = median, >= 0 = a tvl1_iter
// launch of (level, warp, it) or a DeepFlow SOR launch (tf_dbg_launch_profile lists these).  Without profiling: `launch` alone.
template <class Launch>
int profiled(Engine* h, hipStream_t s, int level, int warp, int it, Launch&& launch)
{
    if (!h->profile) { launch(); return TF_OK; }
    if (h->tally.prof_used == h->prof_pool.size()) {
        ProfEv pe;
        hipError_t e = hipEventCreate(&pe.a);
        if (e == hipSuccess && (e = hipEventCreate(&pe.b)) != hipSuccess) (void)hipEventDestroy(pe.a);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(h, TF_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e)); }
        h->prof_pool.push_back(pe);
    }
    ProfEv& pe = h->prof_pool[h->tally.prof_used++];
    pe.level = level; pe.warp = warp; pe.it = it;
    HIPC(h, hipEventRecord(pe.a, s));
    launch();
    HIPC(h, hipEventRecord(pe.b, s));
    return TF_OK;
}
}  // namespace
