/*
 * teeflow.h -- C ABI of libteeflow_hip.so, the MI355X (gfx950) dense optical-flow engine.
 *
 * Drop-in boundary.  The reference is pure Python; on its hot path it holds a
 * cv2.DenseOpticalFlow object and calls three things on it.  Each entry point below names the
 * reference interface it replaces (paths relative to /root/reference):
 *
 *   cv2.optflow.createOptFlow_DualTVL1()            optical_flow/calculate_optical_flow.py:577   -> tf_create
 *   cv2.cuda.OpticalFlowDual_TVL1.create()          optical_flow/calculate_optical_flow.py:575   -> tf_create
 *   OF_model.setLambda(config.lambda_value)         optical_flow/calculate_optical_flow.py:578   -> tf_set_param
 *   OF_model.calc(I0, I1, None)                     optical_flow/calculate_optical_flow.py:642   -> tf_calc_pair
 *   GpuMat.upload x2 + calc + download              optical_flow/calculate_optical_flow.py:634-639 -> tf_calc_pair
 *   the per-frame-pair loop of process_video()      optical_flow/calculate_optical_flow.py:584-600 -> tf_calc_seq
 *   (batch of independent pairs, BASELINE config 3)                                              -> tf_calc_pairs
 *
 * Plain pointers and sizes only; no torch / numpy types.  The library owns all device memory and its
 * HIP streams.  A handle is NOT re-entrant (mirrors the cv2 object, which the reference also reuses
 * sequentially from one thread), but handles are independent of each other: several handles on ONE
 * device may be driven from several host threads at once.
 *
 * Sub-batches and lanes.  A handle solves up to max_batch (128) pairs at a time.  A call that holds more
 * -- tf_calc_pairs with 1024 pairs, tf_calc_seq on a 1025-frame study -- is cut into equal sub-batches (as few as fit, a multiple of
 * the lane count of them: 1024 pairs = 9 x 114) that the
 * handle's LANES (engines of their own inside the library: stream, buffers, host thread; three for
 * DualTVL1, two for DeepFlow) take from a queue one at a time: a lane that has finished a sub-batch starts
 * the next at once, so one sub-batch's tail (few pairs still iterating) runs under the others' full
 * launches.  A call of at most one sub-batch, on an idle queue, is cut into "lanes" (2) contiguous units
 * that the lanes solve side by side (fewer while a unit would hold under 16 pairs; one: the handle alone).  The call returns when all of its sub-batches are done (if one fails, those not yet started
 * are dropped, the ones running finish, and the call returns the failure with nothing left in flight).
 * tf_submit_* queue the same job without waiting (tf_wait collects it), so that consecutive batches --
 * the studies of a folder, the steps of a stream -- keep the lanes busy across calls.  Flows and
 * tf_get_iters are identical whichever lane solved what.  Chained sequences (tf_chain_next) are the
 * exception to the cutting: a chain is one unit, and several chains of one frame size advance in
 * lock-step inside one call, cut over time instead (tf_calc_chains).
 * All functions return TF_OK (0) or an error
 * code; tf_last_error() gives the message (the Python layer raises OpticalFlowCalculationError,
 * reference optical_flow/exceptions.py:26-28).
 *
 * Flow convention (same as cv2): flow[y][x][0] = x displacement, flow[y][x][1] = y displacement, in
 * pixels per frame, such that I1(x + u, y + v) ~= I0(x, y).
 */
#ifndef TEEFLOW_H
#define TEEFLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TF_ABI_VERSION 2   /* 2: tf_stats grew the per-stage times ms_warp .. ms_sched.  Round 5 ADDED entry points (tf_submit_*, tf_wait,
                              tf_saliency_frames_f32, tf_calc_seq_saliency_f32) and changed no struct and no signature: still 2; so did
                              tf_clean_masks, tf_av_centroids, tf_radlong_project_param, tf_polar_project_param, tf_otsu_masks,
                              tf_radlong_overlay, tf_segmentor_input, tf_segmentor_classmap, and the float16 payload calls
                              (tf_calc_seq_rgb_f16, tf_submit_seq_rgb_f16, tf_calc_seq_saliency_f16, tf_echo_frames, tf_dbg_f16_round)
                              and the WASE study calls (tf_calc_seq_rgb_wase, tf_calc_seq_saliency_wase), and inflate on the device
                              (tf_inflate, tf_hold_study_chunks, tf_hold_mask_chunks with the new struct tf_chunked), and deflate on the
                              device (tf_deflate, tf_deflate_array, tf_held_deflate), and the test hook tf_dbg_luma_stats */

enum {
    TF_OK = 0,
    TF_ERR_INVALID_ARG = 1,   /* null pointer, non-positive size, ... (cv2 would raise cv2.error) */
    TF_ERR_UNSUPPORTED = 2,   /* parameter combination the engine does not implement */
    TF_ERR_HIP = 3,           /* a HIP runtime call failed; message in tf_last_error */
    TF_ERR_NOMEM = 4,
    TF_ERR_NO_DEVICE = 5      /* no gfx950 device visible: there is NO CPU fallback */
};

enum { TF_ALGO_TVL1 = 0, TF_ALGO_DEEPFLOW = 1 /* handles come from tf_create_deepflow */ };

/* Which OpenCV DualTVL1 the handle reproduces.  TF_VARIANT_CPU (default, the parity target): cv2.optflow's
 * DualTVL1OpticalFlow, what calculate_optical_flow.py:577-578, 642 runs without CUDA.  TF_VARIANT_CUDA (SURVEY.md row
 * a5): the semantics of cv2.cuda.OpticalFlowDual_TVL1 (calculate_optical_flow.py:572-575, 633-639), what the reference
 * runs for OF_algo='TVL1' on a CUDA box -- one loop of inner*outer iterations per warp, no median filtering, the error sum
 * looked at on odd iterations only, weight-normalised Catmull-Rom warp with clamp addressing (details and what is not
 * modelled: oracle/tvl1_oracle.c, variant 1). */
enum { TF_VARIANT_CPU = 0, TF_VARIANT_CUDA = 1 };

/* keys for tf_set_param / tf_get_param: the 12 cv2.DualTVL1OpticalFlow setters */
enum {
    TF_PARAM_TAU = 0, TF_PARAM_LAMBDA = 1, TF_PARAM_THETA = 2, TF_PARAM_NSCALES = 3,
    TF_PARAM_WARPS = 4, TF_PARAM_EPSILON = 5, TF_PARAM_INNER_ITERATIONS = 6,
    TF_PARAM_OUTER_ITERATIONS = 7, TF_PARAM_SCALE_STEP = 8, TF_PARAM_GAMMA = 9,
    TF_PARAM_MEDIAN_FILTERING = 10, TF_PARAM_USE_INITIAL_FLOW = 11,
    TF_PARAM__COUNT = 12
};

typedef struct tf_params {
    double tau, lambda, theta, epsilon, scale_step, gamma;
    int nscales, warps, inner_iterations, outer_iterations, median_filtering, use_initial_flow;
    int algo;        /* TF_ALGO_* */
    int max_batch;   /* pairs resident per sub-batch (0 = default 128) */
    int variant;     /* TF_VARIANT_* (ABI 2) */
} tf_params;

/* Filled by every tf_calc_* call (may be NULL). Times are milliseconds (HIP events on the handle's stream). */
typedef struct tf_stats {
    int n_pairs;               /* pairs solved by the call */
    int nscales_used;          /* pyramid levels actually used (<= nscales) */
    int warps;
    int reserved0;
    double ms_total;           /* whole call, host clock */
    double ms_h2d, ms_device, ms_d2h;
    /* dominant kernel (tvl1_iter): launches, summed duration (only when profiling is on) and bytes */
    unsigned long long iter_launches;
    unsigned long long iter_pair_steps;    /* DualTVL1: sum over launches of pairs that actually iterated; DeepFlow: pixels x pairs summed over
                                              the SOR launches (a launch's compulsory traffic is 40 B per pixel) */
    double iter_ms;                        /* sum of tvl1_iter launch durations (tf_set_profile(h,1)) */
    double iter_bytes;                     /* algorithmic bytes of all executed pair-iterations (60 B/px) */
    double total_bytes;                    /* algorithmic bytes of the whole solve */
    unsigned long long inner_iters_total;  /* sum over pairs/levels/warps of executed inner iterations */
    unsigned long long outer_iters_total;  /* ... of executed outer iterations (= median passes) */
    /* summed launch durations per stage of the solve, filled like iter_ms only under tf_set_profile(h,1), single lane:
     * ms_warp (k_warp_lds) and ms_median (k_median).  ms_misc and ms_sched are always 0 (they belonged to the free-running
     * scheduler driver removed in round 3; the fields stay so that ABI 2's struct layout does not change). */
    double ms_warp, ms_median, ms_misc, ms_sched;
} tf_stats;

typedef struct tf_handle tf_handle;

/* cv2 defaults: tau .25 lambda .15 theta .3 nscales 5 warps 5 eps .01 inner 30 outer 10 step .8 gamma 0 median 5 */
int tf_default_params(tf_params* p);

/* replaces createOptFlow_DualTVL1() / cuda.OpticalFlowDual_TVL1.create()  (calculate_optical_flow.py:575,577) */
int tf_create(const tf_params* p, int device_id, tf_handle** out);
void tf_destroy(tf_handle* h);

/* cv2.optflow.createOptFlow_DeepFlow() (calculate_optical_flow.py:568) and its OpticalFlowDeepFlow constants; the cv2
 * object exposes no setters in Python, so these are creation-time only.  The handle is used with the same tf_calc_*
 * entry points (OF_model.calc(...), calculate_optical_flow.py:631). */
typedef struct tf_deepflow_params {
    float sigma;                  /* 0.6  Gaussian pre-blur */
    int min_size;                 /* 25   smallest pyramid side */
    float downscale_factor;       /* 0.95 */
    int fixed_point_iterations;   /* 5 */
    int sor_iterations;           /* 25 */
    float alpha, delta, gamma;    /* 1.0, 0.5, 5.0 (VariationalRefinement gets 4*alpha, delta/3, gamma/3) */
    float omega;                  /* 1.6 */
    float zeta, epsilon;          /* 0.1, 0.001 (cv::VariationalRefinement internals) */
    int max_batch;                /* pairs resident per sub-batch (0 = default 128) */
} tf_deepflow_params;
int tf_default_deepflow_params(tf_deepflow_params* p);
int tf_create_deepflow(const tf_deepflow_params* p, int device_id, tf_handle** out);

/* replaces OF_model.setLambda(...) and the 11 sibling setters / getters  (calculate_optical_flow.py:578) */
int tf_set_param(tf_handle* h, int key, double value);
int tf_get_param(tf_handle* h, int key, double* value);

/* use_external != 0: run on the caller's hipStream_t `hip_stream` (NULL = the legacy default stream, which is what
 * torch.cuda.current_stream().cuda_stream reports for torch's default stream); use_external == 0: back to the
 * handle's own non-blocking stream.  Every tf_calc_* still returns only after its work has drained. */
int tf_set_stream(tf_handle* h, void* hip_stream, int use_external);
/* 0 = off; 1 = bracket every tvl1_iter launch with HIP events so tf_stats.iter_ms is filled */
int tf_set_profile(tf_handle* h, int level);

/* replaces OF_model.calc(I0, I1, None)  (calculate_optical_flow.py:631,638,642).
 * I0, I1: host uint8 [H][W] C-contiguous.  flow_out: host float32 [H][W][2]. */
int tf_calc_pair(tf_handle* h, const uint8_t* I0, const uint8_t* I1, int H, int W, float* flow_out, tf_stats* st);

/* replaces the sliding-window loop of process_video() (calculate_optical_flow.py:584-600):
 * frames: host uint8 [N][H][W]; flow_out: host float32 [N-1][H][W][2] = flow(frame i -> frame i+1) * scale.
 * (The caller duplicates the last field, reference :599.) */
int tf_calc_seq(tf_handle* h, const uint8_t* frames, int N, int H, int W, float scale, float* flow_out, tf_stats* st);

/* B independent pairs (BASELINE.json config 3): I0s, I1s host uint8 [B][H][W]; flow_out float32 [B][H][W][2]. */
int tf_calc_pairs(tf_handle* h, const uint8_t* I0s, const uint8_t* I1s, int B, int H, int W, float* flow_out, tf_stats* st);

/* CV_32FC1 frames (host pointers; otherwise identical to tf_calc_pair / tf_calc_pairs).  cv2's DualTVL1 accepts float32 images with
 * values in [0,1] and multiplies them by 255 when it builds level 0; cv2's DeepFlow converts with `convertTo(CV_32F)` and no factor,
 * i.e. takes float frames AS THEY ARE -- a DeepFlow handle does the same (frames in [0,1] stay in [0,1]; zeta and epsilon are not
 * rescaled).  The reference hands over uint8 with no_saliency=True (calculate_optical_flow.py:588) and computeSaliency()'s CV_32F map
 * with no_saliency=False (:586, :631). */
int tf_calc_pair_f32(tf_handle* h, const float* I0, const float* I1, int H, int W, float* flow_out, tf_stats* st);
int tf_calc_pairs_f32(tf_handle* h, const float* I0s, const float* I1s, int B, int H, int W, float* flow_out, tf_stats* st);

/* Same, with every buffer already resident in this device's HBM (pointers are device pointers); work is
 * enqueued on the handle's stream and the call returns after the stream has drained. */
int tf_calc_pairs_device(tf_handle* h, const uint8_t* dI0s, const uint8_t* dI1s, int B, int H, int W,
                         float scale, float* dflow_out, tf_stats* st);
int tf_calc_seq_device(tf_handle* h, const uint8_t* dframes, int N, int H, int W, float scale,
                       float* dflow_out, tf_stats* st);

/* OF_model.calc(I0, I1, flow) with setUseInitialFlow(true) (TF_PARAM_USE_INITIAL_FLOW; DualTVL1, TF_VARIANT_CPU only): B independent
 * pairs, each started from the caller's flow instead of zero.  An initial flow is float32 [H][W][2], x then y displacement in pixels
 * per frame -- the solver's own unit, never multiplied by a call's `scale`.  OpenCV's rule, restated: level 0 of
 * the flow pyramid is the caller's flow; level s is level s-1 resized by INTER_LINEAR with factors (scaleStep, scaleStep) -- the image
 * pyramid's rule and sizes -- times (float)scaleStep, each level rounded to float32 before the next is taken from it; the coarsest level
 * the solve uses starts from its level of that pyramid (with one level: from the flow itself); the duals start at zero and every finer
 * level starts from the upsampled coarser result, as without the flag.  A zero initial flow gives the plain solve bit for bit;
 * non-finite initial flows are undefined.
 *   tf_calc_pairs_init: host pointers.  I0s, I1s: uint8 [B][H][W], or (frames_f32 != 0) float32 [B][H][W] in [0,1] as for
 *     tf_calc_pairs_f32; init_flows: float32 [B][H][W][2]; flow_out: float32 [B][H][W][2].  init_flows == flow_out is allowed (cv2's in/out
 *     `flow`); otherwise the two must not overlap.
 *   tf_calc_pairs_init_device: device pointers, as tf_calc_pairs_device; d_init is unscaled, dflow_out = flow * scale; d_init ==
 *     dflow_out is allowed.
 * With the flag off both calls ignore the initial flows (they may be NULL), as cv2 does.  With the flag ON, every call that carries no
 * initial flow -- tf_calc_pair(s), the _f32 and _device forms, every tf_calc_seq* and tf_submit_* call, the saliency, WASE, float16 and
 * held-payload study calls, and these two with a NULL initial flow -- returns TF_ERR_UNSUPPORTED before any GPU work (a sequence call
 * armed by tf_chain_next, below, carries its own: each pair's is the flow before it).
 * TF_VARIANT_CUDA handles refuse the flag itself, and gamma != 0 stays refused. */
int tf_calc_pairs_init(tf_handle* h, const void* I0s, const void* I1s, int frames_f32, const float* init_flows, int B, int H, int W,
                       float* flow_out, tf_stats* st);
int tf_calc_pairs_init_device(tf_handle* h, const uint8_t* dI0s, const uint8_t* dI1s, const float* d_init, int B, int H, int W, float scale,
                              float* dflow_out, tf_stats* st);

/* A chained sequence, the video idiom `flow = OF_model.calc(frames[k], frames[k+1], flow)` as ONE call (DualTVL1, TF_VARIANT_CPU, with
 * TF_PARAM_USE_INITIAL_FLOW set).  tf_chain_next(h, 1) arms the NEXT solve call of the handle; if that is a sequence call -- tf_calc_seq,
 * tf_calc_seq_device, tf_submit_seq, tf_submit_seq_device, tf_calc_seq_rgb[_f16], tf_submit_seq_rgb[_f16], tf_calc_seq_saliency[_f32|_f16]
 * and the two *_wase forms -- it is solved as a chain: pair 0 starts from zero (the plain solve bit for bit), pair k >= 1 from pair
 * k-1's flow as the solver left it: float32, in pixels per frame, before `scale`, before WASE compensation and before any float16
 * rounding (never read back from the call's output), taken down the pyramid by the rule above; nothing else about a pair's solve
 * changes, so the result equals the loop of tf_calc_pairs_init calls bit for bit, iteration counts included.  The sequence stays on the
 * device and every frame's pyramid is built once, but the pairs are solved one after the other: a chained call is one unit of the lane
 * queue, never split, and costs about N-1 single-pair solves -- several times the batched call (README).  Submitted chains run side by
 * side, one per lane.  With tf_hold_next also armed, the chained float16 study is left held as usual.  The call spends the flag
 * whether it is refused or not; tf_chain_next(h, 0) disarms.  Refused, before any GPU work: arming while TF_PARAM_USE_INITIAL_FLOW is
 * clear (cv2 ignores the flow then: the chain would be the plain solve at N-1 serial steps), or on a DeepFlow or TF_VARIANT_CUDA handle
 * -> TF_ERR_UNSUPPORTED; an armed pairs call -> TF_ERR_INVALID_ARG.  Unarmed sequence calls stay refused while the flag is set.
 * tf_dbg_counter(h, "chain_steps"): pairs solved as chain steps. */
int tf_chain_next(tf_handle* h, int on);

/* Several chained sequences of ONE frame size in lock-step, in one call (DualTVL1, TF_VARIANT_CPU, TF_PARAM_USE_INITIAL_FLOW set; no
 * tf_chain_next needed).  A chain is sequential in time but independent of the other chains, so step k solves pair k of every chain
 * still running as ONE batch, through the kernels that solve a batch of independent pairs: every launch, whose cost one pair cannot
 * fill, carries up to n_chains pairs.  A pair's result does not depend on the batch it is solved in, so chain i gets, bit for bit and
 * iteration count for iteration count, what a chained tf_calc_seq of its own frames gives.  The chains may differ in length; the
 * library orders them by length itself (longest first, stable) and hands the results back in the caller's order.
 *   frames[i]: chain i's gray frames, uint8 [n_frames[i]][H][W]; flows_out[i]: its flows, float32 [n_frames[i]-1][H][W][2] * scale (the
 *   caller repeats a study's last flow where it wants one).  tf_calc_chains: host pointers; tf_calc_chains_device: device pointers
 *   (the two pointer arrays themselves are host memory in both).
 *   tf_calc_chains_rgb: study i as RGB uint8 [n_frames[i]][H][W][3] on the host, conditioned as tf_calc_seq_rgb conditions it; flows to
 *   host float32, or (out_f16 != 0) float16 as tf_calc_seq_rgb_f16 rounds them; echo16_out (NULL, or one pointer per study, NULL to
 *   skip one): the study's echo as in that call.
 * tf_get_iters afterwards: [chain][pair][level][warp][2], chain after chain in the caller's order; tf_stats counts all pairs, and the
 * "chain_steps" counter grows by them.  One engine solves the whole call: with cap = max_batch pairs per sub-batch, a sub-batch is T
 * steps of the S chains still running, S * T <= cap; the seeds carry over from one sub-batch to the next on the device.  The call is one
 * unit of work: it is never split over the lanes (behind submitted jobs it queues as one unit).
 * Refused before any GPU work, TF_ERR_INVALID_ARG: n_chains < 1, a chain of fewer than 2 frames, a null pointer or array; TF_ERR_UNSUPPORTED:
 * a DeepFlow or TF_VARIANT_CUDA handle, TF_PARAM_USE_INITIAL_FLOW clear, more chains than one sub-batch holds pairs (n_chains >
 * max_batch; the message names the limit), images above 2^24 pixels, float16 flows to a device destination, an armed tf_hold_next (a
 * lock-step call holds nothing).  An armed tf_chain_next or tf_hold_next flag is spent by the call, refused or not; a refused call
 * queues nothing.  Not offered: submitted (tf_submit_*) lock-step calls, saliency and WASE forms, held payloads.
 * tf_dbg_chain_order (pure host arithmetic): order_out[s] = the caller's index of the chain the library keeps in state slot s;
 * first_pair_out[i] (or NULL) = where chain i's pairs start in tf_get_iters' output. */
int tf_calc_chains(tf_handle* h, const uint8_t* const* frames, const int* n_frames, int n_chains, int H, int W, float scale,
                   float* const* flows_out, tf_stats* st);
int tf_calc_chains_device(tf_handle* h, const uint8_t* const* dframes, const int* n_frames, int n_chains, int H, int W, float scale,
                          float* const* dflows_out, tf_stats* st);
int tf_calc_chains_rgb(tf_handle* h, const uint8_t* const* rgb, const int* n_frames, int n_chains, int H, int W, float scale, int out_f16,
                       void* const* flows_out, uint16_t* const* echo16_out, tf_stats* st);
int tf_dbg_chain_order(const int* n_frames, int n_chains, int* order_out, long long* first_pair_out);

/* Asynchronous forms of tf_calc_pairs_device, tf_calc_seq_device, tf_calc_pairs and tf_calc_seq (the loop calculate_optical_flow.py:584-597 for SEVERAL studies / batches at a time):
 * the job is queued on the handle's lanes and the call returns with a ticket; every buffer must stay valid and untouched until
 * tf_wait(h, ticket, st) has returned (ticket < 0: all jobs not yet waited for, oldest first; the first failure is returned).
 * Jobs start in submission order; sub-batches of consecutive jobs overlap.  tf_wait leaves the job's iteration counts where
 * tf_get_iters reads them.  While jobs are in flight the synchronous tf_calc_* calls on the same handle queue behind them.
 * uint8 frames only. */
int tf_submit_pairs_device(tf_handle* h, const uint8_t* dI0s, const uint8_t* dI1s, int B, int H, int W, float scale, float* dflow_out, int* ticket);
int tf_submit_seq_device(tf_handle* h, const uint8_t* dframes, int N, int H, int W, float scale, float* dflow_out, int* ticket);
int tf_submit_pairs(tf_handle* h, const uint8_t* I0s, const uint8_t* I1s, int B, int H, int W, float* flow_out, int* ticket);
int tf_submit_seq(tf_handle* h, const uint8_t* frames, int N, int H, int W, float scale, float* flow_out, int* ticket);
/* tf_calc_seq_rgb (below) without waiting: the frames are conditioned at once, into device memory the job owns; `rgb` may be reused as
 * soon as the call returns, `flow_out` belongs to the job until tf_wait.  What process_folder uses to keep the next study's solve on
 * the GPU while the previous one finishes. */
int tf_submit_seq_rgb(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, float* flow_out, int* ticket);
int tf_wait(tf_handle* h, int ticket, tf_stats* st);

/* Frame conditioning of the reference's loop, `img2uint8(rgb2gray(nparr[i]))` (calculate_optical_flow.py:588,
 * optical_flow_utils.py:30-31), on the device: rgb uint8 [N][H][W][3] -> gray uint8 [N][H][W], normalised per frame.
 * tf_calc_seq_rgb = condition + tf_calc_seq without the frames ever returning to the host (flow_out: [N-1][H][W][2]). */
int tf_condition_frames(tf_handle* h, const uint8_t* rgb, int N, int H, int W, uint8_t* gray_out);
int tf_calc_seq_rgb(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, float* flow_out, tf_stats* st);

/* The reference's other preprocessing branch, no_saliency=False (calculate_optical_flow.py:559-560
 * `cv2.saliency.StaticSaliencyFineGrained_create()`, :586 `saliency_obj.computeSaliency(nparr[i])`): the saliency map of every frame
 * takes the place of the conditioned gray frame as the solver's input.  frames: host uint8 [N][H][W][channels], channels 3 (handed to
 * OpenCV's BGR2GRAY in the order given, as the reference does with its RGB frames) or 1.
 *   tf_saliency_frames      -> uint8 [N][H][W]: the algorithm's 8-bit map (what opencv-contrib 3.x returned)
 *   tf_saliency_frames_f32  -> float32 [N][H][W] = that map * (1/255), values in [0,1]: what computeSaliency() returns in
 *                              opencv-contrib 4.x (`dst.convertTo(saliencyMap, CV_32F, 1.0f/255.0f)`), i.e. what the reference's
 *                              OF_model.calc receives under its `opencv-contrib-python>=4.5.0` (requirements.txt:7)
 * tf_calc_seq_saliency / _f32 = maps + tf_calc_seq without the maps returning to the host (flow_out: [N-1][H][W][2]); the _f32 form hands
 * the solver CV_32F frames (DualTVL1 multiplies them by 255 in float, DeepFlow takes them as they are -- see tf_calc_pair_f32) and is
 * the Python layer's default.  Restated from opencv-contrib's saliency module; nothing pins it (oracle/saliency_oracle.c). */
int tf_saliency_frames(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, uint8_t* saliency_out);
int tf_saliency_frames_f32(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, float* saliency_out);
int tf_calc_seq_saliency(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, float scale, float* flow_out,
                         tf_stats* st);
int tf_calc_seq_saliency_f32(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, float scale, float* flow_out,
                             tf_stats* st);

/* The study file's payload from the device: `flow` and `echo` are stored as float16 (calculate_optical_flow.py:400-404,
 * `flow_arr.astype(np.float16)` and `rgb2gray(nparr).astype(np.float16)`).  The *_f16 calls are tf_calc_seq_rgb, tf_submit_seq_rgb and
 * tf_calc_seq_saliency / _f32 (map_f32 != 0) with the flows written as float16 bits: the output kernel multiplies by `scale` in float32,
 * rounds that product to float32 as today, then rounds the float32 to half (nearest-even, subnormal halves kept, overflow to inf) --
 * numpy's `(flows * np.float32(scale)).astype(np.float16)`, bit for bit.  flow16_out: host [N-1][H][W][2] halves; pinned destinations
 * take the overlapped copy-out, pageable ones the in-order path, as for float32 (half the bytes either way).
 * echo16_out (host [N][H][W] halves, or NULL): float16(rgb2gray(frame)) of every frame, the float64 luma rounded ONCE to half (through
 * float32 it differs at 1057 of the 2^24 RGB triples), computed from the upload the conditioning / saliency pass reads anyway.  It is
 * complete when the call -- tf_submit_seq_rgb_f16 included -- returns; the flows of a submitted job are complete at tf_wait.
 * tf_calc_seq_saliency_f16: echo16_out needs channels == 3 (TF_ERR_INVALID_ARG otherwise).  tf_echo_frames is the echo alone
 * (rgb: host uint8 [N][H][W][3]); it runs on the handle's stream and never on a lane's.  Device-pointer float16 destinations are not
 * offered (a held study, tf_hold_next below, is the library's own device copy of the payload). */
int tf_calc_seq_rgb_f16(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, uint16_t* flow16_out, uint16_t* echo16_out,
                        tf_stats* st);
int tf_submit_seq_rgb_f16(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, uint16_t* flow16_out, uint16_t* echo16_out,
                          int* ticket);
int tf_calc_seq_saliency_f16(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, int map_f32, float scale,
                             uint16_t* flow16_out, uint16_t* echo16_out, tf_stats* st);
int tf_echo_frames(tf_handle* h, const uint8_t* rgb, int N, int H, int W, uint16_t* echo16_out);

/* A study with "WASE" background compensation (tf_wase_compensate, below) in ONE call: tf_calc_seq_rgb / tf_calc_seq_saliency (map_f32:
 * the maps reach the solver as float32) at scale 1, the compensation of all N-1 flows against the bkgd mask, the unit scale and the
 * output type, without the flows leaving the device in between:
 *   F[p]          = the solver's float32 flow of frames p, p+1                          (resident, never copied out)
 *   background[p] = np.mean(masked[masked != 0]),  masked = F[p] * bkgd                  (numpy's summation order, as tf_wase_compensate)
 *   flow_out[p]   = (F[p] - background[p]) * scale
 * with three roundings: the difference to float32, the product to float32 (never contracted), and -- out_f16 != 0 -- that float32
 * to half, nearest-even, subnormal halves kept: numpy's `((F[p] - bg) * np.float32(scale))` and its `.astype(np.float16)`, bit for bit.
 * bkgd: host bool bytes [n_frames][H][W][2], n_frames >= 1 and free of N.  flow_out: host [N-1][H][W][2], float32 or (out_f16) halves;
 * echo16_out: host [N][H][W] halves as for the *_f16 calls, or NULL (the saliency form: channels == 3 only); background_out: host
 * float32 [N-1], or NULL.  An empty selection gives a NaN background and NaN flows, as numpy does.  Arguments are checked as by the
 * calls combined here (TF_ERR_INVALID_ARG: null pointers, N < 2, sizes < 1, n_frames < 1, an echo of non-RGB frames; TF_ERR_UNSUPPORTED:
 * more than 65535 frames or mask frames); a refused call has done no work.  Device memory per study, grown on demand and kept with
 * the handle: (N-1) H W 8 bytes of flows, n_frames H W 8 of compacted products, n_frames H W 2 of mask, and the output. */
int tf_calc_seq_rgb_wase(tf_handle* h, const uint8_t* rgb, int N, int H, int W, const uint8_t* bkgd, int n_frames, float scale, int out_f16,
                         void* flow_out, uint16_t* echo16_out, float* background_out, tf_stats* st);
int tf_calc_seq_saliency_wase(tf_handle* h, const uint8_t* frames, int N, int H, int W, int channels, int map_f32, const uint8_t* bkgd,
                              int n_frames, float scale, int out_f16, void* flow_out, uint16_t* echo16_out, float* background_out,
                              tf_stats* st);

/* Mask cleaning of the segmentor modes, `clean_mask` of the reference (calculate_optical_flow.py:90-111 moving_avg_mask, :113-182
 * clean_mask), on the device and exact: for each label l (class id class_ids[l]) and frame,
 *   m      = moving_avg_mask(class_map == id) with its defaults (n = 4, threshold 0.49; the reference ignores its config there),
 *   filled = binary_fill_holes(m)                (background not 4-connected to the image border becomes foreground),
 *   clean  = remove_small_objects(filled, min_size)   (4-connected foreground components of fewer than min_size pixels go;
 *            min_size <= 0 removes nothing),
 * and bkgd = not (clean of any label).  class_map: host uint8 [N][H][W].  masks_out: host [n_labels + 1][N][H][W][2] bytes of 0 / 1,
 * the labels in class_ids' order and bkgd last; each plane is the reference's bool [N,H,W,2] array (channel duplicated).
 * Runs on the handle's stream and never on a lane's, so it may be called while tf_submit_* jobs of the handle are in flight.  Device
 * scratch, grown on demand and kept by the handle: N*H*W bytes for the class map plus, per chunk of frames, (12 * n_labels + 2) bytes per
 * pixel and frame, with chunks of as many frames as fit in 512 MiB (at least one frame).  Host-synchronous. */
int tf_clean_masks(tf_handle* h, const uint8_t* class_map, int N, int H, int W, const uint8_t* class_ids, int n_labels, long long min_size,
                   uint8_t* masks_out);

/* The Otsu segmentation mode, `predict_movie_thres` of the reference (calculate_optical_flow.py:184-213), on the device and exact: for
 * each uint8 RGB frame,
 *   g      = rgb2gray(frame)                  (float64: ((R/255)*0.2125 + (G/255)*0.7154) + (B/255)*0.0721),
 *   thr    = skimage.filters.threshold_otsu(g)    (256-bin np.histogram over [min g, max g], bin centres, the first maximum of the
 *            between-class variance; a frame of one luma value gets that value, so its mask is empty),
 *   clean  = remove_small_objects(binary_fill_holes(g > thr), min_size)   (both 4-connected; min_size <= 0 removes nothing),
 * and then, over the stack of cleaned planes, moving_avg_mask with its defaults (n = 4, threshold 0.49; the reference ignores its config
 * there).  rgb: host uint8 [N][H][W][3].  masks_out: host [N][H][W][2] bytes of 0 / 1, the reference's bool array 'otsu' (channel
 * duplicated).  thresholds_out: host float64 [N], the per-frame thresholds, or NULL.
 * TF_ERR_INVALID_ARG for a null pointer (thresholds_out excepted) or N < 2, H < 2 or W < 2 (the reference's np.squeeze changes meaning
 * or raises there); TF_ERR_UNSUPPORTED for frames of more than 2^31 - 1 pixels or more than 65535 frames; both before any GPU work.
 * Runs on the handle's stream and never on a lane's, so it may be called while tf_submit_* jobs of the handle are in flight; works on a
 * DualTVL1 or a DeepFlow handle.  Device scratch, grown on demand and kept by the handle: 6 bytes per pixel and frame for the study
 * (frames, cleaned planes, output) plus, per chunk of frames, tf_clean_masks' 10 bytes per pixel and frame of labelling scratch, with
 * chunks of as many frames as fit in 512 MiB (at least one frame).  Host-synchronous. */
int tf_otsu_masks(tf_handle* h, const uint8_t* rgb, int N, int H, int W, long long min_size, uint8_t* masks_out, double* thresholds_out);

/* The frame glue around the SAM segmentor, `evaluate_1_slice` of the reference (calculate_optical_flow.py:47-88), on the device and
 * exact.  The network itself stays the caller's (PyTorch); these two calls stand before and behind it.
 *
 * tf_segmentor_input: for each uint8 RGB frame, PIL's Image.resize((out_w, out_h), BILINEAR) -- its two passes with 22-bit fixed-point
 * coefficients and the uint8 rounding between them -- then ToTensor and Normalize as a table look-up: d_out[n][c][y][x] =
 * lut[c][resized[n][y][x][c]].  rgb: host uint8 [N][H][W][3].  lut: host float32 [3][256], the caller's ((b / 255) - mean[c]) / std[c]
 * (tee_optical_flow_amd.masks.segmentor_lut builds it with the reference's torch expression).  d_out: DEVICE float32
 * [N][3][out_h][out_w] on the handle's device, 16-byte aligned when out_w % 4 == 0.
 * Runs on hip_stream (NULL: the handle's stream) and does NOT wait for its kernel: work the caller queues on that stream afterwards is
 * ordered behind it, and d_out must not be read from another stream without such an order.  rgb and lut are copied before the call
 * returns, so the caller may free them at once.  Device scratch and pinned staging, grown on demand and kept by the handle: 3 bytes per
 * pixel and frame of the call plus the tables, each.
 *
 * tf_segmentor_classmap: class_map_out[n][y][x] = argmax over c of d_logits[n][c][iy[y]][ix[x]] with (iy, ix) the source indices of
 * PIL's Image.resize((W, H), NEAREST) from h x w -- the reference's argmax, uint8 cast and NEAREST resize.  The argmax is torch's on
 * the CPU: the lowest index of equal maxima, a NaN counts as the maximum and the first NaN wins.  d_logits: DEVICE float32
 * [N][C][h][w], written by work queued on hip_stream (NULL: the handle's stream) or finished.  class_map_out: host uint8 [N][H][W].
 * Host-synchronous.  Device scratch: N*H*W bytes and the two index tables.
 *
 * Both: TF_ERR_INVALID_ARG for a null pointer or a non-positive dimension; TF_ERR_UNSUPPORTED for C > 256 or a plane (H*W, out_h*out_w,
 * h*w) of more than 2^31 - 1 elements; both before any GPU work.  They work on a DualTVL1 or a DeepFlow handle and never use a lane's
 * stream, so they may be called while tf_submit_* jobs of the handle are in flight. */
int tf_segmentor_input(tf_handle* h, const uint8_t* rgb, int N, int H, int W, int out_h, int out_w, const float* lut, float* d_out,
                       void* hip_stream);
int tf_segmentor_classmap(tf_handle* h, const float* d_logits, int N, int C, int h_in, int w_in, int H, int W, uint8_t* class_map_out,
                          void* hip_stream);

/* ---- radial / longitudinal projection + per-frame statistics of the reference's analysis step
 *      (optical_flow/analysis.py:89-212: calculate_comp_magnitude, calc_bidirectional_hist), float64, on the device.
 * tf_radlong_project: flow host float32 [N][H][W][2], centroids host float64 [N][2] = (row, col).  rad_out / long_out
 *   (host float64 [N][H][W]) may be NULL.  minmax[4] = rad min, rad max, long min, long max over the whole arrays
 *   (zeros included, as np.min/np.max); nonzero[2N] = per frame count of non-zero rad / long values.  The projections
 *   stay resident for the two calls below (which: 0 = radial, 1 = longitudinal).
 * tf_radlong_hist: np.histogram(frame[frame != 0], bins=nbins, range=(edges[0], edges[nbins])) per frame, RAW counts.
 * tf_radlong_select: exact order statistics: values[n][j] = sorted(frame n's non-zero values)[ranks[n][j]] for up to 4
 *   ranks per frame (rank < 0 = skip) -- what np.percentile interpolates between.
 * tf_radlong_hist and tf_radlong_select act on the planes of the LAST projection call of the handle: tf_radlong_project or
 *   tf_radlong_project_param (which 0 = radial, 1 = longitudinal), or tf_polar_project_param (which 0 = magnitude, 1 = angle). */
int tf_radlong_project(tf_handle* h, const float* flow, const double* centroids, int N, int H, int W,
                       double* rad_out, double* long_out, double* minmax, long long* nonzero);
int tf_radlong_hist(tf_handle* h, int which, const double* edges, int nbins, long long* freq_out);
int tf_radlong_select(tf_handle* h, int which, const long long* ranks, double* values_out);

/* ---- the steps before the projection in calculate_3dhist_radlong(ds, param) (optical_flow/analyze_optical_flow.py:320-343), on the
 *      device, and the area loop of the area-based cardiac-cycle detector.  All run on the handle's stream and never on a lane's, so they may be called while tf_submit_* jobs of the handle are
 *      in flight; both are host-synchronous; every argument is checked before any GPU work.
 * tf_av_centroids: calc_AV_centroid's per-frame loop (optical_flow/analyze_optical_flow.py:202-232, find_correct_centroid :202-211).
 *   masks: host uint8 [N][H][W][C], C = 1 or 2; frame n's set is masks[n][.][.][0] != 0, labelled with 8-connectivity
 *   (skimage.measure.label of a bool image).  centroids_out[n] = (row, col) centroid of the largest component (on a tie in area: the
 *   one whose first pixel in raster order comes first), exactly regionprops' coords.mean(axis=0); area_out[n] = its area, 0 for an
 *   empty frame (centroid (0, 0): the caller applies the reference's empty-frame rule, and the Savitzky-Golay filter).  Device
 *   scratch, grown on demand and kept by the handle: (26 + C) bytes per pixel of a chunk of frames of at most 512 MiB (at least one).
 * tf_first_region_areas: the per-frame area loop of AreaDetector.detect (optical_flow/cardiac_cycle_detection.py:159-172:
 *   skimage.measure.label, regionprops, props[0].area).  masks: host uint8 [N][H][W][C], C = 1 or 2; only channel 0 is read.
 *   area_out[n] = the pixel count of the region labelled 1 in frame n: label joins 8-connected pixels of EQUAL value and numbers the
 *   regions by their first pixel in raster order, so this is the 8-connected region of {masks[n][.][.][0] == v0} that holds the
 *   frame's first non-zero pixel, v0 that pixel's value, whatever the sizes of the frame's other regions (tf_av_centroids' area is
 *   the LARGEST region's, of the set != 0).  0 for an empty frame (a region has at least one pixel: the caller applies the
 *   reference's empty-frame rule, and its smoother and peak search).  TF_ERR_INVALID_ARG for a null pointer, N, H or W < 1 or C outside
 *   {1, 2}; TF_ERR_UNSUPPORTED, with a message, for H*W > 2^31 - 1.  Runs on the handle's stream and never on a lane's; host-synchronous.
 *   Device scratch, grown on demand and kept by the handle: (6 + C) bytes per pixel of a chunk of frames of at most 512 MiB (at least one).
 * tf_radlong_project_param: tf_radlong_project of the parameter field OpticalFlowDataset builds (optical_flow/optical_flow_dataset.py:57,
 *   100-101, 182-228): vel = float32(flow); accel = np.gradient(vel, spacing, axis=0) over all N frames; pwr = vel * accel; each
 *   multiplied by the mask, all float32 as numpy keeps them.  flow: host [N][H][W][2], float16 (flow_is_f16, as the study file holds it)
 *   or float32; only the frames the first n_used need are read.  mask: host uint8 [>= n_used][H][W][mask_C] (mask_C = 1: channel 0 for
 *   both components).  grad_f64 = 1 when the gradient's division runs in float64 in the caller's numpy (a np.float64 spacing under
 *   NEP 50), 0 for float32; spacing must be finite and non-zero for acceleration and PWR, which need N >= 2.  centroids: [n_used][2].
 *   Outputs as tf_radlong_project, for frames [0, n_used); the projections stay resident for tf_radlong_hist / tf_radlong_select.
 *   The resident planes and the upload scratch are grown on demand and kept by the handle. */
#define TF_PARAM_VELOCITY 0
#define TF_PARAM_ACCELERATION 1
#define TF_PARAM_PWR 2
int tf_av_centroids(tf_handle* h, const uint8_t* masks, int N, int H, int W, int C, double* centroids_out, long long* area_out);
int tf_first_region_areas(tf_handle* h, const uint8_t* masks, int N, int H, int W, int C, long long* area_out);
int tf_radlong_project_param(tf_handle* h, const void* flow, int flow_is_f16, int N, int n_used, int H, int W, const uint8_t* mask,
                             int mask_C, int param, double spacing, int grad_f64, const double* centroids, double* rad_out,
                             double* long_out, double* minmax, long long* nonzero);

/* ---- the polar steps of the same consumer, on the device: calculate_3dhist(ds, param, label) (optical_flow/analyze_optical_flow.py:
 *      909-966) and the per-frame angle mode of AngleDetector.detect (optical_flow/cardiac_cycle_detection.py:100-120).
 * tf_polar_project_param: cv2.cartToPolar (CV_32F, radians, as OpenCV 4.x's AVX2 / NEON body computes it) of
 *   the param field tf_radlong_project_param builds (flow, N, n_used, mask, mask_C, param, spacing, grad_f64 as there), for frames
 *   [0, n_used).  mag_out / ang_out: host float32 [n_used][H][W], may be NULL.  minmax[4] = mag min, mag max, ang min, ang max over
 *   the frames (zeros included, as np.min / np.max); nonzero[n_used][2] = per frame count of non-zero mag / ang.  ang_mode[n_used]
 *   = scipy.stats.mode of the frame's non-zero np.round(ang, 2): k / 100.f for the most frequent k = rint(ang * 100.f) in 1..628
 *   (the smallest on a tie), NaN for a frame without any.  mag and ang stay resident, as float64 (exact), for tf_radlong_hist /
 *   tf_radlong_select (which 0 = magnitude, 1 = angle).  Runs on the handle's stream and never on a lane's, so it may be called
 *   while tf_submit_* jobs of the handle are in flight; host-synchronous; every argument is checked before any GPU work.  The
 *   resident planes and the scratch (the uploads, 2.5 KiB per frame, and 8 bytes per pixel when mag_out or ang_out is asked
 *   for) are grown on demand and kept by the handle. */
int tf_polar_project_param(tf_handle* h, const void* flow, int flow_is_f16, int N, int n_used, int H, int W, const uint8_t* mask,
                           int mask_C, int param, double spacing, int grad_f64, float* mag_out, float* ang_out, float* minmax,
                           long long* nonzero, float* ang_mode);

/* ---- the per-pixel part of visualize_radlong (optical_flow/analyze_optical_flow.py:488-560; visualization.py:241-297, 1045-1051 for
 *      other colormaps), on the device: the radial / longitudinal overlay frames.
 * tf_radlong_overlay acts on the planes of the handle's last tf_radlong_project / tf_radlong_project_param call; n, H and W are theirs.
 *   half = max |rad[0]| (ONE CenteredNorm, frozen by its first call: frame 0 of the radial plane, used for every frame of both
 *   components); t = (a + half) / (2 * half) in float64, 0 everywhere if half == 0, not clipped; LUT index clip(floor(t * 256), 0, 255)
 *   (matplotlib's lookup with under = entry 0, over = entry 255); m2 = the largest channel value among the LUT entries either
 *   component used; out = uint8(((0.5 * (echo / echo max)) + (0.5 * (lut[index] / m2))) * 255), truncating, radial in columns [0, W),
 *   longitudinal in [W, 2W).  echo: host [>= n][H][W], TF_ECHO_F16 (the study file's float16: quotient and its half are float16
 *   operations, as numpy runs them: computed in float32, rounded to half to nearest-even, subnormals kept) or TF_ECHO_U8 (float64
 *   division); the maximum is over the first n frames.  lut_rad / lut_long: float64 [256][3] RGB, finite and >= 0.
 *   out: host uint8 [n][H][2W][3].  info[3] = half, echo max, m2.
 *   TF_ERR_INVALID_ARG with a message: no projection yet; the last projection was tf_polar_project_param; planes that hold NaN or inf;
 *   a negative or non-finite echo value; an echo maximum of 0; a LUT entry that is negative or not finite; 2 * half overflowing;
 *   m2 == 0 (the reference's result in all of these is an undefined cast).  Runs on the handle's stream and never on a lane's, so it may
 *   be called while tf_submit_* jobs of the handle are in flight; host-synchronous; every argument is checked before any GPU work.
 *   Device scratch, grown on demand and kept by the handle: 2 bytes per pixel of the study (the indices), and 8 (float16 echo) or 7 bytes
 *   per pixel of a chunk of frames of at most 512 MiB (at least one frame): the echo and the output. */
#define TF_ECHO_F16 0
#define TF_ECHO_U8  1
int tf_radlong_overlay(tf_handle* h, const void* echo, int echo_kind, const double* lut_rad, const double* lut_long, uint8_t* out,
                       double* info);
/* shape[3] = n, H, W of the rad/long planes tf_radlong_overlay would act on (what sizes its echo and out); all 0 when there are none
 * or the last projection was tf_polar_project_param.  No GPU work. */
int tf_radlong_shape(tf_handle* h, int* shape);

/* ---- the per-pixel part of the reference's other video, the "single component" magnitude overlay (example_peak_plots.py:459-513), on
 *      the device: the magnitude of get_masked_arr(param, label) through one colormap, blended half and half with the echo.
 * tf_magnitude_overlay builds the param field itself (flow, flow_is_f16, N, H, W, mask, mask_C, param, spacing, grad_f64 as
 *   tf_radlong_project_param, except that the mask covers ALL N frames: host uint8 [N][H][W][mask_C]) and leaves the resident rad/long
 *   or polar planes of the handle's last projection as they are.
 *   mag = sqrt(x*x + y*y) in float32, every step rounded, nothing fused (np.sqrt(x**2 + y**2); not cv2.cartToPolar's magnitude);
 *   vmin, vmax = min, max of mag over all N frames, zeros outside the mask included (ONE Normalize for the study);
 *   frames [0, n_used) are rendered: t = (mag - vmin) / (vmax - vmin) in float32, where the divisor is the float64 difference and the
 *   quotient is rounded to float32 once (norm_f64 = 1: numpy >= 2 under matplotlib's float64 scalars) or the difference rounded to
 *   float32 first (norm_f64 = 0: numpy 1.x); 0 everywhere if vmin == vmax; LUT index min(trunc(t * 256), 255);
 *   per frame: emax = the echo's maximum, cmax = the largest channel among the LUT entries the frame used;
 *   v = ((0.5 * (echo / emax)) + (0.5 * (lut[index] / cmax))) * 255 in float64, with echo / emax = echo when emax == 0 and
 *   lut / cmax = lut when cmax == 0.  echo: host [>= n_used][H][W]; TF_ECHO_F16: the echo term is float16 arithmetic as in
 *   tf_radlong_overlay, and v is stored into a float16 array (rounded to half, nearest-even) before uint8 truncates it, as the
 *   reference's np.zeros_like(gray2rgb(echo)) output does; TF_ECHO_U8: float64 division, v truncated directly.
 *   lut: float64 [256][3] RGB, finite and >= 0.  out: host uint8 [n_used][H][W][3].  info[2] = vmin, vmax.
 *   frame_info[n_used][2] = echo max, colour max of each frame.
 *   TF_ERR_INVALID_ARG for a null pointer, sizes < 1, n_used > N, mask_C outside {1, 2}, an unknown param or echo kind, acceleration
 *   or PWR with N < 2 or a spacing that is zero or not finite; with a message: a LUT entry that is negative or not finite; NaN or inf
 *   in the magnitude; a negative or non-finite echo value (the reference's result in the last two is an undefined cast).
 *   TF_ERR_UNSUPPORTED, with a message, for H*W >= 2^28 or N > 65535.  Runs on the handle's stream and never on a lane's, so it may be
 *   called while tf_submit_* jobs of the handle are in flight; host-synchronous; every argument is checked before any GPU work.
 *   Device scratch, grown on demand and kept by the handle: the flow and mask uploads (the projections' upload scratch, all N
 *   frames), 1 byte per pixel of the n_used frames (the indices), 64 B + 6 KiB per frame (its words and colour terms), and 5 (float16
 *   echo) or 4 bytes per pixel of a chunk of frames of at most 512 MiB (at least one frame; tf_set_tuning "overlay_chunk_kib"): the
 *   echo and the output.
 * tf_held_magnitude_overlay: the same of the held study's flow and echo and the mask in `slot`, which must cover all N held frames;
 *   refusals as the other tf_held_* calls', by message. */
int tf_magnitude_overlay(tf_handle* h, const void* flow, int flow_is_f16, int N, int n_used, int H, int W, const uint8_t* mask, int mask_C,
                         int param, double spacing, int grad_f64, int norm_f64, const void* echo, int echo_kind, const double* lut,
                         uint8_t* out, double* info, double* frame_info);

/* ---- a study HELD on the device: the study file's payload put there once, and the consumer's tail reading it there.  The calls above
 *      take host arrays and upload them on every call; one 65-frame 512 x 512 study's tail (three rad/long params, three polar params,
 *      angle mode, area series, AV centroids, overlay) uploads the same flow seven times and the same masks eight times.  A held study
 *      lives in device buffers of the handle's own -- not in the scratch the other calls share, so no other call overwrites it -- until
 *      the next tf_hold_study / armed study call, tf_release_study or tf_destroy.
 *      Device memory, allocated per study and freed with it: N H W 4 bytes of flow, n_echo H W 2 of echo, n_frames H W C per mask slot.
 * tf_hold_study: flow16 host float16 [N][H][W][2] (the file's `flow`), echo16 host float16 [n_echo][H][W] or NULL with n_echo 0.
 *   Replaces any held study and empties every mask slot.
 * tf_hold_mask: mask host uint8 [n_frames][H][W][C], C = 1 or 2, H and W the held study's, into slot [0, TF_HELD_SLOTS); replaces
 *   what the slot held.
 * tf_hold_next(h, 1): arms the NEXT study call of the handle, which must be a synchronous float16 one (tf_calc_seq_rgb_f16,
 *   tf_calc_seq_saliency_f16, or a *_wase call with out_f16), to leave its payload held: its N - 1 flows and the last one repeated
 *   (N frames, what the file holds), and its echo if the call makes one -- copied on the device from what the call wrote there, never
 *   uploaded; the call's host outputs are the same bytes as without.  The flag is spent by that call whether it succeeds or is
 *   refused.  Armed, a float32 study call or a submitted one (tf_submit_*) is refused with TF_ERR_UNSUPPORTED and a message.  The
 *   study held before goes once the armed call's arguments have passed; if the call fails after that, no study is held.
 * tf_calc_seq_rgb_held: tf_calc_seq_rgb_f16 after tf_hold_next without the host arrays.  The plain RGB study (host uint8
 *   [N][H][W][3]) is solved as that call solves it -- either solver, tf_chain_next honoured -- and its payload is left held: N float16
 *   flow frames, the last one repeated, and (with_echo != 0) N echo frames.  No flow and no echo is copied to the host: each
 *   sub-batch's flows are copied on the device by the engine that solved them, and the echo kernel writes into the held echo.
 *   *st, tf_get_iters and every refusal are the float16 call's (N < 2, a null pointer, the solve calls' limits); both flags are
 *   spent by the call, the study held before goes once the arguments have passed, and a call that fails after that holds nothing.
 *   There is no submitted form.  tf_dbg_counter(h, "study_download_bytes"): the bytes of flow and echo that the study calls
 *   (tf_calc_seq_rgb*, tf_calc_seq_saliency*, the *_wase calls) have copied device -> host since the handle was made, counted when
 *   a synchronous call returns; this call adds nothing.
 * tf_held_shape: out[TF_HELD_SHAPE_LEN] = N, H, W, n_echo (all 0: none held), a generation number that grows with every replacement
 *   and release, then per slot (n_frames, C), both 0 for an empty slot.  No GPU work.
 * tf_release_study frees the buffers (tf_destroy does too).
 * tf_held_*: the call of the same name without `held_`, reading the held flow (float16) / echo and the mask in `slot`; H, W and the
 *   flow's N are the held study's and the mask's C its slot's; every other argument and every output as the original's (the N of
 *   tf_held_av_centroids and tf_held_first_region_areas: the mask's first N frames).  Same internal function, same kernels, same
 *   bits; tf_radlong_hist / _select / _shape act on the planes a held projection leaves.  Like the originals they run on the handle's
 *   stream and never on a lane's, are host-synchronous, check every argument before any GPU work and may be called while tf_submit_*
 *   jobs of the handle are in flight.  TF_ERR_INVALID_ARG with a tf_last_error text that names the cause: no held study; a slot that is
 *   empty or out of range; n_used outside [1, N]; a mask of fewer frames than asked for; no held echo, or one of fewer frames than the
 *   planes (or of another size); acceleration or PWR with N < 2 or a spacing that is zero or not finite; a null pointer.  A refused
 *   call leaves the held study and the resident planes as they were.
 * tf_dbg_counter(h, "tail_upload_bytes"): bytes of flow, mask and echo that tf_av_centroids, tf_first_region_areas, the three
 *   projections and tf_radlong_overlay have copied host -> device since the handle was made, plus what tf_hold_study and tf_hold_mask
 *   uploaded; the tf_held_* calls add nothing. */
#define TF_HELD_SLOTS 12
#define TF_HELD_SHAPE_LEN (5 + 2 * TF_HELD_SLOTS)
int tf_hold_study(tf_handle* h, const uint16_t* flow16, int N, int H, int W, const uint16_t* echo16, int n_echo);
int tf_hold_mask(tf_handle* h, int slot, const uint8_t* mask, int n_frames, int C);
int tf_hold_next(tf_handle* h, int on);
int tf_calc_seq_rgb_held(tf_handle* h, const uint8_t* rgb, int N, int H, int W, float scale, int with_echo, tf_stats* st);
int tf_held_shape(tf_handle* h, long long* out);
int tf_release_study(tf_handle* h);
int tf_held_av_centroids(tf_handle* h, int slot, int N, double* centroids_out, long long* area_out);
int tf_held_first_region_areas(tf_handle* h, int slot, int N, long long* area_out);
int tf_held_radlong_project_param(tf_handle* h, int n_used, int slot, int param, double spacing, int grad_f64, const double* centroids,
                                  double* rad_out, double* long_out, double* minmax, long long* nonzero);
int tf_held_polar_project_param(tf_handle* h, int n_used, int slot, int param, double spacing, int grad_f64, float* mag_out, float* ang_out,
                                float* minmax, long long* nonzero, float* ang_mode);
int tf_held_radlong_overlay(tf_handle* h, const double* lut_rad, const double* lut_long, uint8_t* out, double* info);
int tf_held_magnitude_overlay(tf_handle* h, int n_used, int slot, int param, double spacing, int grad_f64, int norm_f64, const double* lut,
                              uint8_t* out, double* info, double* frame_info);

/* ---- FRAMES held on the device: a study's RGB frames put there once, in the form its file stores them, and read there by every call
 *      that takes frames.  Without this every such call uploads the same 3 bytes per pixel again (tf_otsu_masks or tf_segmentor_input,
 *      then the study call, then tf_echo_frames ...), and the host prepares them first (the reference's calculate_optical_flow.py:524-548:
 *      pydicom's YBR -> RGB conversion, gray2rgb, np.flip(axis=2)).  The held frames live in a buffer of the handle's own, separate from
 *      the held study above: neither touches the other.  All of it runs on the handle's stream (tf_set_stream included) and is waited for.
 * tf_hold_frames: src host uint8, N frames of H x W in `form`; flip_lr != 0 mirrors the columns (np.flip(axis=2)).  The source bytes
 *   are uploaded as stored and k_ingest writes uint8 RGB [N][H][W][3]; whatever frames were held before are replaced.
 *     TF_FRAMES_RGB       [N][H][W][3]   no arithmetic; without flip_lr no kernel either, the upload goes straight into the held buffer
 *     TF_FRAMES_GRAY      [N][H][W]      gray2rgb: the byte three times
 *     TF_FRAMES_YBR_FULL  [N][H][W][3] of Y, Cb, Cr (what pydicom's pixel_array is for YBR_FULL and YBR_FULL_422): DICOM PS3.3
 *       C.7.6.3.1.2's inverse in float32, in one fixed order: (y, cb, cr) = (Y, Cb - 128, Cr - 128); per output channel
 *       t = y * m0; t = fma(cb, m1, t); t = fma(cr, m2, t); out = uint8(clamp(floor(t + 0.5f), 0, 255)), m the float32 roundings of
 *       [[1, 1, 1], [0, -0.114 * 1.772 / 0.587, 1.772], [1.402, -0.299 * 1.402 / 0.587, 0]] (row = input, column = output).  The numpy
 *       twin is frames.ybr_full_to_rgb; parity with pydicom's convert_color_space is NOT pinned (tests/test_pydicom_color_probe.py).
 * tf_held_frames_shape: out[4] = N, H, W (all 0: none held) and a generation number that grows with every replacement and release.
 * tf_release_frames frees the buffer (tf_destroy does too).  tf_download_frames: the held RGB to rgb_out, host [N][H][W][3].
 * tf_frames_next(h, first, count): arms the NEXT frames-taking call of the handle to read held frames [first, first + count) in place
 *   of its host pointer.  The armed call passes a NULL frame pointer, N == count, H and W of the held frames (and channels == 3 where
 *   it has a channel count); otherwise it is refused with TF_ERR_INVALID_ARG and a message that names both shapes, as it is when the
 *   range is outside the held frames or none are held.  The flag is spent by that call, refused or not, and the held frames stay as
 *   they were.  Calls that honour it: the study calls tf_calc_seq_rgb, _rgb_f16, _rgb_held, _rgb_wase, tf_calc_seq_saliency, _f32,
 *   _f16, _wase, tf_submit_seq_rgb, tf_submit_seq_rgb_f16 (a submitted study conditions the frames into its own buffer before submit
 *   returns, so they may be replaced at once), and tf_condition_frames, tf_echo_frames, tf_saliency_frames, tf_saliency_frames_f32,
 *   tf_otsu_masks, tf_segmentor_input (its kernel reads the held frames on the caller's stream: tf_hold_frames and tf_release_frames
 *   wait for it).  The lock-step calls (tf_calc_chains*) spend the flag and refuse with TF_ERR_UNSUPPORTED.
 * tf_dbg_counter(h, "frames_upload_bytes"): bytes of frames that tf_hold_frames and the calls above have copied host -> device since the
 *   handle was made; "frames_held_reads": armed calls that read the held frames; "ingest_kernel_us", "ingest_bytes": k_ingest's device
 *   time in the last tf_hold_frames and the bytes it read and wrote (both 0 where no kernel ran). */
#define TF_FRAMES_RGB      0
#define TF_FRAMES_GRAY     1
#define TF_FRAMES_YBR_FULL 2
int tf_hold_frames(tf_handle* h, const void* src, int form, int flip_lr, int N, int H, int W);
int tf_held_frames_shape(tf_handle* h, long long* out);
int tf_release_frames(tf_handle* h);
int tf_download_frames(tf_handle* h, uint8_t* rgb_out);
int tf_frames_next(tf_handle* h, int first, int count);

/* ---- frames held from DICOM RLE LOSSLESS pixel data (transfer syntax 1.2.840.10008.1.2.5, PS3.5 Annex G), 8-bit samples: the device
 *      decodes the PackBits segments itself, one wave per (frame, segment), so what goes over the bus is the compressed bytes and no
 *      host core touches a pixel.  A frame: a 64-byte header (little-endian uint32 segment count, fifteen little-endian uint32 offsets
 *      from the frame's first byte), then the segments; segment k is sample plane k, H * W bytes, PackBits-coded (control byte c as
 *      int8: 0..127 copy the next c + 1 bytes; -1..-127 write the next byte 1 - c times; -128 nothing); it ends where the next starts,
 *      the last at the frame's end.  What Annex G leaves to the decoder, chosen so that the first H * W bytes are what a
 *      decode-then-trim reader keeps: a segment's decode stops once H * W bytes are produced and the rest of the segment (the
 *      even-length pad, other padding, trailing garbage) is ignored; runs and literals may cross row ends; a literal cut off by the
 *      segment's end gives the bytes that exist; a run whose value byte is missing gives nothing; a segment that ends short fails.
 * A frame's status: 0 ok; 1 bad header (frame shorter than 64 bytes, or segment count != samples); 2 bad offsets (a first offset
 *   other than 64 is allowed, but each of the `samples` offsets must be >= 64, < the frame's length and strictly ascending); 3 a
 *   segment decoded short.  A malformed frame ends with a status: byte i of a frame is read only with i < len, nothing is written
 *   outside the frame's own H * W * samples bytes.  Annex G is the specification; what pydicom's handler makes of a malformed stream is
 *   NOT pinned.  The core is csrc/teeflow_rle_core.h (the same text on host and device), frames.rle_decode_frame its Python twin.
 * Both calls: frame i is the len[i] bytes at blob + off[i] (host; nothing about alignment or padding is assumed); samples is 1 or 3.
 *   Null pointers, N, H or W < 1, H * W > 2^30, a frame of more than 2^32 - 4096 bytes, samples other than 1 or 3 (tf_hold_frames_rle: other than 1 for TF_FRAMES_GRAY and 3 for
 *   TF_FRAMES_RGB / TF_FRAMES_YBR_FULL, or an unknown form) and an off[i] + len[i] that overflows are TF_ERR_INVALID_ARG before any GPU work.
 * tf_rle_decode: -> out_host [N][H][W][samples] and status [N] (both host).  TF_OK when every status is 0; otherwise
 *   TF_ERR_INVALID_ARG, tf_last_error names the first bad frame and its status, status[] is complete, the good frames' outputs are
 *   valid and a bad frame's output is not written (tf_inflate's contract).
 * tf_hold_frames_rle: the compressed bytes are uploaded, decoded into scratch of the handle and waited for once; only when every status
 *   is 0 are the held frames replaced (the generation moves on) and the planes ingested as tf_hold_frames ingests `form` -- RGB / GRAY /
 *   YBR_FULL, flip_lr -- so that the held frames, tf_frames_next and every frames-taking call behave exactly as after tf_hold_frames of
 *   the decoded [N][H][W][samples] array.  On any failure (status may be NULL; where given it is complete) the frames held before stay as they were, generation
 *   and armed range included (tf_hold_study_chunks' rule).
 * tf_dbg_counter: "frames_upload_bytes" grows by the compressed bytes uploaded (the span of the blob that holds the frames);
 *   "rle_kernel_us", "rle_bytes": k_rle_decode's device time in the last of these calls and the bytes it read and wrote (compressed +
 *   decoded); "ingest_kernel_us", "ingest_bytes" as after tf_hold_frames.  tf_rle_stage_bytes(): the bytes of a segment k_rle_decode
 *   stages at a time (the tests walk a stream across every position of that boundary). */
int tf_rle_decode(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                  uint8_t* out_host, int* status);
int tf_hold_frames_rle(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                       int form, int flip_lr, int* status);
int tf_rle_stage_bytes(void);

/* ---- frames held from DICOM JPEG BASELINE pixel data (Process 1, transfer syntax 1.2.840.10008.1.2.4.50), 8-bit samples: the device
 *      parses the entropy data, dequantises, runs the IDCT and upsamples the chroma itself, so what goes over the bus is the compressed
 *      bytes.  Exact: on every valid stream the samples equal libjpeg-turbo's as Pillow drives it (slow-integer IDCT, fancy
 *      upsampling).  The arithmetic, what is accepted and the statuses are fixed in csrc/teeflow_jpeg_core.h (the same text on host and
 *      device); frames.jpeg_decode_frame is the Python twin.  What libjpeg or pydicom make of a MALFORMED stream is NOT pinned: they
 *      repair and warn where this decoder gives a status.
 * A frame is a full interchange stream from SOI on (EOI is not required): SOF0, one component or three with sampling 4:4:4, 4:2:2 or
 *   4:2:0, one interleaved scan, 8-bit quantisation tables, DRI / RSTn; tables may differ from frame to frame.  Per-frame status: 0 ok,
 *   1 bad header, 2 a process that is not decoded, 3 entropy data that does not decode.  Nothing is written outside a frame's own scratch
 *   and output, whatever the stream holds, and no frame's output is written unless its status is 0.
 * Both calls: frame i is the len[i] bytes at blob + off[i] (host; nothing about alignment or padding is assumed); samples is 1 or 3.
 *   Null pointers, N, H or W < 1, H or W > 65535, H * W > 2^30, a frame of more than 2^32 - 4096 bytes, samples other than 1 or 3
 *   (tf_hold_frames_jpeg: other than 1 for TF_FRAMES_GRAY and 3 for TF_FRAMES_RGB / TF_FRAMES_YBR_FULL, an unknown form or color,
 *   TF_JPEG_COLOR_LIBJPEG with a form other than TF_FRAMES_YBR_FULL) and an off[i] + len[i] that overflows are TF_ERR_INVALID_ARG
 *   before any GPU work.
 * tf_jpeg_decode: -> out_host [N][H][W][samples], the stream's own components upsampled, no colour transform, and status [N] (both
 *   host).  TF_OK when every status is 0; otherwise TF_ERR_INVALID_ARG, tf_last_error names the first bad frame and its status,
 *   status[] is complete, the good frames' outputs are valid and a bad frame's output is not written (tf_rle_decode's contract).
 * tf_hold_frames_jpeg: the compressed bytes are uploaded, decoded into scratch of the handle and waited for; only when every status is 0
 *   are the held frames replaced (the generation moves on).  color TF_JPEG_COLOR_NONE: the samples are ingested as tf_hold_frames
 *   ingests `form`, and what is held equals tf_hold_frames of the decoded frames bit for bit.  TF_JPEG_COLOR_LIBJPEG (samples 3, form
 *   TF_FRAMES_YBR_FULL): Y, Cb, Cr go through libjpeg's fixed-point colour tables, and what is held equals tf_hold_frames of the RGB a
 *   libjpeg-backed reader returns, as TF_FRAMES_RGB.  If a frame does not decode the call fails as tf_jpeg_decode does and the frames
 *   held before, their generation, their tokens and an armed range stay as they were.  status (host, [N]) may be null.
 * tf_dbg_counter: "frames_upload_bytes" grows by the compressed bytes uploaded; "jpeg_marks_us", "jpeg_entropy_us", "jpeg_idct_us",
 *   "jpeg_finish_us": the four kernels' device time in the last of these calls; "jpeg_bytes": the compressed bytes read and the sample
 *   bytes written; "jpeg_batches": the batches of frames worked through since the handle was made (a batch's coefficient scratch stays
 *   under 256 MiB; tf_set_tuning "jpeg_batch_kib" lowers that for tests).  tf_jpeg_stage_bytes(): the bytes of a frame the kernels
 *   stage at a time (the tests walk a stream across every position of that boundary). */
#define TF_JPEG_COLOR_NONE 0
#define TF_JPEG_COLOR_LIBJPEG 1
int tf_jpeg_decode(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                   uint8_t* out_host, int* status);
int tf_hold_frames_jpeg(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                        int form, int color, int flip_lr, int* status);
int tf_jpeg_stage_bytes(void);

/* ---- frames held from DICOM JPEG LOSSLESS pixel data (T.81 Process 14, frame marker SOF3; transfer syntaxes 1.2.840.10008.1.2.4.70,
 *      "first-order prediction", and its parent 1.2.840.10008.1.2.4.57), 8-bit samples.  The Huffman-coded value of such a scan is the
 *      prediction difference, so the device's serial entropy pass emits differences only and, with predictor 1, the reconstruction is
 *      prefix sums modulo 2^16: down the first column of a restart interval, then along every row, each row on its own.  Exact by
 *      construction: a valid stream has exactly one decoding, the encoded array.  What is accepted, the rules and the statuses are
 *      fixed in csrc/teeflow_jpegll_core.h (the same text on host and device); frames.jpegll_decode_frame is the Python twin.  What
 *      libjpeg or pydicom make of a MALFORMED stream is NOT pinned: they mask a sample to its precision where this decoder gives a status.
 * A frame is a full interchange stream from SOI on (EOI is not required): SOF3 of precision 8, one component or three sampled 1 x 1,
 *   one interleaved scan with Ss = 1, Se = Ah = Al = 0, Huffman tables of class 0 with ids 0..3, DRI / RSTn with an interval that is a
 *   multiple of W; tables may differ from frame to frame.  Per-frame status: 0 ok, 1 bad header, 2 a process that is not decoded (any
 *   other frame marker, predictor or point transform), 3 data that does not decode -- a reconstructed sample outside 0..255 included.
 *   Nothing is written outside a frame's own scratch and output, whatever the stream holds.
 * Both calls take tf_jpeg_decode's arguments with tf_jpeg_decode's refusals (TF_ERR_INVALID_ARG before any GPU work); tf_jpeg_decode
 *   itself still answers status 2 for an SOF3 stream.
 * tf_jpegll_decode: -> out_host [N][H][W][samples], no colour transform, and status [N] (both host), under tf_jpeg_decode's contract:
 *   TF_OK when every status is 0; otherwise TF_ERR_INVALID_ARG, status[] is complete, the good frames' outputs are valid and a bad
 *   frame's output is not written.
 * tf_hold_frames_jpegll: form TF_FRAMES_GRAY (samples 1), TF_FRAMES_RGB or TF_FRAMES_YBR_FULL (samples 3); the codec applies no colour
 *   transform.  The compressed bytes are uploaded, decoded into scratch of the handle and waited for; only when every status is 0 are
 *   the held frames replaced, and what is held equals tf_hold_frames of the decoded frames bit for bit.  If a frame does not decode the
 *   call fails as tf_jpegll_decode does and the frames held before, their generation, their tokens and an armed range stay as they
 *   were.  status (host, [N]) may be null.
 * tf_dbg_counter: "frames_upload_bytes" grows by the compressed bytes uploaded; "jpegll_entropy_us" (k_jpeg_marks and
 *   k_jpegll_entropy) and "jpegll_restore_us" (k_jpegll_col and k_jpegll_rows): device time in the last of these calls; "jpegll_bytes":
 *   the compressed bytes read and the sample bytes written; "jpegll_batches": the batches of frames worked through since the handle
 *   was made (a batch's differences, 2 bytes a sample, stay under 256 MiB; tf_set_tuning "jpeg_batch_kib" lowers that for tests).
 * The entropy pass of a restart interval has two forms with the same result, frame for frame and status for status.  The serial one is
 *   one wave an interval.  The split one (csrc/teeflow_jpegll_sync_core.h) cuts the interval's data into pieces of
 *   tf_jpegll_segment_bytes() bytes, one lane a piece: every piece is decoded from a guessed start, then handed the exit of the piece
 *   before it round after round -- Huffman streams self-synchronise -- and an interval that a round still changed after the last round
 *   is decoded by the serial form.  tf_set_tuning "jpegll_split": 0 (default) the host picks per frame, before the first launch, by the
 *   bytes of entropy data an interval of the frame holds on average (a frame whose components name different codes stays serial: its
 *   pieces agree on the component only as fast as the truth travels, a block of 256 pieces a round); 1 the serial form only; 2 the split form for every interval (frames
 *   of 128 MiB or more stay serial); any other value is refused.  "jpegll_sync_rounds": the rounds a batch launches, 0..64 (0: the
 *   speculation only; default 8, twice what the measured study needs).  tf_dbg_counter "jpegll_split_intervals": the intervals sent
 *   down the split form since the handle was made; "jpegll_serial_fallbacks": those of them that did not converge and were decoded
 *   serially; "jpegll_sync_rounds": the rounds launched in the last call, all its batches.  "jpegll_entropy_us" covers all entropy work
 *   of either form.  The split form's scratch, 20 bytes a piece, counts into a batch's 256 MiB. */
int tf_jpegll_decode(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                     uint8_t* out_host, int* status);
int tf_hold_frames_jpegll(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, int N, int H, int W, int samples,
                          int form, int flip_lr, int* status);
int tf_jpegll_segment_bytes(void);

/* ---- a study held from the CHUNKS of its file: the gzip chunks of a study file's datasets are independent zlib streams (RFC 1950
 *      around RFC 1951), which the device inflates itself, one wave per stream, and assembles into the row-major arrays; what goes over
 *      the bus is the compressed bytes.  The output bytes are zlib's or the stream is refused: stored, fixed and dynamic blocks, any
 *      window size in the header, the stream's Adler-32 checked; a preset dictionary (FDICT) is refused; bytes after the trailer are
 *      ignored.  A malformed stream ends with a status and writes nothing outside its own output.
 * A stream's status: 0, or 1 bad header (FCHECK, CM != 8, CINFO > 7, FDICT), 2 bad block type, 3 bad stored length, 4 bad code
 *   lengths (over-subscribed or incomplete as zlib judges them, no end-of-block code, or a code the lengths do not define), 5 a distance
 *   before the start of the output, 6 input truncated, 7 output longer or shorter than expected, 8 checksum mismatch.
 * tf_inflate: n streams, stream i the len[i] bytes at blob + off[i] (host), each to out_bytes bytes: out_host [n][out_bytes] (host),
 *   status [n].  raw (or NULL): raw[i] != 0 marks a stream that is not compressed; it is copied as it is and must be out_bytes long.
 *   TF_OK when every status is 0; otherwise TF_ERR_INVALID_ARG, tf_last_error names the first bad stream and its status, status[] is
 *   complete and the good streams' outputs are valid; a bad stream's slot holds what it decoded before it failed and is otherwise
 *   untouched.  Runs on the handle's stream, host-synchronous, like the tail calls.
 * tf_chunked: one chunked dataset.  n chunks, chunk i the len[i] bytes at blob + off[i], raw[i] (raw may be NULL) set where the file's
 *   filter mask says the chunk was stored unfiltered, its first element at coord[i * ndim .. ] of the array; shape and chunk: the
 *   array's and a chunk's extent per dimension (ndim <= 4), elem_bytes 1, 2 or 4, chunk_bytes = the chunk's elements x elem_bytes.  A
 *   chunk at the array's edge is clipped; where the file wrote no chunk the array is 0 (HDF5's fill value).
 * tf_hold_study_chunks: flow 4-D with last dimension 2 and 2-byte elements, echo (or NULL) 3-D with 2-byte elements and the flow's
 *   frame size.  On success the held study is what tf_hold_study of the same arrays leaves.  If any chunk fails to inflate
 *   (TF_ERR_INVALID_ARG; tf_last_error names the chunk) nothing changes: the study held before, its masks and the resident planes stay.
 * tf_hold_mask_chunks: mask 4-D [n_frames][H][W][C], C = 1 or 2, 1-byte elements, H and W the held study's, into `slot`; the same contract.
 * Every argument is checked before any GPU work: null pointers, n < 0, a coord outside the shape, a chunk_bytes that is not the chunk's.
 * "tail_upload_bytes" grows by the compressed bytes uploaded: max(off + len) - min(off) over the call's chunks.
 * tf_dbg_counter(h, "inflate_kernel_us" / "unchunk_kernel_us"): device time of the two kernels since the handle was made (HIP events). */
typedef struct tf_chunked {
    const uint8_t* blob;
    const uint64_t* off;
    const uint32_t* len;
    const uint8_t* raw;
    const int64_t* coord;
    int n, ndim;
    int64_t shape[4], chunk[4];
    int elem_bytes;
    uint32_t chunk_bytes;
} tf_chunked;
int tf_inflate(tf_handle* h, const uint8_t* blob, const uint64_t* off, const uint32_t* len, const uint8_t* raw, int n, uint32_t out_bytes,
               uint8_t* out_host, int* status);
int tf_hold_study_chunks(tf_handle* h, const tf_chunked* flow, const tf_chunked* echo);
int tf_hold_mask_chunks(tf_handle* h, int slot, const tf_chunked* mask);

/* ---- deflate on the device, the mirror of the above: a dataset's chunks, each into the zlib stream that zlib 1.2.11 writes for it at
 *      level 9 (zlib.compress(chunk, 9): header 78 DA, memLevel 8, default strategy, Adler-32), byte for byte -- what a gzip-9 dataset's
 *      write_direct_chunk takes, so the file is the one the host writes.  The match search runs one thread per input byte; the parse, the
 *      Huffman trees and the bits run one thread per chunk.
 * All three give the same outputs: the streams end to end in blob (host, blob_cap bytes; blob_cap must be at least n x
 *   compressBound(chunk_bytes), compressBound(b) = b + (b >> 12) + (b >> 14) + (b >> 25) + 13, checked before any work), chunk i's
 *   stream the len[i] bytes at blob + off[i], off ascending without gaps, status [n].  A status is 0, or 1 the stream passed
 *   compressBound (zlib's never does), 2 a stored block of more than 65,535 bytes; a non-zero status fails the call (TF_ERR_UNSUPPORTED,
 *   tf_last_error names the chunk).  A chunk has at most 16 MiB.
 * tf_deflate: n chunks of chunk_bytes each, packed, in host memory (chunk_bytes 0: n empty streams).
 * tf_deflate_array: a row-major host array of `ndim` (1..4) dimensions `shape` of elem_bytes (1, 2 or 4) byte elements, cut into chunks
 *   of `chunk` elements per dimension as HDF5 stores them: whole chunks, zero beyond the array's edge, in row-major order of the chunk
 *   grid; n must be the number of chunks, the product of ceil(shape[d] / chunk[d]).  coord [n][ndim]: each chunk's first element.  The
 *   outputs with shape, chunk and elem_bytes are a tf_chunked that tf_hold_study_chunks / tf_hold_mask_chunks take back.
 * tf_held_deflate: the same for an array of the held study, read where it is (nothing is uploaded, "tail_upload_bytes" stays): what =
 *   TF_HELD_FLOW ([N][H][W][2], 2-byte elements, chunk[4]), TF_HELD_ECHO ([n_echo][H][W], 2-byte, chunk[3]) or TF_HELD_MASK (the mask
 *   in `slot`, [n_frames][H][W][C], 1-byte, chunk[4]; slot is ignored otherwise).
 * Every argument is checked before any GPU work.  Host-synchronous, on the handle's stream, like the tail calls.  Device scratch: about
 *   12 bytes per input byte plus 192 KiB per chunk, in batches of chunks that keep it under 256 MiB, plus the blob and an uploaded array.
 * tf_dbg_counter(h, "deflate_match_us" / "deflate_emit_us" / "chunk_kernel_us"): device time of the links and the match search, of the
 *   parse, trees, bits and compaction, and of the gather into chunks, since the handle was made (HIP events).
 * tf_dbg_counter(h, "deflate_batches"): the batches of chunks the three calls have worked through since the handle was made. */
enum { TF_HELD_FLOW = 0, TF_HELD_ECHO = 1, TF_HELD_MASK = 2 };
int tf_deflate(tf_handle* h, const uint8_t* chunks, int n, uint32_t chunk_bytes, uint8_t* blob, uint64_t blob_cap, uint64_t* off, uint32_t* len, int* status);
int tf_deflate_array(tf_handle* h, const void* array, int ndim, const int64_t* shape, const int64_t* chunk, int elem_bytes, int n, uint8_t* blob,
                     uint64_t blob_cap, uint64_t* off, uint32_t* len, int64_t* coord, int* status);
int tf_held_deflate(tf_handle* h, int what, int slot, const int64_t* chunk, int n, uint8_t* blob, uint64_t blob_cap, uint64_t* off, uint32_t* len,
                    int64_t* coord, int* status);

/* ---- multi-GPU: the single exchange step of the path.  The reference's loop is sequential
 *      (calculate_optical_flow.py:584-597); here pairs shard over the GPUs of a node with no data-path traffic during the
 *      solve, and ONE RCCL all-gather of the (u,v) fields over xGMI assembles the result on every rank.  librccl is loaded
 *      on first use.  Two ways to form the communicator:
 *        one process per GPU : rank 0 calls tf_comm_unique_id, the launcher hands the 128 bytes to every rank (any
 *                              channel: a file, MPI, torch.distributed's store), each rank calls tf_comm_init_rank;
 *        one process, n GPUs : tf_comm_init_all on n handles created on n different devices (ncclCommInitAll).
 *      tf_allgather_flows enqueues this rank's contribution (count floats, device pointers; recv holds nranks*count)
 *      on the handle's communication stream behind the work already queued on its solve stream and returns at once with
 *      a ticket; tf_comm_wait(h, ticket) blocks the host until that all-gather is done (ticket < 0: all of them), which
 *      is what must happen before d_send / d_recv are reused -- so the exchange of step k overlaps the solve of step k+1.
 *      tf_allgather_flows_all is the single-process form: grouped calls for all n ranks, returns when all are done.
 *      ORDER against the solve that produced d_send, stated: tf_allgather_flows orders the collective behind the work queued on
 *      THIS handle's solve stream and nothing else.  Flows written by the handle's lanes (a call larger than one sub-batch, a
 *      tf_submit_* job) or by ANOTHER handle (a communicator handle that never solves, as round 4's bench.py used) are ordered
 *      by the HOST, by design: every tf_calc_* is host-synchronous and so is tf_wait -- when they have returned, every stream
 *      that worked for them has drained, and the all-gather may be issued at once.  There is no earlier point to hook a stream
 *      dependency on: a solve's launches are issued as its stop reports come back (the iteration count is data-dependent), so
 *      until the call returns the producing streams do not yet hold all of its work, and an event recorded on them would order
 *      the collective behind a prefix of the solve only.  Issue the all-gather after the producing call / tf_wait has returned. */
#define TF_COMM_ID_BYTES 128
int tf_comm_unique_id(unsigned char* id /* [TF_COMM_ID_BYTES] */);
int tf_comm_init_rank(tf_handle* h, int nranks, int rank, const unsigned char* id);
int tf_comm_init_all(tf_handle** handles, int n);
int tf_allgather_flows(tf_handle* h, const float* d_send, size_t count_floats, float* d_recv, int* ticket);
int tf_allgather_flows_all(tf_handle** handles, int n, const float* const* d_send, size_t count_floats, float* const* d_recv);
int tf_comm_wait(tf_handle* h, int ticket);
int tf_comm_destroy(tf_handle* h);

/* Executed iteration counts of the last call: int32 [n_pairs][nscales_used][warps][2] = (inner, outer).
 * Returns the number of ints written (<= capacity) through *written. */
int tf_get_iters(tf_handle* h, int* out, size_t capacity_ints, size_t* written);

/* message of the last failure on this handle (or of the last failed tf_create when h == NULL) */
const char* tf_last_error(tf_handle* h);
int tf_abi_version(void);
int tf_device_count(void);

/* ---- kernel-level test hooks (dense host arrays, one image; used by tests/ to compare each kernel
 *      with the oracle bit for bit; not part of the drop-in surface) -------------------------------- */
/* implementation knobs for experiments (results never change).  DualTVL1: "iter_variant" (0 = 64x16 tiles, 1 = full-width row strips,
 * 2 = row strips with two iterations per launch [default]), "min_rows_work" (rows*pairs below which tiles are used), "strip_blocks" (target
 * blocks per tvl1_iter launch of a sub-batch above 1024 pairs), "strip_test_slots" (tests: >= 1 = the resident-block count the two-iteration
 * row strips of a sub-batch of at most 1024 pairs are sized for on the device is taken to be this, whatever the device and "lane_slots_pct"
 * say, which picks the strip layout; 0 = off [default]; clamped to [0, 2^20]), "lane_slots_pct" (per cent of the resident blocks a queue lane
 * sizes those strips for, default 67), "max_strip_width" (widest level the row strips take), "warp_margin" (pixels of flow the
 * LDS-staged warp covers around its tile: 0 = global gathers only, default 8).  DeepFlow: "sor_rt" (0 = one colour per launch, the plain form),
 * "sor_fuse" (sweeps per launch of the tiled register kernel), "sor_rt_shape" (region shape; 3 = chosen per launch), "sor_coop" (1 = all sweeps
 * of a fixed-point iteration in one launch of co-resident regions where a level needs several [default], 2 = always 128x64 regions, 3 = always
 * 128x32 regions for small batches, 0 = never), "sor_coop_small" (0 = small batches keep the tiled form), "sor_coop_s" (sweeps between two exchanges), "sor_coop_min_util" (per cent of its CUs such a launch must fill, else tiled), "df_fuse_ds" (form of the data/smoothness kernel).
 * Both: "lanes" (contiguous units a call of at most one sub-batch is split into, solved side by side on the queue lanes), "queue_lanes" (lanes
 * that take those units, the sub-batches of larger calls and tf_submit_* jobs from the queue: -1 = 3 for DualTVL1, "lanes" for DeepFlow [default];
 * 0 = no lanes: the handle solves every call alone, sub-batch after sub-batch -- the same flows), "queue_unit" (pairs per queued sub-batch; 0 = equal sub-batches of at most max_batch pairs, a multiple of the lane count of them).
 * tf_radlong_overlay, tf_magnitude_overlay: "overlay_chunk_kib" (tests: the echo and output of a chunk of frames take at most this many KiB, at least one frame; 0 = 512 MiB [default]).
 * tf_first_region_areas: "area_chunk_kib" (tests: the masks and labelling scratch of a chunk of frames take at most this many KiB, at least one frame; 0 = 512 MiB [default]). */
int tf_set_tuning(tf_handle* h, const char* name, int value);
/* counters of the handle for tests and tools: "coop_launches" (launches of the co-resident SOR form since the handle was made),
 * "coop_aborts" (calls repeated with the tiled form because such a launch gave up waiting), "coop_disabled"; "queue_jobs", "queue_units_done",
 * "queue_units_failed", "queue_units_skipped" (sub-batches dropped because an earlier one of their call had failed), "queue_outstanding", "queue_lanes";
 * "tail_upload_bytes" (see tf_hold_study), "study_download_bytes" (see tf_calc_seq_rgb_held); -1 for an unknown name */
long long tf_dbg_counter(tf_handle* h, const char* name);
/* DeepFlow hooks: one cv::VariationalRefinement::calcUV on dense float images (u, v updated in place); 3x3 Gaussian blur */
int tf_dbg_df_refine(tf_handle* h, const float* I0, const float* I1, int w, int hgt, float* u, float* v);
int tf_dbg_df_blur(tf_handle* h, const float* src, int w, int hgt, float* dst);
/* level `level` of DeepFlow's pyramid of one frame (uint8, or float32 with is_f32: taken as it is), by the kernels and the level table of a
 * solve; out may be NULL (the level's size only); a level the pyramid does not have is TF_ERR_INVALID_ARG */
int tf_dbg_df_pyramid(tf_handle* h, const void* frame, int is_f32, int H, int W, int level, float* out, int* ow, int* oh);
/* the flow hand-down between two levels of a DeepFlow solve: (u, v) of sw x sh resized to dw x dh, times 1 / downscale_factor */
int tf_dbg_df_up(tf_handle* h, const float* u, const float* v, int sw, int sh, float* ou, float* ov, int dw, int dh);
/* the float16 output kernels' value function on caller-chosen values: out[i] = bits of half(float32(in[i] * scale)), n <= 2^30 */
int tf_dbg_f16_round(tf_handle* h, const float* in, size_t n, float scale, uint16_t* out);
/* what tf_otsu_masks computes of each frame's float64 luma before it labels anything, by the same three launches (per-frame min / max,
 * the 256-bin histogram over [min, max], Otsu's threshold): RGB frames uint8 [N][H][W][3] (N, H, W >= 1; H * W < 2^31, N <= 65535) ->
 * minmax_out [N][2] (min, max), hist_out [N][256], thr_out [N].  A one-valued frame has min == max, an all-zero histogram and that
 * value as its threshold.  The min / max are also what tf_condition_frames normalises with. */
int tf_dbg_luma_stats(tf_handle* h, const uint8_t* rgb, int N, int H, int W, double* minmax_out, uint32_t* hist_out, double* thr_out);
/* Pinned host memory for flow results.  The reference gets a fresh numpy array from cv2 (`flow = OF_model.calc(...)`,
 * calculate_optical_flow.py:631,642); handing tf_calc_pair/_seq/_pairs a destination from tf_host_alloc (or any pinned
 * host pointer) lets the library copy results out at PCIe speed while the next sub-batch is being solved.  Pageable
 * destinations work too, in order.  tf_host_alloc returns NULL on failure. */
void* tf_host_alloc(size_t bytes);
void  tf_host_free(void* p);
/* "WASE" background compensation (rows a7/f2), replaces the numpy expression of
 * /root/reference/optical_flow/calculate_optical_flow.py:647-652, 659 for ALL flows of a study in one call:
 *   background[p] = np.mean(masked[masked != 0]),  masked = flows[p] * bkgd      (bkgd: bool [n_frames][H][W][2], 0/1 bytes)
 *   flows[p] = (flows[p] - background[p]) * scale                                  (in place)
 * The float32 reduction follows numpy's summation order exactly (8192-element pieces, pairwise sums, float64 divide).
 * tf_wase_compensate takes host pointers, the _device form device pointers; background_out (host, n_flows) may be NULL. */
int tf_wase_compensate(tf_handle* h, float* flows, int n_flows, const uint8_t* bkgd, int n_frames, int H, int W, float scale,
                       float* background_out);
int tf_wase_compensate_device(tf_handle* h, float* flows, int n_flows, const uint8_t* bkgd, int n_frames, int H, int W, float scale,
                              float* background_out);
/* per-launch record of the last solve run with tf_set_profile(h, 1): tvl1_iter launches in issue order (single lane);
 * returns the number of records, fills at most max_n: (level, warp, first iteration) of each launch and its duration. */
int tf_dbg_launch_profile(tf_handle* h, int* level, int* warp, int* it, float* ms, int max_n);
/* strip sizing rule of the tvl1_iter kernel (host arithmetic only): rows per strip R (multiple of RY) and strip count S
 * for n_active pairs still iterating on a device with `slots` resident blocks */
void tf_dbg_strip_rule(int n_active, int H, int RY, int slots, int* R, int* S);
int tf_dbg_pyramid(tf_handle* h, const uint8_t* img, int H, int W, int level, float* out, int* ow, int* oh);
int tf_dbg_resize(tf_handle* h, const float* src, int sw, int sh, float* dst, int dw, int dh,
                  double inv_scale_x, double inv_scale_y, float mul);
int tf_dbg_warp(tf_handle* h, const float* I0, const float* I1, const float* u1, const float* u2, int w, int hgt,
                float* I1wx, float* I1wy, float* rho_c);
int tf_dbg_median(tf_handle* h, const float* src, int w, int hgt, int ksize, float* dst);
int tf_dbg_iterate(tf_handle* h, const float* I1wx, const float* I1wy, const float* rho_c,
                   float* u1, float* u2, float* p11, float* p12, float* p21, float* p22,
                   int w, int hgt, int nsteps, int p_is_zero, unsigned long long* err_q);
/* One (level, warp) stage of a DualTVL1 solve without its warp, for B pairs (1 <= B <= 4096) on the caller's planes: the stage loop a
 * solve runs (medians every `inner` iterations, the tvl1_iter launches in the handle's current form and strip layout, the active-pair
 * reports that end the stage early) and the stage's end (iteration counts, ping-pong bookkeeping).  I1wx, I1wy, rho_c: float32
 * [B][hgt][w]; u1 .. p22: float32 [B][hgt][w], updated in place -- every pair's state as the stage leaves it, read from the ping-pong
 * half the pair's control word names.  ksize: 0 (no median), 3 or 5.  thr: the stage's threshold epsilon^2 * w * hgt as float32 (the
 * CUDA variant compares with the same value as a double); thr < 0: no pair ever stops.  variant: TF_VARIANT_CPU or TF_VARIANT_CUDA
 * (the latter needs an even inner * outer and has no median).  p_is_zero: the stage starts from p == 0 (a level's first warp).
 * err_q: uint64 [B][inner * outer + 1], the exact error sums of the iterations a pair executed (an overshot iteration's too), 0
 * elsewhere; iters: int32 [B][2] = (inner iterations, outer iterations) executed.  lambda, theta, tau are the handle's.  A bad
 * argument is TF_ERR_INVALID_ARG before any GPU work. */
int tf_dbg_stage(tf_handle* h, const float* I1wx, const float* I1wy, const float* rho_c,
                 float* u1, float* u2, float* p11, float* p12, float* p21, float* p22,
                 int B, int w, int hgt, int inner, int outer, int ksize, float thr, int variant, int p_is_zero,
                 unsigned long long* err_q, int* iters);

#ifdef __cplusplus
}
#endif
#endif /* TEEFLOW_H */
