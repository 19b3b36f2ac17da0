"""ctypes binding of libteeflow_hip.so (include/teeflow.h).  There is no CPU fallback: if the HIP
library is missing or no gfx950 device is visible, every entry point raises."""
import ctypes as C
import os

from .exceptions import OpticalFlowCalculationError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TEEFLOW_LIB", os.path.join(_HERE, "libteeflow_hip.so"))   # override only for A/B experiments

TF_OK = 0
TF_ERR_INVALID_ARG = 1
TF_ERR_UNSUPPORTED = 2
ECHO_F16, ECHO_U8 = 0, 1     # TF_ECHO_*
COMM_ID_BYTES = 128          # TF_COMM_ID_BYTES
HELD_SLOTS = 12              # TF_HELD_SLOTS
HELD_SHAPE_LEN = 5 + 2 * HELD_SLOTS   # TF_HELD_SHAPE_LEN
FRAMES_FORMS = {"RGB": 0, "GRAY": 1, "YBR_FULL": 2}   # TF_FRAMES_*
RLE_STAGE_BYTES = 1024       # tf_rle_stage_bytes(): the bytes of a segment k_rle_decode stages at a time (rle::STAGE)
JPEGLL_SEGMENT_BYTES = 32    # tf_jpegll_segment_bytes(): the bytes of a piece of the split JPEG Lossless entropy decode (tfsync::SEG)
JPEGLL_SYNC_ROUNDS = 8       # the library's default of the tuning knob "jpegll_sync_rounds"
JPEG_STAGE_BYTES = 1024      # tf_jpeg_stage_bytes(): the bytes of a frame the k_jpeg_* kernels stage at a time (jpeg::STAGE)
JPEG_COLORS = {"none": 0, "libjpeg": 1}   # TF_JPEG_COLOR_*
PARAM_KEYS = {
    "tau": 0, "lambda": 1, "theta": 2, "nscales": 3, "warps": 4, "epsilon": 5, "inner_iterations": 6,
    "outer_iterations": 7, "scale_step": 8, "gamma": 9, "median_filtering": 10, "use_initial_flow": 11,
}

# every symbol include/teeflow.h declares (tests check that the built library exports all of them)
EXPORTED_SYMBOLS = [
    "tf_abi_version", "tf_device_count", "tf_default_params", "tf_create", "tf_destroy", "tf_set_param",
    "tf_get_param", "tf_set_stream", "tf_set_profile", "tf_calc_pair", "tf_calc_seq", "tf_calc_pairs", "tf_calc_pair_f32", "tf_calc_pairs_f32",
    "tf_calc_pairs_init", "tf_calc_pairs_init_device", "tf_chain_next", "tf_calc_pairs_device", "tf_calc_seq_device", "tf_submit_pairs_device", "tf_submit_seq_device", "tf_submit_pairs", "tf_submit_seq", "tf_submit_seq_rgb", "tf_wait", "tf_condition_frames", "tf_calc_seq_rgb", "tf_saliency_frames", "tf_saliency_frames_f32", "tf_calc_seq_saliency", "tf_calc_seq_saliency_f32", "tf_clean_masks", "tf_otsu_masks", "tf_segmentor_input", "tf_segmentor_classmap", "tf_av_centroids", "tf_first_region_areas", "tf_radlong_project", "tf_radlong_project_param", "tf_polar_project_param", "tf_radlong_hist", "tf_radlong_select", "tf_radlong_overlay", "tf_radlong_shape", "tf_get_iters", "tf_last_error",
    "tf_set_tuning", "tf_dbg_counter", "tf_default_deepflow_params", "tf_create_deepflow", "tf_dbg_df_refine", "tf_dbg_df_blur", "tf_dbg_launch_profile", "tf_dbg_strip_rule", "tf_wase_compensate", "tf_wase_compensate_device", "tf_host_alloc", "tf_host_free",
    "tf_dbg_pyramid", "tf_dbg_resize", "tf_dbg_warp", "tf_dbg_median", "tf_dbg_iterate", "tf_dbg_stage", "tf_dbg_df_pyramid", "tf_dbg_df_up",
    "tf_calc_seq_rgb_f16", "tf_submit_seq_rgb_f16", "tf_calc_seq_saliency_f16", "tf_echo_frames", "tf_dbg_f16_round", "tf_dbg_luma_stats",
    "tf_calc_seq_rgb_wase", "tf_calc_seq_saliency_wase",
    "tf_calc_chains", "tf_calc_chains_device", "tf_calc_chains_rgb", "tf_dbg_chain_order",
    "tf_hold_study", "tf_hold_mask", "tf_hold_next", "tf_calc_seq_rgb_held", "tf_held_shape", "tf_release_study", "tf_held_av_centroids", "tf_held_first_region_areas",
    "tf_held_radlong_project_param", "tf_held_polar_project_param", "tf_held_radlong_overlay",
    "tf_magnitude_overlay", "tf_held_magnitude_overlay",
    "tf_inflate", "tf_hold_study_chunks", "tf_hold_mask_chunks",
    "tf_deflate", "tf_deflate_array", "tf_held_deflate",
    "tf_hold_frames", "tf_held_frames_shape", "tf_release_frames", "tf_download_frames", "tf_frames_next",
    "tf_rle_decode", "tf_hold_frames_rle", "tf_rle_stage_bytes",
    "tf_jpeg_decode", "tf_hold_frames_jpeg", "tf_jpeg_stage_bytes",
    "tf_jpegll_decode", "tf_hold_frames_jpegll", "tf_jpegll_segment_bytes",
    "tf_comm_unique_id", "tf_comm_init_rank", "tf_comm_init_all", "tf_allgather_flows", "tf_allgather_flows_all", "tf_comm_wait", "tf_comm_destroy",
]


class TfParams(C.Structure):
    _fields_ = [("tau", C.c_double), ("lambda_", C.c_double), ("theta", C.c_double), ("epsilon", C.c_double),
                ("scale_step", C.c_double), ("gamma", C.c_double), ("nscales", C.c_int), ("warps", C.c_int),
                ("inner_iterations", C.c_int), ("outer_iterations", C.c_int), ("median_filtering", C.c_int),
                ("use_initial_flow", C.c_int), ("algo", C.c_int), ("max_batch", C.c_int), ("variant", C.c_int)]


class TfDeepflowParams(C.Structure):
    _fields_ = [("sigma", C.c_float), ("min_size", C.c_int), ("downscale_factor", C.c_float), ("fixed_point_iterations", C.c_int),
                ("sor_iterations", C.c_int), ("alpha", C.c_float), ("delta", C.c_float), ("gamma", C.c_float), ("omega", C.c_float),
                ("zeta", C.c_float), ("epsilon", C.c_float), ("max_batch", C.c_int)]


class TfStats(C.Structure):
    _fields_ = [("n_pairs", C.c_int), ("nscales_used", C.c_int), ("warps", C.c_int), ("reserved0", C.c_int),
                ("ms_total", C.c_double), ("ms_h2d", C.c_double), ("ms_device", C.c_double), ("ms_d2h", C.c_double),
                ("iter_launches", C.c_ulonglong), ("iter_pair_steps", C.c_ulonglong), ("iter_ms", C.c_double),
                ("iter_bytes", C.c_double), ("total_bytes", C.c_double), ("inner_iters_total", C.c_ulonglong),
                ("outer_iters_total", C.c_ulonglong), ("ms_warp", C.c_double), ("ms_median", C.c_double),
                ("ms_misc", C.c_double), ("ms_sched", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved0"}


HELD_FLOW, HELD_ECHO, HELD_MASK = 0, 1, 2      # tf_held_deflate's `what`


class TfChunked(C.Structure):
    """tf_chunked: one chunked dataset of a study file (include/teeflow.h)"""
    _fields_ = [("blob", C.c_void_p), ("off", C.c_void_p), ("len", C.c_void_p), ("raw", C.c_void_p), ("coord", C.c_void_p),
                ("n", C.c_int), ("ndim", C.c_int), ("shape", C.c_int64 * 4), ("chunk", C.c_int64 * 4), ("elem_bytes", C.c_int),
                ("chunk_bytes", C.c_uint32)]


_lib = None


def load():
    """Load the HIP library or fail loudly (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OpticalFlowCalculationError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C tee_optical_flow_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    # The CPU checker (oracle/libteeflow_cpu.so, test infrastructure) exports the same ABI.  It must never stand in for the
    # product: refuse anything that lives under an oracle/ directory or carries the checker's own entry points.
    real = os.path.realpath(LIB_PATH)
    if "oracle" in real.split(os.sep)[:-1]:
        raise OpticalFlowCalculationError(f"{LIB_PATH} resolves into an oracle/ directory: the CPU checker is test infrastructure, not a backend")
    L = C.CDLL(LIB_PATH)
    if hasattr(L, "orc_set_num_threads") or hasattr(L, "orc_tvl1_calc"):
        raise OpticalFlowCalculationError(f"{LIB_PATH} is the CPU checker library (it exports orc_* symbols): there is no CPU backend")
    vp, i32, f32, dbl = C.c_void_p, C.c_int, C.c_float, C.c_double
    L.tf_abi_version.restype = i32
    L.tf_device_count.restype = i32
    L.tf_default_params.argtypes = [C.POINTER(TfParams)]
    L.tf_create.argtypes = [C.POINTER(TfParams), i32, C.POINTER(vp)]
    L.tf_destroy.argtypes = [vp]
    L.tf_destroy.restype = None
    L.tf_set_param.argtypes = [vp, i32, dbl]
    L.tf_get_param.argtypes = [vp, i32, C.POINTER(dbl)]
    L.tf_set_stream.argtypes = [vp, vp, i32]
    L.tf_set_profile.argtypes = [vp, i32]
    L.tf_set_tuning.argtypes = [vp, C.c_char_p, i32]
    L.tf_dbg_counter.argtypes = [vp, C.c_char_p]
    L.tf_dbg_counter.restype = C.c_longlong
    L.tf_default_deepflow_params.argtypes = [C.POINTER(TfDeepflowParams)]
    L.tf_create_deepflow.argtypes = [C.POINTER(TfDeepflowParams), i32, C.POINTER(vp)]
    L.tf_dbg_df_refine.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    L.tf_dbg_df_blur.argtypes = [vp, vp, i32, i32, vp]
    L.tf_dbg_df_pyramid.argtypes = [vp, vp, i32, i32, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.tf_dbg_df_up.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, i32]
    L.tf_dbg_launch_profile.argtypes = [vp, vp, vp, vp, vp, i32]
    L.tf_dbg_strip_rule.argtypes = [i32, i32, i32, i32, vp, vp]
    L.tf_dbg_strip_rule.restype = None
    L.tf_host_alloc.argtypes = [C.c_size_t]
    L.tf_host_alloc.restype = vp
    L.tf_host_free.argtypes = [vp]
    L.tf_host_free.restype = None
    L.tf_wase_compensate.argtypes = [vp, vp, i32, vp, i32, i32, i32, C.c_float, vp]
    L.tf_wase_compensate_device.argtypes = [vp, vp, i32, vp, i32, i32, i32, C.c_float, vp]
    L.tf_calc_pair.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(TfStats)]
    L.tf_calc_seq.argtypes = [vp, vp, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_calc_pairs.argtypes = [vp, vp, vp, i32, i32, i32, vp, C.POINTER(TfStats)]
    L.tf_calc_pairs_f32.argtypes = [vp, vp, vp, i32, i32, i32, vp, C.POINTER(TfStats)]
    L.tf_calc_pair_f32.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(TfStats)]
    L.tf_calc_pairs_device.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_calc_seq_device.argtypes = [vp, vp, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_calc_pairs_init.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, vp, C.POINTER(TfStats)]
    L.tf_calc_pairs_init_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_submit_pairs_device.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, C.POINTER(i32)]
    L.tf_submit_seq_device.argtypes = [vp, vp, i32, i32, i32, f32, vp, C.POINTER(i32)]
    L.tf_submit_pairs.argtypes = [vp, vp, vp, i32, i32, i32, vp, C.POINTER(i32)]
    L.tf_submit_seq.argtypes = [vp, vp, i32, i32, i32, f32, vp, C.POINTER(i32)]
    L.tf_submit_seq_rgb.argtypes = [vp, vp, i32, i32, i32, f32, vp, C.POINTER(i32)]
    L.tf_wait.argtypes = [vp, i32, C.POINTER(TfStats)]
    L.tf_condition_frames.argtypes = [vp, vp, i32, i32, i32, vp]
    L.tf_saliency_frames.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.tf_calc_seq_saliency.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_saliency_frames_f32.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.tf_calc_seq_saliency_f32.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_clean_masks.argtypes = [vp, vp, i32, i32, i32, vp, i32, C.c_longlong, vp]
    L.tf_otsu_masks.argtypes = [vp, vp, i32, i32, i32, C.c_longlong, vp, vp]
    L.tf_segmentor_input.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]
    L.tf_segmentor_classmap.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
    L.tf_av_centroids.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    L.tf_first_region_areas.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.tf_radlong_project_param.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.tf_polar_project_param.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.tf_calc_seq_rgb.argtypes = [vp, vp, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_calc_seq_rgb_f16.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp, C.POINTER(TfStats)]
    L.tf_submit_seq_rgb_f16.argtypes = [vp, vp, i32, i32, i32, f32, vp, vp, C.POINTER(i32)]
    L.tf_calc_seq_saliency_f16.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, C.POINTER(TfStats)]
    L.tf_echo_frames.argtypes = [vp, vp, i32, i32, i32, vp]
    L.tf_calc_seq_rgb_wase.argtypes = [vp, vp, i32, i32, i32, vp, i32, f32, i32, vp, vp, vp, C.POINTER(TfStats)]
    L.tf_calc_seq_saliency_wase.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, f32, i32, vp, vp, vp, C.POINTER(TfStats)]
    L.tf_dbg_f16_round.argtypes = [vp, vp, C.c_size_t, f32, vp]
    L.tf_dbg_luma_stats.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    L.tf_radlong_project.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.tf_radlong_hist.argtypes = [vp, i32, vp, i32, vp]
    L.tf_radlong_select.argtypes = [vp, i32, vp, vp]
    L.tf_radlong_overlay.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.tf_radlong_shape.argtypes = [vp, C.POINTER(i32 * 3)]
    L.tf_magnitude_overlay.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, dbl, i32, i32, vp, i32, vp, vp, vp, vp]
    L.tf_hold_study.argtypes = [vp, vp, i32, i32, i32, vp, i32]
    L.tf_hold_mask.argtypes = [vp, i32, vp, i32, i32]
    L.tf_hold_next.argtypes = [vp, i32]
    L.tf_calc_seq_rgb_held.argtypes = [vp, vp, i32, i32, i32, f32, i32, C.POINTER(TfStats)]
    L.tf_chain_next.argtypes = [vp, i32]
    # (the per-chain pointers and frame counts: ctypes arrays of c_void_p / c_int)
    L.tf_calc_chains.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_calc_chains_device.argtypes = [vp, vp, vp, i32, i32, i32, f32, vp, C.POINTER(TfStats)]
    L.tf_calc_chains_rgb.argtypes = [vp, vp, vp, i32, i32, i32, f32, i32, vp, vp, C.POINTER(TfStats)]
    L.tf_dbg_chain_order.argtypes = [vp, i32, vp, vp]
    L.tf_held_shape.argtypes = [vp, C.POINTER(C.c_longlong * HELD_SHAPE_LEN)]
    L.tf_release_study.argtypes = [vp]
    L.tf_held_av_centroids.argtypes = [vp, i32, i32, vp, vp]
    L.tf_held_first_region_areas.argtypes = [vp, i32, i32, vp]
    L.tf_held_radlong_project_param.argtypes = [vp, i32, i32, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.tf_held_polar_project_param.argtypes = [vp, i32, i32, i32, dbl, i32, vp, vp, vp, vp, vp]
    L.tf_held_radlong_overlay.argtypes = [vp, vp, vp, vp, vp]
    L.tf_held_magnitude_overlay.argtypes = [vp, i32, i32, i32, dbl, i32, i32, vp, vp, vp, vp]
    L.tf_inflate.argtypes = [vp, vp, vp, vp, vp, i32, C.c_uint32, vp, vp]
    L.tf_deflate.argtypes = [vp, vp, i32, C.c_uint32, vp, C.c_uint64, vp, vp, vp]
    L.tf_deflate_array.argtypes = [vp, vp, i32, vp, vp, i32, i32, vp, C.c_uint64, vp, vp, vp, vp]
    L.tf_held_deflate.argtypes = [vp, i32, i32, vp, i32, vp, C.c_uint64, vp, vp, vp, vp]
    L.tf_hold_frames.argtypes = [vp, vp, i32, i32, i32, i32, i32]
    L.tf_held_frames_shape.argtypes = [vp, C.POINTER(C.c_longlong * 4)]
    L.tf_release_frames.argtypes = [vp]
    L.tf_download_frames.argtypes = [vp, vp]
    L.tf_frames_next.argtypes = [vp, i32, i32]
    L.tf_rle_decode.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.tf_hold_frames_rle.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.tf_rle_stage_bytes.restype = i32
    L.tf_jpeg_decode.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.tf_hold_frames_jpeg.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.tf_jpeg_stage_bytes.restype = i32
    L.tf_jpegll_segment_bytes.restype = i32
    L.tf_jpegll_decode.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.tf_hold_frames_jpegll.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    L.tf_hold_study_chunks.argtypes = [vp, C.POINTER(TfChunked), C.POINTER(TfChunked)]
    L.tf_hold_mask_chunks.argtypes = [vp, i32, C.POINTER(TfChunked)]
    L.tf_get_iters.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.tf_last_error.argtypes = [vp]
    L.tf_last_error.restype = C.c_char_p
    L.tf_dbg_pyramid.argtypes = [vp, vp, i32, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.tf_dbg_resize.argtypes = [vp, vp, i32, i32, vp, i32, i32, dbl, dbl, f32]
    L.tf_dbg_warp.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    L.tf_dbg_median.argtypes = [vp, vp, i32, i32, i32, vp]
    L.tf_dbg_iterate.argtypes = [vp] + [vp] * 9 + [i32, i32, i32, i32, vp]
    L.tf_dbg_stage.argtypes = [vp] + [vp] * 9 + [i32, i32, i32, i32, i32, i32, f32, i32, i32, vp, vp]
    L.tf_comm_unique_id.argtypes = [vp]
    L.tf_comm_init_rank.argtypes = [vp, i32, i32, vp]
    L.tf_comm_init_all.argtypes = [C.POINTER(vp), i32]
    L.tf_allgather_flows.argtypes = [vp, vp, C.c_size_t, vp, C.POINTER(i32)]
    L.tf_allgather_flows_all.argtypes = [C.POINTER(vp), i32, C.POINTER(vp), C.c_size_t, C.POINTER(vp)]
    L.tf_comm_wait.argtypes = [vp, i32]
    L.tf_comm_destroy.argtypes = [vp]
    for name in EXPORTED_SYMBOLS:
        getattr(L, name)  # AttributeError here = header/library mismatch
    if L.tf_abi_version() != 2:
        raise OpticalFlowCalculationError("libteeflow_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc, handle=None, what="teeflow"):
    if rc != TF_OK:
        msg = load().tf_last_error(handle)
        err = OpticalFlowCalculationError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
        err.code = rc
        raise err
