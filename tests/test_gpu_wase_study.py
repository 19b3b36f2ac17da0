"""A bkgd_comp="WASE" study in one device call (tf_calc_seq_rgb_wase, tf_calc_seq_saliency_wase; DenseFlow.calc_study_wase & co.).

The yardstick is numpy on the engine's own unscaled float32 flows F = calc_study(rgb) (calc_study_saliency for the saliency forms),
which the oracle tests pin:
    bg[p]  = np.mean(m[m != 0]),  m = F[p] * mask
    ref32  = (F[p] - bg[p]) * np.float32(scale)
    ref16  = ref32.astype(np.float16)
Every comparison is of bits (uint32 / uint16 views); the repository's own WASE path is not consulted.  Only the empty selection, whose
NaNs carry the FPU's sign and payload, is compared by NaN position."""
import ctypes as C
import logging
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALES = (1.0, 2.0, 0.1)                                         # at 0.1 a fused multiply-convert differs from two roundings


def _frames(N, H, W):
    from tee_optical_flow_amd.synth import speckle_sequence
    return np.ascontiguousarray(np.repeat(speckle_sequence(N * 1000 + H + W, N, H, W)[..., None], 3, axis=3))


def _mask(n, H, W, density=0.4):
    m = np.random.default_rng([n, H, W]).random((n, H, W, 2)) < density
    m[0] = False
    return m


def _numpy(F, mask, scale):
    """(ref32 [P,H,W,2], bg [P]) -- finite, or the case is not one for a comparison of bits"""
    bg = np.empty(F.shape[0], np.float32)
    ref = np.empty_like(F)
    for p in range(F.shape[0]):
        m = F[p] * mask
        bg[p] = np.mean(m[m != 0])
        ref[p] = (F[p] - bg[p]) * np.float32(scale)
    assert bg.dtype == np.float32 and ref.dtype == np.float32 and np.isfinite(bg).all() and np.isfinite(ref).all()
    return ref, bg


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    g, r = got.view(u).reshape(-1), ref.view(u).reshape(-1)
    if not np.array_equal(g, r):
        bad = np.flatnonzero(g != r)
        raise AssertionError(f"{what}: {bad.size} of {g.size} values differ, first at {bad[0]}: device {got.reshape(-1)[bad[0]]!r} "
                             f"({g[bad[0]]:#x}), numpy {ref.reshape(-1)[bad[0]]!r} ({r[bad[0]]:#x})")


def _padded(a):
    return np.concatenate([a, a[-1:]])


_cases = {}


def _case(engine, N, H, W, n_mask=None):
    """frames, mask and the engine's unscaled flows of one size: made once, shared, never written"""
    key = (N, H, W, n_mask)
    if key not in _cases:
        rgb = _frames(N, H, W)
        F = np.array(engine.calc_study(rgb))
        for a in (rgb, F):
            a.setflags(write=False)
        _cases[key] = (rgb, _mask(n_mask or N, H, W), F)
    return _cases[key]


def _check_both_types(eng, rgb, mask, F, scale, what, saliency=None, pads=(False, True)):
    """float32 and float16 forms against numpy, backgrounds and (float16 form) the echo included"""
    ref32, bg = _numpy(F, mask, scale)
    ref16 = ref32.astype(np.float16)
    kw = {} if saliency is None else {"map_dtype": saliency}
    f32 = eng.calc_study_wase if saliency is None else eng.calc_study_saliency_wase
    f16 = eng.calc_study_wase_payload if saliency is None else eng.calc_study_saliency_wase_payload
    for pad in pads:
        out, b = f32(rgb, mask, scale=scale, pad_last=pad, **kw)
        _same_bits(b, bg, f"{what} float32 pad_last={pad}: backgrounds")
        _same_bits(out, _padded(ref32) if pad else ref32, f"{what} float32 pad_last={pad}: flows")
        out16, e16, b = f16(rgb, mask, scale=scale, pad_last=pad, echo=pad, **kw)
        _same_bits(b, bg, f"{what} float16 pad_last={pad}: backgrounds")
        _same_bits(out16, _padded(ref16) if pad else ref16, f"{what} float16 pad_last={pad}: flows")
        if pad:
            _same_bits(e16, eng.echo_frames(rgb), f"{what}: echo")
        else:
            assert e16 is None
    return ref32, bg


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", [(6, 33, 47), (5, 40, 64)])
def test_both_output_types_equal_numpy_dualtvl1(engine, shape, scale):
    """(6,33,47): an odd width, so the rows of the half store alternate in 4-byte parity, and 2HW = 3102, so the second compaction chunk
    of 2048 is partial; (5,40,64): whole chunks, even rows."""
    rgb, mask, F = _case(engine, *shape)
    _check_both_types(engine, rgb, mask, F, scale, f"{shape} x {scale}:")


def test_sub_batches_on_the_lanes_equal_numpy_and_the_default_engine(engine):
    """max_batch=4 and 10 frames: 9 pairs in three sub-batches, taken by the lanes, written into the one resident flow buffer"""
    import tee_optical_flow_amd as T
    rgb, mask, F = _case(engine, 10, 24, 40)
    small = T.DenseFlow(max_batch=4)
    try:
        ref32, bg = _check_both_types(small, rgb, mask, F, 2.0, "max_batch=4:", pads=(True,))
    finally:
        small.close()
    out, b = engine.calc_study_wase(rgb, mask, scale=2.0)
    _same_bits(out, ref32, "default engine: flows")
    _same_bits(b, bg, "default engine: backgrounds")


def test_deepflow_both_output_types():
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(algo="deepflow")
    try:
        rgb, mask = _frames(5, 48, 64), _mask(5, 48, 64)
        F = np.array(eng.calc_study(rgb))
        _check_both_types(eng, rgb, mask, F, 0.1, "deepflow:", pads=(True,))
    finally:
        eng.close()


@pytest.mark.parametrize("map_dtype", ["f32", "u8"])
def test_saliency_forms(engine, map_dtype):
    rgb, mask = _frames(5, 40, 64), _mask(5, 40, 64)
    F = np.array(engine.calc_study_saliency(rgb, map_dtype=map_dtype))
    _check_both_types(engine, rgb, mask, F, 2.0, f"saliency {map_dtype}:", saliency=map_dtype, pads=(True,))


def test_mask_of_two_frames_for_a_study_of_six(engine):
    rgb, mask, F = _case(engine, 6, 33, 47, n_mask=2)
    assert mask.shape[0] == 2 and mask[1].any()
    _check_both_types(engine, rgb, mask, F, 2.0, "2 mask frames:", pads=(False,))


def test_empty_selection_is_nan_everywhere_and_the_engine_goes_on(engine):
    """np.mean of an empty selection is NaN, and so is every value minus it; sign and payload of those NaNs are the FPU's, so this one
    case is compared by NaN position (the convention of test_gpu_wase.py)."""
    rgb, mask, F = _case(engine, 5, 40, 64)
    empty = np.zeros_like(mask)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        m = F[0] * empty
        assert np.isnan(np.mean(m[m != 0]))                      # what numpy says of it
    out, bg = engine.calc_study_wase(rgb, empty, scale=2.0)
    assert out.dtype == np.float32 and out.shape == F.shape and np.isnan(bg).all() and np.isnan(out).all()
    out16, e16, bg = engine.calc_study_wase_payload(rgb, empty, scale=2.0, pad_last=False, echo=False)
    assert out16.dtype == np.float16 and out16.shape == F.shape and e16 is None and np.isnan(bg).all() and np.isnan(out16).all()
    _check_both_types(engine, rgb, mask, F, 2.0, "after the empty selection:", pads=(True,))


def test_back_to_back_sizes_on_one_engine():
    """(6,48,64) then (4,24,40): the grow-only slots first grow, then are used only in part"""
    import tee_optical_flow_amd as T
    eng = T.DenseFlow()
    try:
        for shape in [(6, 48, 64), (4, 24, 40)]:
            rgb, mask = _frames(*shape), _mask(*shape)
            F = np.array(eng.calc_study(rgb))
            _check_both_types(eng, rgb, mask, F, 0.1, f"{shape}:", pads=(True,))
    finally:
        eng.close()


def test_refused_calls_leave_the_engine_usable(engine):
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
    L = _lib.load()
    rgb, mask, F = _case(engine, 5, 40, 64)
    N, H, W = rgb.shape[:3]
    bad_masks = {"mask height": mask[:, :-1], "mask width": mask[:, :, :-1], "uint8 mask": mask.view(np.uint8), "float mask": mask.astype(np.float32),
                 "one component": mask[..., :1]}
    for name, bad in bad_masks.items():
        for call in (engine.calc_study_wase, engine.calc_study_wase_payload, engine.calc_study_saliency_wase, engine.calc_study_saliency_wase_payload):
            with pytest.raises(OpticalFlowCalculationError, match="bkgd mask"):
                call(rgb, bad)
    for call in (engine.calc_study_wase, engine.calc_study_wase_payload):
        with pytest.raises(OpticalFlowCalculationError):
            call(rgb[:1], mask)                                                   # N = 1
    _check_both_types(engine, rgb, mask, F, 2.0, "after the refused Python calls:", pads=(False,))
    # the raw binding: each refused call returns its error, writes nothing, and the next call is right
    m8 = mask.view(np.uint8)
    out = np.full(F.shape, 7.0, np.float32)
    bg = np.full(N - 1, 5.0, np.float32)
    st = _lib.TfStats()
    o, b, r, m = out.ctypes.data, bg.ctypes.data, rgb.ctypes.data, m8.ctypes.data
    raw = {"null output": (r, N, H, W, m, N, 1.0, 0, None, None, b), "null frames": (None, N, H, W, m, N, 1.0, 0, o, None, b),
           "null mask": (r, N, H, W, None, N, 1.0, 0, o, None, b), "N = 1": (r, 1, H, W, m, N, 1.0, 0, o, None, b),
           "n_frames = 0": (r, N, H, W, m, 0, 1.0, 0, o, None, b), "H = 0": (r, N, 0, W, m, N, 1.0, 0, o, None, b),
           "null output, float16": (r, N, H, W, m, N, 1.0, 1, None, None, b)}
    for name, a in raw.items():
        assert L.tf_calc_seq_rgb_wase(engine._h, *a, C.byref(st)) == _lib.TF_ERR_INVALID_ARG, name
        assert L.tf_last_error(engine._h), name
        assert L.tf_calc_seq_saliency_wase(engine._h, *a[:4], 3, 1, *a[4:], C.byref(st)) == _lib.TF_ERR_INVALID_ARG, name
        assert (out == 7.0).all() and (bg == 5.0).all(), name
    e16 = np.zeros((N, H, W), np.float16)
    assert L.tf_calc_seq_saliency_wase(engine._h, rgb[..., 0].copy().ctypes.data, N, H, W, 1, 1, m, N, 1.0, 0, o, e16.ctypes.data, b,
                                       C.byref(st)) == _lib.TF_ERR_INVALID_ARG                   # an echo of gray frames
    assert (out == 7.0).all() and not e16.any()
    assert L.tf_calc_seq_rgb_wase(engine._h, r, N, H, W, m, N, 2.0, 0, o, None, None, C.byref(st)) == _lib.TF_OK      # no backgrounds asked for
    _same_bits(out, _numpy(F, mask, 2.0)[0], "raw binding, background_out NULL")
    assert (bg == 5.0).all()
    _check_both_types(engine, rgb, mask, F, 0.1, "after the refused raw calls:", pads=(True,))


def test_process_video_device_payload_with_wase(engine, caplog):
    """payload="device" with bkgd_comp="WASE" and a DenseFlow model: the file's float16 flows from the engine, no fallback message;
    payload="host" takes the one-call float32 form and equals numpy with the last flow repeated."""
    from tee_optical_flow_amd import pipeline
    rgb, mask, F = _case(engine, 6, 33, 47)
    md = {"pixel_spacing": 0.04, "frame_rate": 50.0, "R_wave_data_present": False, "R_times": None}
    kw = dict(verbose=False, mode="RVIO_2class", bkgd_comp="WASE", no_saliency=True, nparr=rgb, metadata=md, mask_dict={"bkgd": mask},
              flow_model=engine)
    pipeline._payload_fallbacks.clear()
    with caplog.at_level(logging.WARNING, logger=pipeline.logger.name):
        dev = pipeline.process_video(None, None, None, payload="device", **kw)
    host = pipeline.process_video(None, None, None, payload="host", **kw)
    assert not [r for r in caplog.records if "payload='device' not used" in r.getMessage()]
    assert not pipeline._payload_fallbacks
    ref32 = _padded(_numpy(F, mask, 0.04 * 50.0)[0])
    _same_bits(host, ref32, "payload='host'")
    assert dev.dtype == np.float16
    _same_bits(dev, host.astype(np.float16), "payload='device' vs the host path's cast")
