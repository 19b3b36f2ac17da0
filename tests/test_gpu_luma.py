"""The luma front door on the device -- luma_f64 and its three consumers: conditioning (k_cond_minmax, k_cond_norm), Otsu's histogram
and threshold (k_otsu_hist, k_otsu_thr; read through tf_dbg_luma_stats, which runs the launches tf_otsu_masks opens with) and the
float16 echo (k_echo_f16) -- against the order-explicit float64 reference of tests/luma_cases.py, on the corpus that module names: the
whole RGB cube as 256 frames and as one 4096 x 4096 frame, flat and one-pixel frames, grey ramps that fire hist_bin's two fix-up steps,
extremes planted where the min / max reduction could lose them, and sizes around a wave, a block and the echo's four-pixel step.
Everything is exact: bytes and bit patterns, no tolerance.  (tests/test_luma_cpu.py asserts what the corpus holds.)"""
import functools

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tests import luma_cases as LC

pytestmark = pytest.mark.gpu

GROUPS = ("flat", "one_lit", "ramps", "planted_131072", "planted_131073", "planted_262145", "sizes", "cube_frames", "cube_one_frame")
SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def _calls(group):
    """{call name: frames [N,H,W,3]} of one group of the corpus"""
    if group == "sizes":
        calls = {"sizes_" + k: v for k, v in LC.sizes_calls().items()}
        H, W = LC.SIZES_REVERSED
        calls[f"sizes_5x{H}x{W}_reversed"] = np.ascontiguousarray(calls[f"sizes_5x{H}x{W}"][::-1])
        return calls
    if group.startswith("planted_"):
        return {group: LC.planted_call(int(group.split("_")[1]))}
    return {group: getattr(LC, group)()}


@functools.lru_cache(maxsize=None)
def _ref(group):
    return {name: LC.reference(rgb) for name, rgb in _calls(group).items()}


def _luma_stats(eng, rgb):
    """tf_dbg_luma_stats -> (min / max as bit patterns uint64 [N,2], counts uint32 [N,256], thresholds float64 [N])"""
    rgb = np.ascontiguousarray(rgb)
    N, H, W, _ = rgb.shape
    mm, hist, thr = np.empty((N, 2), np.float64), np.empty((N, 256), np.uint32), np.empty(N, np.float64)
    _lib.check(eng._L.tf_dbg_luma_stats(eng._h, rgb.ctypes.data, N, H, W, mm.ctypes.data, hist.ctypes.data, thr.ctypes.data), eng._h, "tf_dbg_luma_stats")
    return mm.view(np.uint64), hist, thr


_stats_cache = {}


def _stats(eng, group):
    if group not in _stats_cache:
        _stats_cache[group] = {name: _luma_stats(eng, rgb) for name, rgb in _calls(group).items()}
    return _stats_cache[group]


def _reversed_pair(per_call):
    H, W = LC.SIZES_REVERSED
    return per_call[f"sizes_5x{H}x{W}"], per_call[f"sizes_5x{H}x{W}_reversed"]


def _where(got, want):
    bad = np.argwhere(got != want)
    return len(bad), bad[:6].tolist(), got[tuple(bad[:6].T)].tolist(), want[tuple(bad[:6].T)].tolist()


# ---- 1. conditioning ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_conditioning_equals_the_plain_order_reference(engine, group):
    got = {}
    for name, rgb in _calls(group).items():
        got[name] = engine.condition_frames(rgb)
        want = _ref(group)[name]["cond"]
        assert got[name].dtype == np.uint8 and got[name].shape == rgb.shape[:3]
        assert np.array_equal(got[name], want), (name,) + _where(got[name], want)
    if group == "flat":
        assert not got[group].any()                               # 0/0 and zero contrast
    if group == "sizes":
        a, b = _reversed_pair(got)
        assert np.array_equal(a[::-1], b)


# ---- 2. extremes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_extremes_equal_the_reference_bit_for_bit(engine, group):
    for name, (mm, hist, thr) in _stats(engine, group).items():
        want = _ref(group)[name]["minmax"].view(np.uint64)
        assert np.array_equal(mm, want), (name,) + _where(mm, want)
        one = mm[:, 0] == mm[:, 1]                                # a one-valued frame: no histogram, its value as the threshold
        assert not hist[one].any() and np.array_equal(thr[one].view(np.uint64), mm[one, 0])
        assert hist[~one].any(axis=1).all()
    if group == "flat":
        assert one.all()
    if group == "sizes":
        a, b = _reversed_pair(_stats(engine, group))
        assert all(np.array_equal(x[::-1], y) for x, y in zip(a, b))


# ---- 3. histogram -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_histogram_equals_np_histogram(engine, group):
    for name, (mm, hist, thr) in _stats(engine, group).items():
        want = _ref(group)[name]["hist"]
        assert np.array_equal(hist, want), (name,) + _where(hist.astype(np.int64), want)
        N, H, W = _calls(group)[name].shape[:3]
        some = mm[:, 0] != mm[:, 1]                               # (a one-valued frame has no histogram)
        assert (hist.sum(axis=1, dtype=np.int64)[some] == H * W).all()


# ---- 4. threshold -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_threshold_equals_threshold_otsu(engine, group):
    for name, (mm, hist, thr) in _stats(engine, group).items():
        want = _ref(group)[name]["thr"]
        assert np.array_equal(thr.view(np.uint64), want.view(np.uint64)), (name, thr.tolist()[:4], want.tolist()[:4])
        rgb = _calls(group)[name]
        if min(rgb.shape[:3]) >= 2:                               # tf_otsu_masks takes N, H, W >= 2
            _, thr_masks = engine.otsu_masks(rgb, 0, return_thresholds=True)
            assert np.array_equal(thr_masks.view(np.uint64), thr.view(np.uint64)), name


def test_threshold_of_a_two_valued_frame_is_the_centre_of_bin_0(engine):
    rgb = LC.two_valued()
    mm, hist, thr = _luma_stats(engine, rgb)
    assert thr.tolist() == [LC.TWO_VALUED_THRESHOLD] * 2
    assert hist[:, 0].tolist() == [48, 48] and hist[:, 255].tolist() == [16, 16] and not hist[:, 1:255].any()
    assert np.array_equal(engine.otsu_masks(rgb, 0, return_thresholds=True)[1], thr)
    assert np.array_equal(LC.threshold(rgb), thr)


# ---- 5. echo ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["cube_frames", "flat", "one_lit", "sizes"])
def test_echo_equals_the_luma_rounded_once(engine, group):
    for name, rgb in _calls(group).items():
        got = np.array(engine.echo_frames(rgb))
        want = _ref(group)[name]["echo"]
        assert got.dtype == np.float16 and got.shape == rgb.shape[:3]
        assert np.array_equal(got.view(np.uint16), want), (name,) + _where(got.view(np.uint16), want)


# ---- 6. the study calls condition the same way --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deepflow_engine():
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0, algo="deepflow")
    yield eng
    eng.close()


@pytest.mark.parametrize("held", [False, True], ids=["host", "held"])
@pytest.mark.parametrize("algo,H,W", [("TVL1", 41, 67), ("deepflow", 55, 123)])
def test_study_calls_condition_as_condition_frames_does(engine, deepflow_engine, algo, H, W, held):
    eng = engine if algo == "TVL1" else deepflow_engine
    rgb = LC.study(H, W)
    cond = LC.condition(rgb)
    assert not cond[1].any() and not cond[3].any() and cond[4].sum() == 255
    want = np.array(eng.calc_batch(cond))
    frames = eng.hold_frames(rgb) if held else rgb
    try:
        assert np.array_equal(eng.condition_frames(frames), cond)
        assert np.array_equal(np.array(eng.calc_study(frames)), want)
        assert np.array_equal(np.array(eng.wait(eng.submit_study(frames))), want)
        flow16, echo16 = eng.calc_study_payload(frames, pad_last=False)
        assert np.array_equal(np.array(echo16).view(np.uint16), LC.echo_bits(rgb))
        assert np.array_equal(np.array(flow16).view(np.uint16), want.astype(np.float16).view(np.uint16))
    finally:
        if held:
            eng.release_frames()
    assert np.isfinite(want).all() and want.any()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_the_hook_refuses_before_any_gpu_work(engine):
    L, h = engine._L, engine._h
    rgb = LC.sizes_calls()["5x1x257"]
    N, H, W, _ = rgb.shape
    mm, hist, thr = np.full((N, 2), SENTINEL, np.uint64), np.full((N, 256), SENTINEL, np.uint32), np.full(N, SENTINEL, np.uint64)
    names = ("frames_upload_bytes", "tail_upload_bytes", "study_download_bytes", "frames_held_reads", "queue_jobs", "queue_outstanding")
    before = [engine.counter(n) for n in names]
    p = (rgb.ctypes.data, mm.ctypes.data, hist.ctypes.data, thr.ctypes.data)
    bad = [(None, p[0], N, H, W, p[1], p[2], p[3]), (h, None, N, H, W, p[1], p[2], p[3]), (h, p[0], N, H, W, None, p[2], p[3]),
           (h, p[0], N, H, W, p[1], None, p[3]), (h, p[0], N, H, W, p[1], p[2], None),
           (h, p[0], 0, H, W, p[1], p[2], p[3]), (h, p[0], N, 0, W, p[1], p[2], p[3]), (h, p[0], N, H, 0, p[1], p[2], p[3]),
           (h, p[0], -1, H, W, p[1], p[2], p[3]), (h, p[0], N, -3, W, p[1], p[2], p[3]), (h, p[0], N, H, -257, p[1], p[2], p[3])]
    for args in bad:
        assert L.tf_dbg_luma_stats(*args) == _lib.TF_ERR_INVALID_ARG, args[2:5]
    assert L.tf_dbg_luma_stats(h, p[0], 65536, H, W, p[1], p[2], p[3]) == _lib.TF_ERR_UNSUPPORTED       # (frames are a grid dimension)
    assert L.tf_dbg_luma_stats(h, p[0], 1, 1 << 16, 1 << 15, p[1], p[2], p[3]) == _lib.TF_ERR_UNSUPPORTED   # 2^31 pixels
    assert (mm == SENTINEL).all() and (hist == SENTINEL).all() and (thr == SENTINEL).all()
    assert [engine.counter(n) for n in names] == before
    ref = LC.reference(rgb)
    got = _luma_stats(engine, rgb)
    assert np.array_equal(got[0], ref["minmax"].view(np.uint64)) and np.array_equal(got[1], ref["hist"])
    assert np.array_equal(got[2].view(np.uint64), ref["thr"].view(np.uint64))
    assert [engine.counter(n) for n in names] == before              # the hook uploads to buffers of its own: no study counter moves
    assert np.array_equal(engine.condition_frames(rgb), ref["cond"])
