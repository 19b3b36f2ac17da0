"""Frames held on the device (tf_hold_frames, tf_frames_next & co.; DenseFlow.hold_frames and the HeldFrames token): what is held
against the numpy twin frames.ingest_host, and every call that takes frames, armed with the token, against the same call given the
twin's host RGB -- np.array_equal, no tolerance anywhere.  The yardstick is the host-pointer calls, which other tests pin; the held
path is never compared with itself.  Small studies (6 frames of 37 x 53 from flipped YBR, 7 of 40 x 56 from grey, 5 of 37 x 53 from
flipped RGB), sub-batches of 3 pairs so that a solve crosses sub-batches on the lanes.  The two cases that share device pointers or a
stream with torch run in one child process that imports torch first (tests/frames_cases.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests import frames_cases as FC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 0.04 * 50
FLOW_CHUNKS, ECHO_CHUNKS = (2, 10, 14, 1), (2, 19, 27)
STUDIES = [("YBR_FULL", True, 6, 37, 53), ("GRAY", False, 7, 40, 56), ("RGB", True, 5, 37, 53)]


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0, max_batch=3)
    yield e
    e.close()


@pytest.fixture(scope="module", params=STUDIES, ids=lambda s: f"{s[0]}{'-flip' if s[1] else ''}-{s[2]}x{s[3]}x{s[4]}")
def study(request):
    """(source as stored, form, flip, the twin's host RGB)"""
    form, flip, N, H, W = request.param
    src = FC.speckle_source(form, N, H, W)
    return src, form, flip, F.ingest_host(src, form, flip)


def _same(a, b, what):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(b)]
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
        return
    if a is None or b is None:
        assert a is None and b is None, what
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, int((a != b).sum()))


def _both(e, study, call, what):
    """call(frames) with the token of the held study and with the twin's host RGB: equal, the held frames read once and nothing uploaded"""
    src, form, flip, rgb = study
    tok = e.hold_frames(src, form, flip)
    up, reads = e.counter("frames_upload_bytes"), e.counter("frames_held_reads")
    got = call(tok)
    assert e.counter("frames_upload_bytes") == up and e.counter("frames_held_reads") > reads, what
    want = call(rgb)
    assert e.counter("frames_upload_bytes") > up, what
    _same(got, want, what)
    assert np.array_equal(e.download_frames(), rgb), what           # the call left the held frames as they were
    return got


# ---- what is held ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_held_frames_equal_the_twin(eng, shape):
    for form in FC.FORMS:
        for flip in (False, True):
            src = FC.source(form, *shape)
            before = eng.counter("frames_upload_bytes")
            tok = eng.hold_frames(src, form, flip)
            assert tok.shape == shape + (3,) and eng.counter("frames_upload_bytes") - before == src.nbytes
            assert np.array_equal(eng.download_frames(), F.ingest_host(src, form, flip)), (form, flip)
            kernel = not (form == "RGB" and not flip)                # plain RGB: the upload is the held frames, no kernel
            assert (eng.counter("ingest_bytes") == src.nbytes + 3 * int(np.prod(shape))) if kernel else eng.counter("ingest_bytes") == 0


def test_every_ybr_triple(eng):
    cube = FC.cube()
    eng.hold_frames(cube, "YBR_FULL")
    got = eng.download_frames()
    want = F.ybr_full_to_rgb(cube)
    print(f"k_ingest over the cube: {eng.counter('ingest_kernel_us')} us for {eng.counter('ingest_bytes')} bytes; "
          f"{int((got != want).any(-1).sum())} of 2^24 triples differ from the twin")
    assert np.array_equal(got, want)
    eng.release_frames()
    with pytest.raises(OpticalFlowCalculationError, match="no frames are held"):
        eng.download_frames()


# ---- every consumer, armed with the token, against the same call on the twin's host RGB -------------------------------------------------
def test_calc_study_payload(eng, study):
    flow, echo = _both(eng, study, lambda fr: eng.calc_study_payload(fr, SCALE), "calc_study_payload")
    assert flow.dtype == np.float16 and np.abs(flow.astype(np.float32)).max() > 0 and echo.shape == study[3].shape[:3]
    _both(eng, study, lambda fr: eng.calc_study(fr, SCALE, pad_last=True), "calc_study")


@pytest.mark.parametrize("map_dtype", ["f32", "u8"])
def test_calc_study_saliency_payload(eng, study, map_dtype):
    _both(eng, study, lambda fr: eng.calc_study_saliency_payload(fr, SCALE, map_dtype=map_dtype), f"saliency payload {map_dtype}")


def test_calc_study_wase_payload(eng, study):
    N, H, W = study[3].shape[:3]
    bkgd = np.random.default_rng(5).random((2, H, W, 2)) < 0.3
    _both(eng, study, lambda fr: eng.calc_study_wase_payload(fr, bkgd, SCALE), "calc_study_wase_payload")


def test_submit_study_payload_and_frames_replaced_right_after(eng, study):
    src, form, flip, rgb = study
    want = eng.calc_study_payload(rgb, SCALE)
    tok = eng.hold_frames(src, form, flip)
    ticket = eng.submit_study_payload(tok, SCALE)
    other = eng.hold_frames(np.full_like(rgb, 255), "RGB")               # the job conditioned its frames at submit: these are not its
    _same(eng.wait(ticket), want, "submitted from the token, frames replaced before the wait")
    with pytest.raises(OpticalFlowCalculationError, match="stale"):
        eng.submit_study_payload(tok, SCALE)
    assert np.array_equal(eng.download_frames(), np.full_like(rgb, 255)) and other.generation > tok.generation


def test_chained_study(study):
    e = T.DenseFlow(device_id=0, max_batch=3)
    try:
        e.setUseInitialFlow(True)
        _both(e, study, lambda fr: e.calc_study_payload(fr, SCALE, chain=True), "chained study")
        assert e.counter("chain_steps") > 0
    finally:
        e.close()


def test_calc_study_held_and_study_chunks(eng, study):
    def held(fr):
        eng.calc_study_held(fr, SCALE)
        return eng.held, eng.held_deflate("flow", FLOW_CHUNKS), eng.held_deflate("echo", ECHO_CHUNKS)
    (_, *a), (_, *b) = _both_raw(eng, study, held)
    _same(a, b, "calc_study_held")
    _both(eng, study, lambda fr: eng.study_chunks(fr, SCALE, FLOW_CHUNKS, ECHO_CHUNKS), "study_chunks")


def _both_raw(e, study, call):
    src, form, flip, rgb = study
    return call(e.hold_frames(src, form, flip)), call(rgb)


def test_deepflow_handle(study):
    e = T.createOptFlow_DeepFlow(max_batch=3)
    try:
        _both(e, study, lambda fr: e.calc_study_payload(fr, SCALE), "DeepFlow calc_study_payload")
    finally:
        e.close()


def test_otsu_masks_with_thresholds(eng, study):
    masks, thr = _both(eng, study, lambda fr: eng.otsu_masks(fr, 20, return_thresholds=True), "otsu_masks")
    assert masks.any() and not masks.all() and thr.shape == (study[3].shape[0],)


def test_echo_condition_and_saliency_frames(eng, study):
    _both(eng, study, eng.echo_frames, "echo_frames")
    _both(eng, study, eng.condition_frames, "condition_frames")
    for dt in (np.float32, np.uint8):
        _both(eng, study, lambda fr: eng.saliency_frames(fr, dt), f"saliency_frames {dt.__name__}")
    src, form, flip, rgb = study
    tok = eng.hold_frames(src, form, flip)
    _same(eng.echo_frames(tok[1:4]), eng.echo_frames(rgb[1:4]), "echo_frames of a frame range")
    _same(eng.condition_frames(tok[2:]), eng.condition_frames(rgb[2:]), "condition_frames of a frame range")


def test_one_upload_per_study(eng, study):
    """masks and solve from the token: the study's bytes cross the bus once, as stored; from host RGB, once per call"""
    src, form, flip, rgb = study
    c0 = eng.counter("frames_upload_bytes")
    tok = eng.hold_frames(src, form, flip)
    eng.otsu_masks(tok, 20)
    eng.calc_study_payload(tok, SCALE)
    eng.echo_frames(tok)
    c1 = eng.counter("frames_upload_bytes")
    assert c1 - c0 == src.nbytes
    eng.otsu_masks(rgb, 20)
    eng.calc_study_payload(rgb, SCALE)
    eng.echo_frames(rgb)
    assert eng.counter("frames_upload_bytes") - c1 == 3 * rgb.nbytes


def test_held_frames_and_a_held_study_coexist(eng, study):
    src, form, flip, rgb = study
    tok = eng.hold_frames(src, form, flip)
    flow, echo = eng.calc_study_payload(tok, SCALE, hold=True)
    held = eng.held
    assert held is not None and (held.N, held.H, held.W) == rgb.shape[:3]
    rec = eng.held_deflate("flow", FLOW_CHUNKS)
    assert np.array_equal(eng.download_frames(), rgb)                    # the study call left the frames
    eng.hold_frames(src, form, not flip)                                 # ... and new frames leave the study
    assert eng.held == held
    _same(eng.held_deflate("flow", FLOW_CHUNKS), rec, "the held study after the frames were replaced")
    eng.release_frames()
    assert eng.held == held
    eng.release_study()
    tok = eng.hold_frames(src, form, flip)
    _same(eng.calc_study_payload(tok, SCALE), (flow, echo), "after both were released")


# ---- the refusals: each leaves the flag spent and the held frames as they were ---------------------------------------------------------
def _armed_echo(e, first, count, ptr, N, H, W):
    """tf_frames_next(first, count), then tf_echo_frames with the given pointer and sizes -> (code, message, the output untouched?)"""
    out = np.full((max(N, 1), H, W), 7, np.uint16)
    assert e._L.tf_frames_next(e._h, first, count) == _lib.TF_OK
    rc = e._L.tf_echo_frames(e._h, ptr, N, H, W, out.ctypes.data)
    return rc, e._L.tf_last_error(e._h).decode(), bool((out == 7).all())


def test_refusals(eng, study):
    src, form, flip, rgb = study
    N, H, W = rgb.shape[:3]
    tok = eng.hold_frames(src, form, flip)
    spent = lambda: eng._L.tf_echo_frames(eng._h, None, N, H, W, np.empty((N, H, W), np.uint16).ctypes.data) == _lib.TF_ERR_INVALID_ARG
    for what, args, text in (
            ("frame count", (0, N, None, N - 1, H, W), f"{N - 1} x {H} x {W} x 3.*{N} x {H} x {W} x 3"),
            ("frame size", (0, N, None, N, W, H), f"{N} x {W} x {H} x 3.*{N} x {H} x {W} x 3"),
            ("range past the end", (2, N - 1, None, N - 1, H, W), rf"\[2, 2 \+ {N - 1}\), outside the {N} held"),
            ("negative start", (-1, 2, None, 2, H, W), "outside"),
            ("empty range", (0, 0, None, 0, H, W), "outside"),
            ("a host pointer too", (0, N, rgb.ctypes.data, N, H, W), "null frame pointer")):
        rc, msg, untouched = _armed_echo(eng, *args)
        assert rc == _lib.TF_ERR_INVALID_ARG and untouched, (what, rc, msg)
        import re
        assert re.search(text, msg), (what, msg)
        assert spent(), what                                             # the flag went with the refused call: this one is not armed
        assert np.array_equal(eng.download_frames(), rgb), what
    # a saliency call with one channel cannot read the three-channel held frames
    assert eng._L.tf_frames_next(eng._h, 0, N) == _lib.TF_OK
    out = np.empty((N, H, W), np.uint8)
    assert eng._L.tf_saliency_frames(eng._h, None, N, H, W, 1, out.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert f"{N} x {H} x {W} x 1" in eng._L.tf_last_error(eng._h).decode() and spent()
    # an armed lock-step call
    assert eng._L.tf_frames_next(eng._h, 0, N) == _lib.TF_OK
    with pytest.raises(OpticalFlowCalculationError, match="tf_frames_next was armed: chains in lock-step") as ei:
        eng.calc_study_chains([rgb, rgb], SCALE)
    assert ei.value.code == _lib.TF_ERR_UNSUPPORTED and spent()
    assert np.array_equal(eng.download_frames(), rgb)
    _same(eng.echo_frames(tok), eng.echo_frames(rgb), "the token after the refusals")
    # a stale token, in Python, before anything is armed
    tok2 = eng.hold_frames(src, form, flip)
    for call in (eng.echo_frames, lambda t: eng.calc_study_payload(t, SCALE), lambda t: eng.otsu_masks(t, 20), lambda t: eng.echo_frames(t[1:3])):
        with pytest.raises(OpticalFlowCalculationError, match="stale"):
            call(tok)
    assert spent() and np.array_equal(eng.download_frames(), rgb)
    with pytest.raises(OpticalFlowCalculationError, match="at least 2 frames"):
        eng.calc_study_payload(tok2[1:2], SCALE)
    # nothing held
    eng.release_frames()
    rc, msg, untouched = _armed_echo(eng, 0, N, None, N, H, W)
    assert rc == _lib.TF_ERR_INVALID_ARG and "no frames are held" in msg and untouched and spent()
    with pytest.raises(OpticalFlowCalculationError, match="stale.*no frames"):
        eng.echo_frames(tok2)
    other = T.DenseFlow(device_id=0, max_batch=3)
    try:
        with pytest.raises(OpticalFlowCalculationError, match="another engine"):
            other.echo_frames(eng.hold_frames(src, form, flip))
    finally:
        other.close()
    with pytest.raises(OpticalFlowCalculationError, match="form must be one of"):
        eng.hold_frames(src, "YBR_PARTIAL_420")
    with pytest.raises(OpticalFlowCalculationError):
        eng.hold_frames(rgb[..., :2], "RGB")


# ---- with torch in the process: segmentor_input over token[a:b] chunks, and everything on a caller's stream ------------------------------
@pytest.fixture(scope="module")
def torch_results():
    r = subprocess.run([sys.executable, "-m", "tests.frames_cases"], cwd=ROOT, capture_output=True, text=True,
                       env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", FC.TORCH_CASES)
def test_torch_case(torch_results, name):
    seconds, outcome = torch_results[name]
    print(f"{name}: {seconds} s in the child process")
    assert outcome == "ok", outcome
    assert seconds < 10.0
