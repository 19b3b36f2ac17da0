"""What the study entry points turn away, and how: the return code and the tf_last_error text of every refusal the nine solving
entries and the two tf_saliency_frames* entries make before any device work, through the C ABI directly; and the shapes and types
DenseFlow's ten study methods refuse and accept.

One engine, one 3-frame 16x24 study.  Every buffer handed in is real and large enough for the call as it was asked for (the frames
hold three channels whatever channel count is passed), so a refusal that turned into an acceptance would compute something harmless.
After each refusal a good calc_study on the same engine must return the bits it returned before: a refusal leaves the handle usable.
tf_last_error keeps its text until the next failure, so each case first leaves another failure's text there."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

pytestmark = pytest.mark.gpu

N, H, W = 3, 16, 24
SOLVING = ("tf_calc_seq_rgb", "tf_submit_seq_rgb", "tf_calc_seq_rgb_f16", "tf_submit_seq_rgb_f16", "tf_calc_seq_saliency",
           "tf_calc_seq_saliency_f32", "tf_calc_seq_saliency_f16", "tf_calc_seq_rgb_wase", "tf_calc_seq_saliency_wase")
MAPS = ("tf_saliency_frames", "tf_saliency_frames_f32")
WITH_CHANNELS = MAPS + ("tf_calc_seq_saliency", "tf_calc_seq_saliency_f32", "tf_calc_seq_saliency_f16", "tf_calc_seq_saliency_wase")
WITH_ECHO_AND_CHANNELS = ("tf_calc_seq_saliency_f16", "tf_calc_seq_saliency_wase")
WASE = ("tf_calc_seq_rgb_wase", "tf_calc_seq_saliency_wase")
SUBMIT = ("tf_submit_seq_rgb", "tf_submit_seq_rgb_f16")


@pytest.fixture(scope="module")
def study(engine):
    """the buffers of every call, and the flows a good calc_study returns before any refusal"""
    from tee_optical_flow_amd.synth import speckle_sequence
    rgb = np.ascontiguousarray(np.repeat(speckle_sequence(77, N, H, W)[..., None], 3, axis=3))
    mask = np.random.default_rng(5).random((N, H, W, 2)) < 0.4
    s = SimpleNamespace(rgb=rgb, mask=mask, mask_u8=np.ascontiguousarray(mask).view(np.uint8),
                        flow=np.zeros((N, H, W, 2), np.float32),              # room for N float32 flows, whatever the output type
                        echo=np.zeros((N, H, W), np.float16), maps=np.zeros((N, H, W), np.float32), bg=np.zeros(N, np.float32),
                        st=_lib.TfStats(), ticket=C.c_int(-1))
    s.before = np.array(engine.calc_study(rgb))
    rgb.setflags(write=False)
    s.before.setflags(write=False)
    return s


def _call(eng, s, name, n=N, ch=3, echo=False, n_frames=N, ticket=True):
    """entry point `name` on the study, with the given departures from a good call -> its return code"""
    L, h = eng._L, eng._h
    fr, fl, e = s.rgb.ctypes.data, s.flow.ctypes.data, s.echo.ctypes.data if echo else None
    st, t = C.byref(s.st), C.byref(s.ticket) if ticket else None
    wase = (s.mask_u8.ctypes.data, n_frames, 1.0, 0, fl, e, s.bg.ctypes.data, st)
    args = {"tf_calc_seq_rgb": (1.0, fl, st),
            "tf_submit_seq_rgb": (1.0, fl, t),
            "tf_calc_seq_rgb_f16": (1.0, fl, e, st),
            "tf_submit_seq_rgb_f16": (1.0, fl, e, t),
            "tf_saliency_frames": (ch, s.maps.ctypes.data),
            "tf_saliency_frames_f32": (ch, s.maps.ctypes.data),
            "tf_calc_seq_saliency": (ch, 1.0, fl, st),
            "tf_calc_seq_saliency_f32": (ch, 1.0, fl, st),
            "tf_calc_seq_saliency_f16": (ch, 1, 1.0, fl, e, st),
            "tf_calc_seq_rgb_wase": wase,
            "tf_calc_seq_saliency_wase": (ch, 1) + wase}[name]
    return getattr(L, name)(h, fr, n, H, W, *args)


def _refused(eng, s, name, code, fragment, **departure):
    L, h = eng._L, eng._h
    assert L.tf_set_tuning(h, b"no_such_knob", 0) == _lib.TF_ERR_INVALID_ARG
    assert b"unknown tuning knob" in L.tf_last_error(h)
    rc = _call(eng, s, name, **departure)
    msg = L.tf_last_error(h).decode()
    print(f"{name} {departure}: code {rc}, tf_last_error {msg!r}")
    assert rc == code, (name, departure, rc, msg)
    assert fragment in msg, (name, departure, msg)
    after = eng.calc_study(s.rgb)
    assert np.array_equal(after.view(np.uint32), s.before.view(np.uint32)), f"calc_study after the refusal of {name} {departure}"


@pytest.mark.parametrize("name", SOLVING)
def test_one_frame_is_no_sequence(engine, study, name):
    _refused(engine, study, name, _lib.TF_ERR_INVALID_ARG, "at least 2 frames", n=1)


@pytest.mark.parametrize("name", MAPS)
def test_saliency_frames_takes_one_frame(engine, study, name):
    assert _call(engine, study, name, n=1) == _lib.TF_OK
    ref = engine.saliency_frames(study.rgb[:1], np.float32 if name.endswith("f32") else np.uint8)
    got = study.maps.reshape(-1).view(ref.dtype)[:ref.size].reshape(ref.shape)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("name", WITH_CHANNELS)
def test_two_channels(engine, study, name):
    _refused(engine, study, name, _lib.TF_ERR_INVALID_ARG, "1 or 3 channels", ch=2)


@pytest.mark.parametrize("name", WITH_ECHO_AND_CHANNELS)
def test_echo_of_gray_frames(engine, study, name):
    _refused(engine, study, name, _lib.TF_ERR_INVALID_ARG, "echo needs RGB", ch=1, echo=True)


@pytest.mark.parametrize("name", WASE)
def test_wase_without_mask_frames(engine, study, name):
    _refused(engine, study, name, _lib.TF_ERR_INVALID_ARG, "bkgd mask", n_frames=0)


@pytest.mark.parametrize("name", SUBMIT)
def test_submit_without_ticket(engine, study, name):
    # (refused without a text of its own: tf_last_error keeps the one it had)
    _refused(engine, study, name, _lib.TF_ERR_INVALID_ARG, "unknown tuning knob", ticket=False)
    assert engine.counter("queue_outstanding") == 0


# ---- the Python layer: DenseFlow's ten study methods -----------------------------------------------------------------------------------
# name -> (takes the bkgd mask, what a good call returns: the flows' dtype, then the further members of the tuple)
METHODS = {"calc_study": (False, np.float32, ()),
           "calc_study_payload": (False, np.float16, ("echo",)),
           "calc_study_saliency": (False, np.float32, ()),
           "calc_study_saliency_payload": (False, np.float16, ("echo",)),
           "submit_study": (False, np.float32, ()),
           "submit_study_payload": (False, np.float16, ("echo",)),
           "calc_study_wase": (True, np.float32, ("bg",)),
           "calc_study_wase_payload": (True, np.float16, ("echo", "bg")),
           "calc_study_saliency_wase": (True, np.float32, ("bg",)),
           "calc_study_saliency_wase_payload": (True, np.float16, ("echo", "bg"))}


def _method(eng, s, name, frames, **kw):
    fn = getattr(eng, name)
    got = fn(frames, s.mask, **kw) if METHODS[name][0] else fn(frames, **kw)
    return eng.wait(got) if name.startswith("submit") else got


@pytest.mark.parametrize("name", METHODS)
def test_method_refuses(engine, study, name):
    outstanding = len(engine._jobs)
    for what, frames in (("[N,H,W]", study.rgb[..., 0]), ("[1,H,W,3]", study.rgb[:1]), ("float32", study.rgb.astype(np.float32)),
                         ("[N,H,W,2]", study.rgb[..., :2])):
        with pytest.raises(OpticalFlowCalculationError):
            _method(engine, study, name, frames)
            pytest.fail(f"{name} took {what} frames")
    assert len(engine._jobs) == outstanding
    assert np.array_equal(engine.calc_study(study.rgb).view(np.uint32), study.before.view(np.uint32))


@pytest.mark.parametrize("name", METHODS)
def test_method_accepts(engine, study, name):
    _, dtype, rest = METHODS[name]
    for pad in (False, True):
        got = _method(engine, study, name, study.rgb, pad_last=pad)
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == 1 + len(rest), (name, len(got))
        flows = got[0]
        assert flows.dtype == dtype and flows.shape == (N if pad else N - 1, H, W, 2)
        if pad:
            assert np.array_equal(flows[N - 1].view(np.uint8), flows[N - 2].view(np.uint8))
        for kind, a in zip(rest, got[1:]):
            assert (a.dtype, a.shape) == {"echo": (np.float16, (N, H, W)), "bg": (np.float32, (N - 1,))}[kind], (name, kind)
    if "echo" in rest:
        got = _method(engine, study, name, study.rgb, echo=False)
        assert got[1] is None and len(got) == 1 + len(rest)
    if name == "calc_study":
        assert np.array_equal(flows[:N - 1].view(np.uint32), study.before.view(np.uint32))


@pytest.mark.parametrize("name", METHODS)
def test_one_channel_frames(engine, study, name):
    """only calc_study_saliency takes [N,H,W,1]"""
    gray = np.ascontiguousarray(study.rgb[..., :1])
    if name == "calc_study_saliency":
        got = engine.calc_study_saliency(gray)
        assert got.dtype == np.float32 and got.shape == (N - 1, H, W, 2)
        # gray frames repeated to three channels have the same 8-bit gray, hence the same maps and flows
        assert np.array_equal(got.view(np.uint32), engine.calc_study_saliency(study.rgb).view(np.uint32))
    else:
        with pytest.raises(OpticalFlowCalculationError):
            _method(engine, study, name, gray)
