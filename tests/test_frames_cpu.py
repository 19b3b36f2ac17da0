"""Frame preparation's numpy twins (frames.ybr_full_to_rgb, frames.ingest_host), the ingest core under the sanitizers
(tests/csrc/verify_ingest.cpp over csrc/teeflow_ingest_core.h) and the HeldFrames token's rules, without a GPU.

The YBR conversion is defined by the twin's float32 chain; over all 2^24 triples this file records how other evaluations of the same
equations differ from it (each by at most one count):
  * multiply, add, add in float32 without fusion: 42 triples (asserted: numpy's elementwise arithmetic does not depend on a BLAS);
  * float64, multiply, add, add, with the float32 coefficients: 8913 triples (asserted likewise);
  * np.matmul in float32: 0 where the host's BLAS fuses (asserted where it is 0, printed otherwise: a BLAS without FMA may differ);
  * np.matmul in float64 with the float64 coefficients: BLAS-dependent, printed (8294 where this was written; 8252 against the unfused
    float32 order)."""
import os
import subprocess

import numpy as np
import pytest

from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.dense_flow import HeldFrames
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
from tee_optical_flow_amd.pipeline import _prep_frames

from tests import frames_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cube():
    return FC.cube()


@pytest.fixture(scope="module")
def cube_rgb(cube):
    return F.ybr_full_to_rgb(cube)


def _differing(a, b):
    return int((a != b).any(-1).sum()), int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


def test_grey_input_stays_grey_and_both_clamps_are_hit(cube, cube_rgb):
    grey = (cube[..., 1] == 128) & (cube[..., 2] == 128)
    assert grey.sum() == 256
    assert (cube_rgb[grey] == cube[grey][:, :1]).all()                      # R = G = B = Y
    x = cube.astype(np.float64)
    r = x[..., 0] + 1.402 * (x[..., 2] - 128)
    assert (cube_rgb[..., 0][r < -1] == 0).all() and (r < -1).sum() > 0     # clamped below
    assert (cube_rgb[..., 0][r > 256] == 255).all() and (r > 256).sum() > 0   # ... and above
    assert cube_rgb.min() == 0 and cube_rgb.max() == 255


def test_other_orders_of_the_same_equations_are_recorded(cube, cube_rgb):
    assert _differing(cube_rgb, F.ybr_full_to_rgb_unfused(cube)) == (42, 1)
    assert _differing(cube_rgb, F.ybr_full_to_rgb_f64(cube)) == (8913, 1)
    n, worst = _differing(cube_rgb, F.ybr_full_to_rgb_matmul(cube))
    print(f"np.matmul in float32 differs from the twin at {n} of 2^24 triples (largest difference {worst})")
    if n:
        print("  this host's BLAS does not fuse the way the device does: allowed, the twin is the definition")
    assert worst <= 1
    x = F._ybr_inputs(cube).astype(np.float64)
    f64 = np.clip(np.floor(np.matmul(x, F.YBR_TO_RGB) + 0.5), 0, 255).astype(np.uint8)
    print(f"np.matmul in float64 with float64 coefficients differs from the twin at {_differing(cube_rgb, f64)[0]} triples, from the "
          f"unfused float32 order at {_differing(F.ybr_full_to_rgb_unfused(cube), f64)[0]}")
    assert _differing(cube_rgb, f64)[1] <= 1


@pytest.mark.parametrize("flip", [False, True])
def test_ingest_host_equals_prep_frames_for_rgb_and_grey(flip):
    for N, H, W in FC.SHAPES:
        rgb, grey = FC.source("RGB", N, H, W), FC.source("GRAY", N, H, W)
        assert np.array_equal(F.ingest_host(rgb, "RGB", flip), _prep_frames(rgb, flip))
        if N > 1:                                                          # (_prep_frames leaves a one-frame grey stack as it is)
            assert np.array_equal(F.ingest_host(grey, "GRAY", flip), _prep_frames(grey, flip))
        ybr = FC.source("YBR_FULL", N, H, W)
        got = F.ingest_host(ybr, "YBR_FULL", flip)
        assert np.array_equal(got, _prep_frames(F.ybr_full_to_rgb(ybr), flip)) and got.flags.c_contiguous and got.dtype == np.uint8


def test_ingest_host_refuses_what_is_no_such_form():
    for arr, form in ((np.zeros((2, 3, 4), np.uint8), "RGB"), (np.zeros((2, 3, 4, 3), np.uint8), "GRAY"), (np.zeros((2, 3, 4, 2), np.uint8), "YBR_FULL"),
                      (np.zeros((2, 3, 4, 3), np.float32), "RGB"), (np.zeros((2, 3, 4, 3), np.uint8), "YBR_PARTIAL_420")):
        with pytest.raises(ValueError):
            F.ingest_host(arr, form)


# ---- the core, lane by lane, under the sanitizers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verify_ingest(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ingest") / "verify_ingest"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_ingest.cpp"), "-o", str(exe)])
    return str(exe)


def _run_core(exe, tmp_path, src, form, flip):
    N, H, W = src.shape[:3]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    src.tofile(fin)
    r = subprocess.run([exe, str(fin), str(fout), str(FC.FORMS.index(form)), str(int(flip)), str(N), str(H), str(W)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    return np.fromfile(fout, np.uint8).reshape(N, H, W, 3)


def test_core_converts_the_cube_under_the_sanitizers(verify_ingest, tmp_path, cube, cube_rgb):
    assert np.array_equal(_run_core(verify_ingest, tmp_path, cube, "YBR_FULL", False), cube_rgb)


@pytest.mark.parametrize("shape", FC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_core_stays_inside_exact_size_buffers(verify_ingest, tmp_path, shape):
    for form in FC.FORMS:
        for flip in (False, True):
            src = FC.source(form, *shape)
            assert np.array_equal(_run_core(verify_ingest, tmp_path, src, form, flip), F.ingest_host(src, form, flip)), (form, flip)


# ---- the token ------------------------------------------------------------------------------------------------------------------------
def test_token_ranges_and_refusals():
    e = FC.NumpyFrames()
    src = FC.source("YBR_FULL", 7, 5, 6)
    tok = e.hold_frames(src, "YBR_FULL", flip=True)
    want = F.ingest_host(src, "YBR_FULL", True)
    assert tok.shape == (7, 5, 6, 3) and len(tok) == 7 and tok.dtype == np.uint8 and tok.ndim == 4
    assert np.array_equal(e.download_frames(), want) and np.array_equal(e.resolve(tok), want)
    assert np.array_equal(e.resolve(tok[2:5]), want[2:5]) and tok[2:5].shape == (3, 5, 6, 3)
    assert np.array_equal(e.resolve(tok[4:][1:]), want[5:]) and np.array_equal(e.resolve(tok[-2:]), want[-2:])
    assert e.uploads == src.nbytes and e.held_reads == 4
    for bad in (3, slice(0, 4, 2), slice(4, 4), slice(9, 12), (slice(0, 2), 0)):
        with pytest.raises(OpticalFlowCalculationError):
            tok[bad]
    with pytest.raises(OpticalFlowCalculationError, match="at least 2 frames"):
        e.resolve(tok[3:4], min_frames=2)
    with pytest.raises(OpticalFlowCalculationError, match="another engine"):
        FC.NumpyFrames().resolve(tok)
    tok2 = e.hold_frames(FC.source("GRAY", 2, 5, 6), "GRAY")                # the next hold: the first token is stale, its ranges too
    for stale in (tok, tok[1:3]):
        with pytest.raises(OpticalFlowCalculationError, match="stale"):
            e.resolve(stale)
    assert e.resolve(tok2).shape == (2, 5, 6, 3)
    e.release_frames()
    with pytest.raises(OpticalFlowCalculationError, match="stale.*no frames"):
        e.resolve(tok2)
    with pytest.raises(OpticalFlowCalculationError, match="no frames are held"):
        e.download_frames()
    assert isinstance(tok2, HeldFrames) and "generation" in repr(tok2)


def test_library_declares_the_held_frames_calls():
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.dense_flow import DenseFlow
    assert {"tf_hold_frames", "tf_held_frames_shape", "tf_release_frames", "tf_download_frames", "tf_frames_next"} <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    out = np.full(4, -7, np.int64)
    assert L.tf_hold_frames(None, out.ctypes.data, 0, 0, 1, 1, 1) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_frames_next(None, 0, 1) == L.tf_release_frames(None) == L.tf_download_frames(None, out.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_held_frames_shape(None, None) == _lib.TF_ERR_INVALID_ARG and (out == -7).all()
    for name in ("hold_frames", "download_frames", "release_frames"):
        assert callable(getattr(DenseFlow, name))
    assert _lib.FRAMES_FORMS == {"RGB": 0, "GRAY": 1, "YBR_FULL": 2}


def test_a_refused_frames_taking_call_spends_tf_frames_next_without_reading_the_handle():
    """tf_frames_next's state is kept beside the handles: a frames-taking call refused for its arguments spends the flag and never
    reads the handle (the same 64-byte stand-in as in test_otsu_cpu and test_segmentor_glue_cpu), armed or not"""
    import ctypes as C
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(64)            # never dereferenced: every check comes before the handle is used
    h = C.addressof(fake)
    rgb, out = np.zeros((2, 4, 4, 3), np.uint8), np.full((2, 4, 4), 7, np.uint16)
    for armed in (False, True):
        for call in (lambda p: L.tf_condition_frames(h, p, 2, 0, 4, out.ctypes.data),
                     lambda p: L.tf_echo_frames(h, p, 2, 4, -1, out.ctypes.data),
                     lambda p: L.tf_otsu_masks(h, p, 1, 4, 4, 5, out.ctypes.data, None),
                     lambda p: L.tf_segmentor_input(h, p, 2, 4, 4, 0, 8, out.ctypes.data, out.ctypes.data, None)):
            if armed:
                assert L.tf_frames_next(h, 0, 2) == _lib.TF_OK
            assert call(None if armed else rgb.ctypes.data) == _lib.TF_ERR_INVALID_ARG
            assert L.tf_echo_frames(h, None, 2, 4, 4, out.ctypes.data) == _lib.TF_ERR_INVALID_ARG   # spent: a null pointer is a mistake again
    assert (out == 7).all()
