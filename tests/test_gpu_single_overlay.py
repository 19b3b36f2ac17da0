"""The magnitude overlay on the device (tf_magnitude_overlay, tf_held_magnitude_overlay; DenseFlow.magnitude_overlay /
held_magnitude_overlay; analysis.magnitude_overlay(..., engine=)): bytes, (vmin, vmax) and the per-frame (echo max, colour max) equal
the numpy twin's on every case of tests/single_overlay_cases.py -- the reference's recorded frames among them -- through the
host-pointer call and through the held call, after hold_study and after hold_study_chunks.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests.inflate_cases import chunked
from tests.single_overlay_cases import FIXTURE_CASES, Recorder, cases, fixture_study, hot, load_fixture

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.fixture(scope="module")
def z():
    return load_fixture()


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0)
    yield e
    e.close()


def _same(got, want, what):
    assert got[0].dtype == np.uint8 and got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), (what, int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])


def _hold_chunks(e, st):
    N, H, W, _ = st.flow.shape
    ch = (2, 16, 16)
    e.hold_study_chunks(chunked(st.flow, ch + (2,))[0], chunked(st.echo, ch)[0])
    for label, m in st.masks.items():
        m = np.ascontiguousarray(m).view(np.uint8)
        e.hold_mask_chunks(label, chunked(m, ch + (m.shape[3],))[0])
    return A.HeldStudy(e, st.frame_rate, nframes=st.nframes, mode=st.mode, filename=st.filename)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_the_twin(eng, case):
    name, st, param, kw, kib = case
    want = A.magnitude_overlay(st, param, "rv", return_info=True, **kw)
    eng.set_tuning("overlay_chunk_kib", kib)
    try:
        _same(A.magnitude_overlay(st, param, "rv", return_info=True, engine=eng, **kw), want, f"{name}: host arrays")
        if st.flow.dtype == np.float16 and st.echo.dtype == np.float16:
            held = A.HeldStudy.from_study(eng, st)
            c0 = eng.counter("tail_upload_bytes")
            _same(A.magnitude_overlay(held, param, "rv", return_info=True, engine=eng, **kw), want, f"{name}: held")
            assert eng.counter("tail_upload_bytes") == c0                # the held call uploads nothing
            held = _hold_chunks(eng, st)
            _same(A.magnitude_overlay(held, param, "rv", return_info=True, engine=eng, **kw), want, f"{name}: held from chunks")
    finally:
        eng.set_tuning("overlay_chunk_kib", 0)


@pytest.mark.parametrize("case", FIXTURE_CASES)
def test_device_equals_the_reference_frames(eng, z, case):
    name, param = case.split("/")
    out = A.magnitude_overlay(fixture_study(z, name), param, "rv", engine=eng, norm_f64=False)
    assert np.array_equal(out, z[f"{case}/frames"]), case


def test_visualize_magnitude_with_engine(eng, z, tmp_path):
    rec = Recorder()
    path = A.visualize_magnitude(fixture_study(z, "main"), "PWR", "rv", str(tmp_path), fps=24, engine=eng, norm_f64=False, writer_factory=rec)
    assert path.endswith(str(z["main/PWR/path"])) and rec.closed and np.array_equal(np.stack(rec.frames), z["main/PWR/frames"])


def test_the_resident_planes_survive_the_call(eng, z):
    """a rad/long projection before the call is still served by tf_radlong_hist and tf_radlong_overlay after it"""
    from tests.overlay_cases import FIX as RL_FIX, fixture_study as rl_study
    with np.load(RL_FIX) as f:
        zr = {k: f[k] for k in f.files}
    rl = rl_study(zr, "main")
    n = rl.nframes
    cent = A.av_centroids(rl.get_mask("av"), n, filter=False)
    lr, ll = A.colormap_lut("bwr"), A.colormap_lut("BrBG")
    mm, _, _, _ = eng.radlong_project_param(rl.flow, rl.get_mask("rv"), 0, 1 / 30, False, n, cent)
    edges = np.linspace(mm[0], mm[1], 41)
    hist0 = eng.radlong_hist(0, edges, n)
    ov0, info0 = eng.radlong_overlay(rl.echo, lr, ll)
    assert np.array_equal(ov0, zr["main/velocity/frames"])

    def shape():
        s = (C.c_int * 3)()
        assert eng._L.tf_radlong_shape(eng._h, C.byref(s)) == 0
        return tuple(s)
    s0 = shape()
    st = fixture_study(z, "main")                                      # another frame size than the planes'
    for ds in (st, A.HeldStudy.from_study(eng, st)):
        out = A.magnitude_overlay(ds, "PWR", "rv", engine=eng, norm_f64=False)
        assert np.array_equal(out, z["main/PWR/frames"])
        assert shape() == s0 == (n,) + rl.flow.shape[1:3]
        assert np.array_equal(eng.radlong_hist(0, edges, n), hist0)
        ov1, info1 = eng.radlong_overlay(rl.echo, lr, ll)
        assert np.array_equal(ov1, ov0) and np.array_equal(info1, info0)


def test_while_a_submitted_solve_is_in_flight(z):
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(29, 12, 192, 192)
    rgb = np.ascontiguousarray(np.repeat(g[..., None], 3, axis=3))
    e = T.DenseFlow(device_id=0)
    try:
        serial = e.calc_study(rgb).copy()
        t = e.submit_study(rgb)
        for case in FIXTURE_CASES[:4]:
            name, param = case.split("/")
            out = A.magnitude_overlay(fixture_study(z, name), param, "rv", engine=e, norm_f64=False)
            assert np.array_equal(out, z[f"{case}/frames"]), case
        flows = e.wait(t)
    finally:
        e.close()
    assert np.array_equal(flows, serial)


def test_library_refusals_and_their_messages(z):
    e = T.DenseFlow(device_id=0)
    try:
        st = fixture_study(z, "main")
        n, N = st.nframes, st.flow.shape[0]
        rv, lut = st.masks["rv"], hot()

        def call(**kw):
            a = dict(flow=st.flow, mask=rv, param=0, spacing=1 / 30, grad_f64=False, norm_f64=False, n_used=n, echo=st.echo, lut=lut)
            a.update(kw)
            return e.magnitude_overlay(**a)
        good = call()
        assert np.array_equal(good[0], z["main/velocity/frames"])
        # the tables and the data, by message
        for bad_lut, msg in ((-lut, "colormap entry is negative or not finite"), (np.where(lut == lut[0, 0], np.nan, lut), "colormap entry")):
            with pytest.raises(OpticalFlowCalculationError, match=msg):
                call(lut=bad_lut)
        f32 = st.flow.astype(np.float32)
        f32[N - 1, 15, 22, 1] = np.inf                                   # a frame that is not rendered: the range is over all of them
        with pytest.raises(OpticalFlowCalculationError, match="magnitude holds NaN or inf"):
            call(flow=f32)
        for v in (np.nan, np.inf, -1.0):
            echo = st.echo.copy()
            echo[n - 1, 3, 4] = v
            with pytest.raises(OpticalFlowCalculationError, match="echo holds a negative or non-finite value"):
                call(echo=echo)
            e.set_tuning("overlay_chunk_kib", 1)                         # ... from every chunk, not the first alone
            with pytest.raises(OpticalFlowCalculationError, match="echo holds a negative or non-finite value"):
                call(echo=echo)
            e.set_tuning("overlay_chunk_kib", 0)
            bad = fixture_study(z, "main")
            bad.echo = echo
            for en in (None, e):                                       # the data's refusals are the twin's ValueErrors
                with pytest.raises(ValueError, match="negative or non-finite"):
                    A.magnitude_overlay(bad, "velocity", "rv", engine=en)
        # the Python layer's checks, before the library reads anything
        for kw in (dict(n_used=0), dict(n_used=N + 1), dict(param=3), dict(param=1, spacing=0.0), dict(mask=rv[:n]), dict(mask=rv[:, :5]),
                   dict(echo=st.echo[:2]), dict(echo=st.echo.astype(np.float32)), dict(echo=st.echo[:, :4]), dict(lut=lut[:200]),
                   dict(flow=st.flow[..., 0])):
            with pytest.raises(OpticalFlowCalculationError):
                call(**kw)
        # the library's own argument checks: no message, no GPU work
        L, h = e._L, e._h
        fl, m8, ec = np.ascontiguousarray(st.flow), np.ascontiguousarray(rv).view(np.uint8), np.ascontiguousarray(st.echo[:n])
        H, W = fl.shape[1:3]
        out, info, finfo = np.zeros((n, H, W, 3), np.uint8), np.zeros(2), np.zeros((n, 2))

        def raw(N_=N, n_=n, C_=2, param=0, spacing=1 / 30, kind=_lib.ECHO_F16, flow=fl.ctypes.data, echo=ec.ctypes.data):
            return L.tf_magnitude_overlay(h, flow, 1, N_, n_, H, W, m8.ctypes.data, C_, param, spacing, 0, 0, echo, kind, lut.ctypes.data,
                                          out.ctypes.data, info.ctypes.data, finfo.ctypes.data)
        assert raw() == 0 and np.array_equal(out, good[0])
        for kw in (dict(n_=N + 1), dict(n_=0), dict(C_=3), dict(param=3), dict(param=1, spacing=0.0), dict(param=2, spacing=float("nan")),
                   dict(kind=2), dict(flow=None), dict(echo=None), dict(N_=1, n_=1, param=1)):
            assert raw(**kw) == _lib.TF_ERR_INVALID_ARG, kw
        # the held call's refusals, by message
        with pytest.raises(OpticalFlowCalculationError, match="no mask is held"):
            e.held_magnitude_overlay("rv", 0, 1 / 30, False, False, n, lut)
        info2 = np.zeros(2)
        assert L.tf_held_magnitude_overlay(h, n, 0, 0, 1 / 30, 0, 0, lut.ctypes.data, out.ctypes.data, info2.ctypes.data, finfo.ctypes.data) == _lib.TF_ERR_INVALID_ARG
        assert b"no study is held" in L.tf_last_error(h)
        e.hold_study(st.flow)                                            # no echo
        e.hold_mask("rv", rv)
        e.hold_mask("short", rv[:n])
        with pytest.raises(OpticalFlowCalculationError, match="has no echo"):
            e.held_magnitude_overlay("rv", 0, 1 / 30, False, False, n, lut)
        e.hold_study(st.flow, st.echo[:2])
        e.hold_mask("rv", rv)
        e.hold_mask("short", rv[:n])
        with pytest.raises(OpticalFlowCalculationError, match="held echo has 2 frames"):
            e.held_magnitude_overlay("rv", 0, 1 / 30, False, False, n, lut)
        with pytest.raises(OpticalFlowCalculationError, match="fewer than the study's"):
            e.held_magnitude_overlay("short", 0, 1 / 30, False, False, 2, lut)
        for bad_n in (0, N + 1):
            with pytest.raises(OpticalFlowCalculationError, match="outside"):
                e.held_magnitude_overlay("rv", 0, 1 / 30, False, False, bad_n, lut)
        with pytest.raises(OpticalFlowCalculationError, match="spacing"):
            e.held_magnitude_overlay("rv", 1, 0.0, False, False, 2, lut)
        with pytest.raises(OpticalFlowCalculationError, match="colormap entry"):
            e.held_magnitude_overlay("rv", 0, 1 / 30, False, False, 2, -lut)
        # after every refusal the handle renders the same frames, held and not
        two = e.held_magnitude_overlay("rv", 0, 1 / 30, False, False, 2, lut)
        assert np.array_equal(two[0], good[0][:2]) and np.array_equal(two[1], good[1])
        _same(call(), good, "after the refusals")
    finally:
        e.close()
