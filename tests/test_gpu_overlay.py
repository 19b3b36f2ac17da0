"""The rad/long overlay frames on the device (tf_radlong_overlay; DenseFlow.radlong_overlay; analysis.radlong_overlay(..., engine=)):
bit-identical to tests/golden/reference_overlay.npz, the frames the reference's own visualize_radlong and
VisualizationManager.visualize_radlong handed to their video writer, and to the numpy twin at study sizes, at the smallest sizes and on
100 seeded random cases.  No tolerance anywhere."""
import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests.overlay_cases import CASES, COLORMAPS, FIX, Recorder, fixture_study, random_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    with np.load(FIX) as f:
        return {k: f[k] for k in f.files}


def _both(st, param, cent, engine, **kw):
    host, hinfo = A.radlong_overlay(st, param, centroids=cent, return_info=True, **kw)
    dev, dinfo = A.radlong_overlay(st, param, centroids=cent, return_info=True, engine=engine, **kw)
    assert dev.dtype == np.uint8 and dev.shape == host.shape
    assert np.array_equal(dev, host), (param, kw, int((dev != host).sum()))
    assert np.array_equal(dinfo, hinfo), (dinfo, hinfo)
    return dev, dinfo


def _check_fixture(engine, z):
    for case, kw in CASES:
        st = fixture_study(z, case.split("/")[0])
        out, info = A.radlong_overlay(st, case.split("/")[1], av_filter_flag=False, return_info=True, engine=engine, **kw)
        assert np.array_equal(out, z[f"{case}/frames"]), case
        if case.startswith("vm"):
            assert info[2] == z["vm/m2"]
        if case.startswith("empty0"):
            assert info[0] == 0


def test_device_equals_the_reference(engine, z):
    _check_fixture(engine, z)


def _study(seed, N, H, W, echo_dtype=np.float16):
    """speckle flow that is quiet in frame 0 (later frames leave +-half), an rv mask of drifting discs, a sector-like echo"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    amp = np.concatenate([[0.5], rng.uniform(1, 6, N - 1)])[:, None, None, None] if N > 1 else 1.0
    flow = (rng.normal(0, 1, (N, H, W, 2)) * amp).astype(np.float16)
    rv = np.zeros((N, H, W), bool)
    for f in range(N):
        rv[f] = ((yy - H / 2 - f / 4) / (0.35 * H + 1)) ** 2 + ((xx - W / 2 + f / 4) / (0.4 * W + 1)) ** 2 < 1
    echo = rng.integers(0, 256, (N, H, W))
    if echo_dtype == np.float16:
        echo = (echo * rng.choice([1.0, 0.25, 200.0])).astype(np.float16)
    else:
        echo = echo.astype(np.uint8)
    echo[0, 0, 0] = max(echo[0, 0, 0], 1)
    return flow, np.stack([rv, rv], -1), echo


@pytest.mark.parametrize("N,H,W", [(65, 512, 512), (65, 600, 800)])
def test_study_sized_device_equals_host(engine, N, H, W):
    flow, rv, echo = _study(N + H + W, N, H, W)
    n = N - 2
    rng = np.random.default_rng(N)
    cent = [(H / 3 + rng.uniform(-5, 5), W / 2 + rng.uniform(-5, 5)) for _ in range(n)]
    st = A.FlowStudy(flow, {"rv": rv, "av": rv}, 50.0, echo=echo)
    for param in A.PARAMS:
        _, info = _both(st, param, cent, engine)
        assert info[0] > 0 and info[1] == echo[:n].max()
    st8 = A.FlowStudy(flow, {"rv": rv, "av": rv}, 50.0, echo=_study(N, N, H, W, np.uint8)[2])
    _both(st8, "velocity", cent, engine, colormap_rad="PiYG", colormap_long="viridis")


@pytest.mark.parametrize("N,n,H,W", [(3, 1, 1, 1), (1, 1, 1, 1), (5, 3, 37, 53), (2, 1, 37, 53), (1, 1, 64, 3), (4, 4, 2, 2), (6, 5, 3, 1)])
def test_small_and_ragged_sizes(engine, N, n, H, W):
    for dt in (np.float16, np.uint8):
        flow, rv, echo = _study(N * 1000 + H + W, N, H, W, dt)
        rv[:] = True
        st = A.FlowStudy(flow, {"rv": rv, "av": rv}, 30.0, nframes=n, echo=echo)
        cent = [(H / 2 + 0.25, W / 2 - 0.25)] * n
        for param in A.PARAMS if N > 1 else ("velocity",):
            _both(st, param, cent, engine)


def test_subnormal_echo_on_the_device(engine):
    rng = np.random.default_rng(11)
    N, H, W = 4, 45, 70
    flow, rv, _ = _study(11, N, H, W)
    echo = rng.integers(0, 2, (N, H, W)).astype(np.float16)
    echo[1, 20, 30] = 60000
    st = A.FlowStudy(flow, {"rv": rv, "av": rv}, 30.0, echo=echo)
    out, info = _both(st, "velocity", [(20.0, 30.0)] * 2, engine)
    assert info[1] == 60000
    # the float16 steps are visible in the result: float64 arithmetic on the same echo gives other bytes
    e64 = 0.5 * (echo[:2].astype(np.float64) / 60000.0)
    e16 = (0.5 * (echo[:2] / np.float16(60000))).astype(np.float64)
    assert (e64 != e16).any()
    # smaller still: every quotient's half underflows float16 to 0 or to its smallest subnormal
    echo2 = np.full((N, H, W), 6e-8, np.float16)
    echo2[0, 0, 0] = 1
    echo2[1] = 1.2e-7
    st.echo = echo2
    _both(st, "acceleration", [(20.0, 30.0)] * 2, engine)


def test_half_zero_and_custom_colormaps(engine):
    N, H, W = 5, 41, 67
    flow, rv, echo = _study(5, N, H, W)
    rv[0] = False                                                      # frame 0's field is all zero: half == 0
    st = A.FlowStudy(flow, {"rv": rv, "av": rv}, 30.0, echo=echo)
    cent = [(20.5, 33.5)] * 3
    out, info = _both(st, "velocity", cent, engine)
    assert info[0] == 0
    rng = np.random.default_rng(9)
    lut_a, lut_b = rng.uniform(0, 1, (256, 3)), rng.uniform(0, 0.5, (256, 3))
    lut_b[0] = 0
    rv[0] = True
    _, info = _both(st, "PWR", cent, engine, colormap_rad=lut_a, colormap_long=lut_b)
    assert info[2] != 1
    for a in COLORMAPS:
        _both(st, "velocity", cent, engine, colormap_rad=a, colormap_long=COLORMAPS[(COLORMAPS.index(a) + 1) % 4])


def test_visualize_radlong_with_engine(engine, z, tmp_path):
    rec = Recorder()
    st = fixture_study(z, "main")
    path = A.visualize_radlong(st, "PWR", str(tmp_path), fps=24, av_filter_flag=False, engine=engine, writer_factory=rec)
    assert path.endswith(str(z["main/PWR/path"])) and rec.closed and np.array_equal(np.stack(rec.frames), z["main/PWR/frames"])


def test_on_a_deepflow_handle(z):
    import tee_optical_flow_amd as T
    eng = T.createOptFlow_DeepFlow()
    try:
        _check_fixture(eng, z)
    finally:
        eng.close()


@pytest.mark.parametrize("algo", ["TVL1", "deepflow"])
def test_while_submitted_studies_are_in_flight(z, algo):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(29, 24, 256, 256)
    rgb = np.ascontiguousarray(np.repeat(g[..., None], 3, axis=3))
    eng = T.DenseFlow(device_id=0, algo=algo)
    try:
        serial = eng.calc_study(rgb).copy()
        t = eng.submit_study(rgb)
        _check_fixture(eng, z)
        flows = eng.wait(t)
    finally:
        eng.close()
    assert np.array_equal(flows, serial)


def test_refusals_leave_the_handle_usable(z):
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    try:
        st = fixture_study(z, "main")
        n = st.nframes
        lut = A.colormap_lut("bwr")
        with pytest.raises(OpticalFlowCalculationError, match="needs a preceding"):
            eng.radlong_overlay(st.echo, lut, lut)                     # before any projection
        eng.polar_project_param(st.flow, st.get_mask("rv"), 0, 1 / 30, False, n)
        with pytest.raises(OpticalFlowCalculationError, match="tf_polar_project_param"):
            eng.radlong_overlay(st.echo, lut, lut)
        _check_fixture(eng, z)                                          # still usable
        # argument errors, before any GPU work: the planes of the last projection stay valid
        for bad in (dict(echo=st.echo.astype(np.float32)), dict(echo=st.echo[:2]), dict(echo=st.echo[:, :4]), dict(echo=st.echo[0]),
                    dict(lut_rad=lut[:200]), dict(lut_rad=-lut), dict(lut_long=np.where(lut == lut[0, 0], np.inf, lut))):
            a = dict(echo=st.echo, lut_rad=lut, lut_long=lut)
            a.update(bad)
            with pytest.raises(OpticalFlowCalculationError):
                eng.radlong_overlay(a["echo"], a["lut_rad"], a["lut_long"])
        good, _ = eng.radlong_overlay(st.echo, lut, lut)
        # the data's refusals are the twin's ValueErrors
        cent = A.av_centroids(st.get_mask("av"), n, filter=False)
        for v in (np.nan, np.inf, -1.0):
            bad = fixture_study(z, "main")
            bad.echo = bad.echo.copy()
            bad.echo[n - 1, 3, 4] = v
            for e in (None, eng):
                with pytest.raises(ValueError, match="negative or non-finite"):
                    A.radlong_overlay(bad, "velocity", centroids=cent, engine=e)
        bad = fixture_study(z, "main")
        bad.echo = np.zeros_like(bad.echo)
        for e in (None, eng):
            with pytest.raises(ValueError, match="maximum is 0"):
                A.radlong_overlay(bad, "velocity", centroids=cent, engine=e)
        bad = fixture_study(z, "main")
        bad.flow = bad.flow.astype(np.float32)
        bad.flow[2, 15, 22, 0] = np.inf
        for e in (None, eng):
            with pytest.raises(ValueError, match="NaN or inf"):
                A.radlong_overlay(bad, "velocity", centroids=cent, engine=e)
        black = np.zeros((256, 3))
        for e in (None, eng):
            with pytest.raises(ValueError, match="black"):
                A.radlong_overlay(st, "velocity", centroids=cent, colormap_rad=black, colormap_long=black, engine=e)
        # after every refusal: the same frames as before
        eng.radlong_project_param(st.flow, st.get_mask("rv"), 0, 1 / 30, False, n, cent)
        again, _ = eng.radlong_overlay(st.echo, lut, lut)
        assert np.array_equal(again, good)
        _check_fixture(eng, z)
    finally:
        eng.close()


@pytest.mark.parametrize("dt", [np.float16, np.uint8], ids=["f16", "u8"])
def test_a_study_of_several_chunks(z, dt):
    """The echo and the output go through in chunks of frames of at most 512 MiB, which no test-sized study fills: the
    overlay_chunk_kib knob shrinks the chunk.  7 frames of 37 x 53 take 8 (float16 echo) or 7 bytes per pixel, 15.3 / 13.4 KiB a
    frame: 40 KiB = chunks of 2, 2, 2, 1 frames; 50 KiB = 3, 3, 1; 1 KiB = less than a frame, so one frame at a time; 0 = the default."""
    import tee_optical_flow_amd as T
    N, n, H, W = 9, 7, 37, 53
    flow, rv, echo = _study(77, N, H, W, dt)
    st = A.FlowStudy(flow, {"rv": rv, "av": rv}, 30.0, echo=echo)
    cent = [(H / 2 + 0.25 * f, W / 2 - 0.5 * f) for f in range(n)]
    eng = T.DenseFlow(device_id=0)
    try:
        whole, winfo = _both(st, "velocity", cent, eng)
        for kib in (40, 50, 1, 0):
            eng.set_tuning("overlay_chunk_kib", kib)
            for param, kw in (("velocity", {}), ("PWR", dict(colormap_rad="BrBG", colormap_long="PiYG"))):
                out, info = _both(st, param, cent, eng, **kw)
                if param == "velocity":
                    assert np.array_equal(out, whole) and np.array_equal(info, winfo), kib
            _check_fixture(eng, z)
        # the refusals that are found on the device come from every chunk, not the first alone
        eng.set_tuning("overlay_chunk_kib", 40)
        bad = A.FlowStudy(flow, {"rv": rv, "av": rv}, 30.0, echo=echo.copy())
        if dt == np.float16:
            bad.echo[n - 1, H - 1, W - 1] = np.nan
            with pytest.raises(ValueError, match="negative or non-finite"):
                A.radlong_overlay(bad, "velocity", centroids=cent, engine=eng)
        bad.echo[:] = 0
        bad.echo[n - 1, H - 1, W - 1] = 3                              # the maximum sits in the last, shorter chunk
        _, info = _both(bad, "velocity", cent, eng)
        assert info[1] == 3
    finally:
        eng.close()


def test_the_resident_shape_query(z):
    import ctypes as C
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    try:
        def shape():
            s = (C.c_int * 3)()
            assert eng._L.tf_radlong_shape(eng._h, C.byref(s)) == 0
            return tuple(s)
        st = fixture_study(z, "main")
        n, H, W = st.nframes, st.flow.shape[1], st.flow.shape[2]
        assert shape() == (0, 0, 0)
        cent = A.av_centroids(st.get_mask("av"), n, filter=False)
        eng.radlong_project_param(st.flow, st.get_mask("rv"), 0, 1 / 30, False, n, cent)
        assert shape() == (n, H, W)
        eng.polar_project_param(st.flow, st.get_mask("rv"), 0, 1 / 30, False, n)
        assert shape() == (0, 0, 0)
        eng.radlong_project_param(st.flow, st.get_mask("rv"), 0, 1 / 30, False, n - 1, cent[:n - 1])
        assert shape() == (n - 1, H, W)
    finally:
        eng.close()


def test_after_the_plain_projection(engine):
    """tf_radlong_project (float32 flow, no param field) leaves planes the overlay takes as well"""
    rng = np.random.default_rng(21)
    N, H, W = 3, 19, 31
    flow = rng.normal(0, 2, (N, H, W, 2)).astype(np.float32)
    cent = [(9.0, 15.5)] * N
    echo = rng.integers(0, 200, (N, H, W)).astype(np.uint8)
    res = A.radlong_stats_device(engine, flow, cent, nbins=20, return_arrays=True)
    lr, ll = A.colormap_lut("bwr"), A.colormap_lut("BrBG")
    dev, dinfo = engine.radlong_overlay(echo, lr, ll)
    host, hinfo = A.overlay_host(res["rad_arr"], res["long_arr"], echo, lr, ll)
    assert np.array_equal(dev, host) and np.array_equal(dinfo, hinfo)


def test_100_random_cases_equal_the_twin(engine):
    same = 0
    for k in range(100):
        st, param, kw, cent = random_case(20261017 + k)
        _both(st, param, cent, engine, **kw)
        same += 1
    assert same == 100
