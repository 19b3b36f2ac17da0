"""The consumer's rad/long call of a study without a GPU: the host twins of av_centroids / param_radlong_stats /
calculate_3dhist_radlong against tests/golden/reference_study_stats.npz (the reference's calc_AV_centroid and
calculate_3dhist_radlong on a study file opened by its own OpticalFlowDataset; make_reference_study_stats_fixtures.py), numpy's
gradient types, and the argument checks of tf_av_centroids / tf_radlong_project_param, which return before any GPU work."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
from scipy import ndimage

from tee_optical_flow_amd import analysis as A

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_study_stats.npz")
COMPS = ("radial", "longitudinal")
FIELDS = ("freq", "edges", "hi", "lo")


@pytest.fixture(scope="module")
def z():
    with np.load(FIX) as f:
        return {k: f[k] for k in f.files}


def study(z, frame_rate=None):
    # the fixture was made under numpy 1.26, which divides the gradient in float32 for any frame_rate: a Python float does so here too
    return A.FlowStudy(z["flow"], {"rv": z["rv"], "av": z["av"]}, float(z["frame_rate"]) if frame_rate is None else frame_rate)


def _largest(frame, structure):
    lab, n = ndimage.label(frame, structure=structure)
    areas = np.bincount(lab.ravel())[1:]
    return lab, n, areas


def test_fixture_covers_the_labelling_cases(z):
    av = z["av"][..., 0]
    n = int(z["nframes"])
    assert n == z["flow"].shape[0] - 2 and z["flow"].dtype == np.float16 and z["rv"].dtype == np.bool_
    full, cross = np.ones((3, 3), bool), ndimage.generate_binary_structure(2, 1)
    e = z["case/empty"]
    assert e[0] == 0 and 0 < e[1] < n - 1 and not av[e].any()
    lab, k, areas = _largest(av[z["case/tie"][0]], full)
    assert (areas == areas.max()).sum() == 2
    for f in (z["case/diagonal"][0], z["case/checker"][0], z["case/staircase"][0]):
        lab8, _, a8 = _largest(av[f], full)
        lab4, _, a4 = _largest(av[f], cross)
        assert a8.max() > a4.max()                                   # a 4-connected labeller finds another region, or a smaller one
    # the diagonal join sits on a 64 x 16 tile corner
    f = z["case/diagonal"][0]
    assert av[f, 15, 63] and av[f, 16, 64] and not av[f, 15, 64] and not av[f, 16, 63]
    lab8, _, _ = _largest(av[f], full)
    assert lab8[15, 63] == lab8[16, 64]
    # the checkerboard is one region under 8-connectivity and many under 4
    f = z["case/checker"][0]
    board = av[f, 8:28, 54:74]
    assert ndimage.label(board, structure=full)[1] == 1 and ndimage.label(board, structure=cross)[1] == 200


def test_host_centroids_equal_the_reference(z):
    n = int(z["nframes"])
    got = A.av_centroids(z["av"], n, filter=False)
    assert isinstance(got, list) and len(got) == n
    assert np.array_equal(np.asarray(got, np.float64), z["cent_nofilter"])
    sg = A.av_centroids(z["av"], n, filter=True, savgol_window=9, savgol_poly=4)
    assert isinstance(sg, np.ndarray) and sg.shape == (n, 2)
    np.testing.assert_allclose(sg, z["cent_sg9"], rtol=0, atol=1e-9)       # scipy 1.7 made the fixture


def test_empty_and_short_rules(caplog):
    m = np.zeros((3, 6, 8, 2), bool)
    m[1, 2:4, 3:6] = True
    with caplog.at_level(logging.WARNING):
        got = A.av_centroids(m, 3, filter=True, savgol_window=10)
    assert got == [(3.0, 4.0), (2.5, 4.0), (2.5, 4.0)]              # frame 0: (H/2, W/2); frame 2: carried over; too short: unfiltered
    assert sum("empty AV mask" in r.message for r in caplog.records) == 2
    assert any(r.levelno == logging.ERROR and "Savitzky-Golay" in r.message for r in caplog.records)


def test_host_radlong_equals_the_reference_for_every_param(z):
    st = study(z)
    cent = A.av_centroids(z["av"], st.nframes, filter=False)
    for param in A.PARAMS:
        for got in (A.calculate_3dhist_radlong(study(z), param, av_filter_flag=False),
                    A.calculate_3dhist_radlong(st, param, centroids=cent)):
            for comp in COMPS:
                for i, k in enumerate(FIELDS):
                    assert np.array_equal(got[comp][i], z[f"{param}/{comp}/{k}"]), (param, comp, k)


def test_radlong_refuses_what_the_reference_refuses(z, caplog):
    with caplog.at_level(logging.ERROR):
        assert A.calculate_3dhist_radlong(study(z), "speed") is None
        st = study(z)
        st.mode = "A4C"
        assert A.calculate_3dhist_radlong(st, "velocity") is None
    assert len([r for r in caplog.records if r.levelno == logging.ERROR]) == 2


def test_a_dataset_with_vel_array_only_is_read_as_it_is(z):
    """a reference OpticalFlowDataset has .vel_array (float32) and no .flow"""
    class DS:
        vel_array = z["flow"].astype(np.float32)
        frame_rate = float(z["frame_rate"])
        nframes = int(z["nframes"])
        mode = "RVIO_2class"

        def get_mask(self, label):
            return z[label]
    got = A.calculate_3dhist_radlong(DS(), "PWR", av_filter_flag=False)
    for comp in COMPS:
        for i, k in enumerate(FIELDS):
            assert np.array_equal(got[comp][i], z[f"PWR/{comp}/{k}"])


def test_float64_frame_rate_follows_numpy_in_this_process(z):
    fr = z["frame_rate"][()]                                           # the scalar h5py hands OpticalFlowDataset
    assert isinstance(fr, np.float64)
    assert A.gradient_is_f64(fr) == (int(np.__version__.split(".")[0]) >= 2)
    assert not A.gradient_is_f64(float(fr)) and not A.gradient_is_f64(30)
    n = int(z["nframes"])
    vel = z["flow"].astype(np.float32)
    accel = np.gradient(vel, 1 / fr, axis=0)                           # what OpticalFlowDataset computes in this process
    for param, ref in (("acceleration", accel), ("PWR", vel * accel), ("velocity", vel)):
        got = A.param_field(z["flow"], z["rv"], param, fr, n)
        assert got.dtype == np.float32
        assert np.array_equal(got, (ref * z["rv"])[:n]), param
    if A.gradient_is_f64(fr):
        assert not np.array_equal(A.param_field(z["flow"], z["rv"], "acceleration", float(fr), n), accel[:n] * z["rv"][:n])
    cent = A.av_centroids(z["av"], n, filter=False)
    rad, lon = A.calculate_comp_magnitude((accel * z["rv"])[:n], cent)
    got = A.param_radlong_stats(z["flow"], z["rv"], "acceleration", fr, n, cent, return_arrays=True)
    assert np.array_equal(got["rad_arr"], rad) and np.array_equal(got["long_arr"], lon)


def test_flow_study_defaults():
    st = A.FlowStudy(np.zeros((6, 4, 5, 2), np.float16), {"rv": np.zeros((6, 4, 5, 2), bool)}, 50.0)
    assert st.nframes == 4 and st.mode == "RVIO_2class" and st.flow.dtype == np.float16 and st.vel_array.dtype == np.float32
    assert st.get_mask("av") is None
    with pytest.raises(ValueError):
        A.FlowStudy(np.zeros((6, 4, 5)), {}, 50.0)


def _fake_handle():
    fake = C.create_string_buffer(64)            # never dereferenced: every check comes before the handle is used
    return fake, C.addressof(fake)


def test_tf_av_centroids_rejects_bad_arguments_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    m = np.zeros((2, 4, 4, 2), np.uint8)
    cent = np.zeros((2, 2))
    area = np.zeros(2, np.int64)
    keep, h = _fake_handle()
    good = dict(h=h, m=m.ctypes.data, N=2, H=4, W=4, C=2, cent=cent.ctypes.data, area=area.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_av_centroids(a["h"], a["m"], a["N"], a["H"], a["W"], a["C"], a["cent"], a["area"])

    assert call(h=None) == 1
    for bad in (dict(m=None), dict(cent=None), dict(area=None), dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=3)):
        assert call(**bad) == 1, bad
    assert not cent.any() and not area.any()


def test_tf_radlong_project_param_rejects_bad_arguments_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    flow = np.zeros((3, 4, 4, 2), np.float16)
    m = np.zeros((3, 4, 4, 2), np.uint8)
    cent = np.zeros((2, 2))
    mm = np.zeros(4)
    nz = np.zeros(4, np.int64)
    keep, h = _fake_handle()
    good = dict(h=h, flow=flow.ctypes.data, f16=1, N=3, n=2, H=4, W=4, m=m.ctypes.data, C=2, param=1, sp=0.02, f64=0,
                cent=cent.ctypes.data, rad=None, lon=None, mm=mm.ctypes.data, nz=nz.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_radlong_project_param(a["h"], a["flow"], a["f16"], a["N"], a["n"], a["H"], a["W"], a["m"], a["C"], a["param"], a["sp"],
                                          a["f64"], a["cent"], a["rad"], a["lon"], a["mm"], a["nz"])

    assert call(h=None) == 1
    for bad in (dict(flow=None), dict(m=None), dict(cent=None), dict(mm=None), dict(nz=None), dict(N=0), dict(n=0), dict(H=0),
                dict(W=-2), dict(n=4), dict(C=0), dict(C=3), dict(param=-1), dict(param=3), dict(N=1, n=1),
                dict(N=1, n=1, param=2), dict(sp=0.0), dict(sp=float("inf")), dict(sp=float("nan"))):
        assert call(**bad) == 1, bad
    assert not mm.any() and not nz.any()
