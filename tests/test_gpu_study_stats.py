"""The consumer's rad/long call of a study on the device (tf_av_centroids, tf_radlong_project_param; DenseFlow.av_centroids /
radlong_project_param; analysis.calculate_3dhist_radlong(..., engine=)): bit-identical to tests/golden/reference_study_stats.npz, which
the reference's own calc_AV_centroid and calculate_3dhist_radlong produced, and to the host twins at study sizes.  The labelling is
checked against scipy.ndimage.label with the 3x3 structure on shapes made to break a tiled 8-connected labeller."""
import os

import numpy as np
import pytest
from scipy import ndimage

from tee_optical_flow_amd import analysis as A
from tests.labelling_cases import load_fuzzer, stress_frames, twins

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_study_stats.npz")
COMPS = ("radial", "longitudinal")


@pytest.fixture(scope="module")
def z():
    with np.load(FIX) as f:
        return {k: f[k] for k in f.files}


def _same_stats(a, b, what=""):
    for comp in COMPS:
        for i in range(4):
            assert np.array_equal(np.asarray(a[comp][i]), np.asarray(b[comp][i])), (what, comp, i)


def _scipy_largest(frame):
    """(centroid, area) of the largest 3x3-connected component (first label on a tie) straight from scipy, or None"""
    lab, n = ndimage.label(frame, structure=np.ones((3, 3), bool))
    if n == 0:
        return None
    areas = ndimage.sum_labels(np.ones_like(lab), lab, np.arange(1, n + 1))
    k = 1 + int(np.argmax(areas))
    rr, cc = np.nonzero(lab == k)
    return (rr.mean(), cc.mean()), len(rr)


def test_device_centroids_equal_the_reference(engine, z):
    n = int(z["nframes"])
    got = A.av_centroids(z["av"], n, filter=False, engine=engine)
    assert np.array_equal(np.asarray(got, np.float64), z["cent_nofilter"])
    cent, area = engine.av_centroids(z["av"][:n])
    for i in range(n):
        want = A._largest_component(z["av"][i, :, :, 0])
        assert (area[i] == 0) if want is None else (area[i] == want[1] and tuple(cent[i]) == want[0]), i


def test_device_radlong_equals_the_reference_for_every_param(engine, z):
    st = A.FlowStudy(z["flow"], {"rv": z["rv"], "av": z["av"]}, float(z["frame_rate"]))      # float: the fixture's float32 gradient
    for param in A.PARAMS:
        got = A.calculate_3dhist_radlong(st, param, av_filter_flag=False, engine=engine)
        want = {c: tuple(z[f"{param}/{c}/{k}"] for k in ("freq", "edges", "hi", "lo")) for c in COMPS}
        _same_stats(got, want, param)
    # the reference's defaults (Savitzky-Golay, window 10): equal to the host twin in this process
    for param in A.PARAMS:
        _same_stats(A.calculate_3dhist_radlong(st, param, engine=engine), A.calculate_3dhist_radlong(st, param), param)


def _study(seed, N, H, W):
    """speckle flow (float16 as a study file holds it), an rv mask of drifting discs, an av mask of random blobs with empty frames"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    flow = rng.normal(0, 4, (N, H, W, 2)).astype(np.float16)
    rv = np.zeros((N, H, W), bool)
    av = np.zeros((N, H, W), bool)
    for f in range(N):
        rv[f] = ((yy - H / 2 - f) / (0.35 * H)) ** 2 + ((xx - W / 2 + f) / (0.4 * W)) ** 2 < 1
        for _ in range(int(rng.integers(0, 6))):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(2, H / 6), rng.uniform(2, W / 6)
            av[f] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
        av[f] ^= rng.random((H, W)) < 0.002                                   # specks, and holes
    av[0] = False
    av[N // 2] = False
    return flow, np.stack([rv, rv], -1), np.stack([av, av], -1)


@pytest.mark.parametrize("N,H,W", [(65, 512, 512), (65, 600, 800)])
def test_study_sized_device_equals_host(engine, N, H, W):
    flow, rv, av = _study(N + H + W, N, H, W)
    n = N - 2
    cent_h = A.av_centroids(av, n)
    cent_d = A.av_centroids(av, n, engine=engine)
    assert np.array_equal(cent_d, cent_h)                                     # filtered (window 10) from equal raw centroids
    raw_h = A.av_centroids(av, n, filter=False)
    assert A.av_centroids(av, n, filter=False, engine=engine) == raw_h
    for param in A.PARAMS:
        host = A.param_radlong_stats(flow, rv, param, 50.0, n, cent_h, return_arrays=True)
        dev = A.param_radlong_stats(flow, rv, param, 50.0, n, cent_h, return_arrays=True, engine=engine)
        _same_stats(dev, host, param)
        assert np.array_equal(dev["rad_arr"], host["rad_arr"]) and np.array_equal(dev["long_arr"], host["long_arr"])
        f32 = A.param_radlong_stats(flow.astype(np.float32), rv, param, 50.0, n, cent_h, engine=engine)
        _same_stats(f32, host, param + " f32 input")
    # a np.float64 frame_rate: the gradient divides in float64 under numpy 2 (and in float32 under numpy 1.x); both paths follow numpy
    fr = np.float64(49.9)
    for param in ("acceleration", "PWR"):
        host = A.param_radlong_stats(flow, rv[..., :1], param, fr, n, cent_h, return_arrays=True)
        dev = A.param_radlong_stats(flow, rv[..., :1], param, fr, n, cent_h, return_arrays=True, engine=engine)
        _same_stats(dev, host, param + " f64")
        assert np.array_equal(dev["rad_arr"], host["rad_arr"])


def test_gradient_edges_and_n_used_equal_to_n(engine):
    """n_used = N: the last projected frame takes the one-sided difference; N = 2: both frames do"""
    rng = np.random.default_rng(5)
    for N, H, W in ((7, 33, 70), (2, 17, 65)):
        flow = rng.normal(0, 2, (N, H, W, 2)).astype(np.float32)
        mask = rng.random((N, H, W, 2)) < 0.8
        cent = [(rng.uniform(0, H), rng.uniform(0, W)) for _ in range(N)]
        for param in A.PARAMS:
            for fr in (30.0, np.float64(29.97)):
                host = A.param_radlong_stats(flow, mask, param, fr, N, cent, nbins=50, return_arrays=True)
                dev = A.param_radlong_stats(flow, mask, param, fr, N, cent, nbins=50, return_arrays=True, engine=engine)
                _same_stats(dev, host, (N, param))
                assert np.array_equal(dev["rad_arr"], host["rad_arr"]) and np.array_equal(dev["long_arr"], host["long_arr"])


def test_labelling_stress_equals_scipy(engine):
    for j, fr in stress_frames().items():
        H, W = fr.shape
        for C in (1, 2):
            m = np.repeat(fr[None, :, :, None], C, axis=3)
            m = np.concatenate([m, m[:, ::-1, ::-1]], axis=0) if H > 1 or W > 1 else m
            cent, area = engine.av_centroids(m)
            for f in range(m.shape[0]):
                want = _scipy_largest(m[f, :, :, 0])
                host = A._largest_component(m[f, :, :, 0])
                if want is None:
                    assert area[f] == 0 and host is None, j
                else:
                    assert area[f] == want[1] == host[1], (j, f, area[f], want[1])
                    assert tuple(cent[f]) == host[0], (j, f)
                    np.testing.assert_allclose(cent[f], want[0], rtol=0, atol=1e-9)


@pytest.mark.parametrize("seed,H,W,down_left", [((1, 0), 12, 40, False), ((5, 1), 40, 150, False), ((3, 2), 33, 130, True)])
def test_equal_largest_areas_pick_the_earliest_first_pixel(engine, seed, H, W, down_left):
    """k_cent_pick's tie rule on frames whose two largest components are copies of one blob: inside one tile, with first pixels in
    different tiles, and with the later copy lower and further left, so that it has the smaller column centroid.  Exact."""
    F = load_fuzzer()
    m = twins(np.random.default_rng(seed), H, W, down_left=down_left)
    t = F.ref_components(m)
    first, later = sorted((r for r in t.tolist() if r[0] == t[:, 0].max()), key=lambda r: r[1])[:2]
    assert first[0] == later[0] > 1 and first[1] < later[1]
    tile = lambda r: (r[1] // W // 16, r[1] % W // 64)
    assert (tile(first) != tile(later)) == (H > 16)
    assert (later[3] / later[0] < first[3] / first[0]) == down_left
    want = ((first[2] / first[0], first[3] / first[0]), first[0])
    assert F.ref_centroid(m) == want == A._largest_component(m)
    for frames in (m[None, :, :, None], np.stack([m, m[::-1, ::-1], m])[..., None]):          # alone, and between other frames
        cent, area = engine.av_centroids(frames)
        for f in range(frames.shape[0]):
            (r, c), a = F.ref_centroid(frames[f, :, :, 0])
            assert int(area[f]) == a and float(cent[f, 0]) == r and float(cent[f, 1]) == c, (f, area[f], tuple(cent[f]), a, (r, c))


def test_beside_a_submitted_study(z):
    """both calls run on the handle's stream while a submitted study solves on the lanes: same results, same flows"""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(21, 40, 128, 160)
    rgb = np.repeat(g[..., None], 3, axis=3)
    st = A.FlowStudy(z["flow"], {"rv": z["rv"], "av": z["av"]}, float(z["frame_rate"]))
    eng = T.DenseFlow(device_id=0)
    try:
        serial = eng.calc_study(rgb).copy()
        alone = {p: A.calculate_3dhist_radlong(st, p, av_filter_flag=False, engine=eng) for p in A.PARAMS}
        t = eng.submit_study(rgb)
        beside = {p: A.calculate_3dhist_radlong(st, p, av_filter_flag=False, engine=eng) for p in A.PARAMS}
        flows = eng.wait(t)
    finally:
        eng.close()
    for p in A.PARAMS:
        _same_stats(beside[p], alone[p], p)
        want = {c: tuple(z[f"{p}/{c}/{k}"] for k in ("freq", "edges", "hi", "lo")) for c in COMPS}
        _same_stats(beside[p], want, p)
    assert np.array_equal(flows, serial)


def test_analysis_session_survives_a_solve():
    """The planes a projection leaves on the device belong to the handle, not to its solver: a solve on the same engine -- here one that
    makes the solver allocate, on an engine without lanes -- leaves tf_radlong_hist's answer and tf_radlong_shape's as they were."""
    import ctypes as C
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.synth import speckle_pair
    rng = np.random.default_rng(14)
    flow = rng.normal(0, 2, (3, 24, 32, 2)).astype(np.float32)
    cent = [(11.5, 15.25), (12.0, 16.0), (3.75, 30.5)]
    edges = np.linspace(-6.0, 6.0, 41)
    eng = T.DenseFlow(device_id=0)
    eng.set_tuning("queue_lanes", 0)

    def session():
        freq, shape = np.zeros((3, 40), np.int64), (C.c_int * 3)()
        _lib.check(eng._L.tf_radlong_hist(eng._h, 0, edges.ctypes.data, 40, freq.ctypes.data), eng._h, "tf_radlong_hist")
        _lib.check(eng._L.tf_radlong_shape(eng._h, C.byref(shape)), eng._h, "tf_radlong_shape")
        return freq, tuple(shape)
    try:
        A.radlong_stats_device(eng, flow, cent)
        before, shape = session()
        assert shape == (3, 24, 32) and before.sum() > 0
        I0, I1, _ = speckle_pair(9, 48, 64)
        assert eng.calc(I0, I1, None).shape == (48, 64, 2)
        after, shape = session()
    finally:
        eng.close()
    assert np.array_equal(after, before) and shape == (3, 24, 32)
