"""The polar steps of the consumer on the device (tf_polar_project_param; DenseFlow.polar_project_param; analysis.calculate_3dhist /
angle_mode_series with engine=): bit-identical to tests/golden/reference_polar.npz, which the reference's own calculate_3dhist and
AngleDetector.detect produced on analysis.cart_to_polar, to cart_to_polar itself on stress inputs, and to the host twins at study
size, alone and beside a submitted study."""
import os

import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTS = ("mag_freq", "ang_freq", "mag_edges", "ang_edges", "hi")


@pytest.fixture(scope="module")
def z():
    with np.load(os.path.join(GOLD, "reference_polar.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def studies(z):
    with np.load(os.path.join(GOLD, "reference_study_stats.npz")) as f:
        st = A.FlowStudy(f["flow"], {"rv": f["rv"], "av": f["av"]}, np.float64(f["frame_rate"]))
    ss = A.FlowStudy(z["stress/flow"], {"all": z["stress/all"], "late": z["stress/late"]}, np.float64(z["stress/frame_rate"]),
                     nframes=int(z["stress/nframes"]))
    return {"study": (st, ("rv", "av")), "stress": (ss, ("all", "late"))}


def _same(got, want, what):
    for i, k in enumerate(OUTS):
        g, w = np.asarray(got[i]), np.asarray(want[i])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


def _check_fixture(engine, z, studies):
    for tag, (st, labels) in studies.items():
        for param in A.PARAMS:
            for label in labels:
                key = f"{tag}/{param}/{label}"
                if f"{key}/raises" in z:
                    with pytest.raises(IndexError):
                        A.calculate_3dhist(st, param, label, engine=engine)
                else:
                    _same(A.calculate_3dhist(st, param, label, engine=engine), tuple(z[f"{key}/{k}"] for k in OUTS), key)
                got = A.angle_mode_series(st, param, label, engine=engine)
                w = z[f"{key}/ang_mode"]
                assert got.dtype == w.dtype and np.array_equal(got, w, equal_nan=True), key


def test_device_equals_the_reference(engine, z, studies):
    _check_fixture(engine, z, studies)


def test_device_planes_equal_cart_to_polar_on_stress_inputs(engine, z):
    """the planes bit for bit, on the fixture's stress study and on inputs where the unfused magnitude rounds differently (so the
    kernel's equality with the fma form shows that it fuses)"""
    rng = np.random.default_rng(9)
    fl = z["stress/flow"]
    extra = rng.normal(0, 3, (3, 37, 129, 2)).astype(np.float32)
    extra[0, 0, :8] = [(0, 0), (-0.0, 0), (0, -0.0), (-0.0, -0.0), (-1, -0.0), (1e-45, 0), (-1e-45, -1e-45), (4, -4)]
    for flow, mask in ((fl, z["stress/all"]), (fl, z["stress/late"][..., :1]), (extra, np.ones((3, 37, 129, 2), bool))):
        n = flow.shape[0]
        for param in A.PARAMS:
            for fr in (30.0, np.float64(29.97)):
                mm, nz, mode, mag, ang = engine.polar_project_param(flow, mask, A.PARAMS.index(param), 1 / fr, A.gradient_is_f64(fr), n,
                                                                   return_arrays=True)
                field = A.param_field(flow, mask, param, fr, n)
                hm, ha = A.cart_to_polar(field[..., 0], field[..., 1])
                assert np.array_equal(mag.view(np.int32), hm.view(np.int32)) and np.array_equal(ang.view(np.int32), ha.view(np.int32))
                assert np.array_equal(mm, np.float32([hm.min(), hm.max(), ha.min(), ha.max()]))
                assert np.array_equal(nz, np.stack([(hm != 0).sum((1, 2)), (ha != 0).sum((1, 2))], 1))
                want = np.asarray([A._mode_of_rounded(ha[i]) for i in range(n)], np.float32)
                assert np.array_equal(mode, want, equal_nan=True), (param, fr)
                if param == "velocity" and flow is extra:
                    unfused = np.sqrt(field[..., 0] * field[..., 0] + field[..., 1] * field[..., 1])
                    assert (mag != unfused).any()


def _study(seed, N, H, W):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    flow = rng.normal(0, 4, (N, H, W, 2)).astype(np.float16)
    flow[:, : H // 8] = np.abs(flow[:, : H // 8])                           # a band of one quadrant: a clear mode
    rv = np.zeros((N, H, W), bool)
    av = np.zeros((N, H, W), bool)
    for f in range(N):
        rv[f] = ((yy - H / 2 - f) / (0.35 * H)) ** 2 + ((xx - W / 2 + f) / (0.4 * W)) ** 2 < 1
        av[f] = ((yy - H / 5) / (0.15 * H)) ** 2 + ((xx - W / 3 - f) / (0.2 * W)) ** 2 < 1
    av[N // 2] = False                                                       # an empty frame in the middle
    return A.FlowStudy(flow, {"rv": np.stack([rv, rv], -1), "av": av[..., None]}, np.float64(50.0))


def test_study_sized_device_equals_host(engine):
    st = _study(4, 65, 512, 512)
    for param in A.PARAMS:
        for label in ("rv", "av"):
            _same(A.calculate_3dhist(st, param, label, engine=engine), A.calculate_3dhist(st, param, label), (param, label))
            d = A.angle_mode_series(st, param, label, engine=engine)
            h = A.angle_mode_series(st, param, label)
            assert np.array_equal(d, h, equal_nan=True), (param, label)


@pytest.mark.parametrize("algo", ["TVL1", "deepflow"])
def test_beside_a_submitted_study(algo, z, studies):
    """tf_polar_project_param and the statistics run on the handle's stream while a submitted study solves on the lanes: the same
    results, and the same flows as the study alone"""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(23, 24, 256, 256)
    rgb = np.ascontiguousarray(np.repeat(g[..., None], 3, axis=3))
    eng = T.DenseFlow(device_id=0, algo=algo)
    try:
        serial = eng.calc_study(rgb).copy()
        t = eng.submit_study(rgb)
        _check_fixture(eng, z, studies)
        flows = eng.wait(t)
    finally:
        eng.close()
    assert np.array_equal(flows, serial)


def test_argument_errors_come_before_gpu_work(engine, z):
    fl = z["stress/flow"]
    m = z["stress/all"]
    n = int(z["stress/nframes"])
    bad = [dict(flow=fl[..., :1]), dict(flow=fl[0]), dict(n_used=0), dict(n_used=fl.shape[0] + 1), dict(param=3), dict(param="PWR"),
           dict(mask=m[:, :5]), dict(mask=m.astype(np.float32)), dict(mask=np.zeros(m.shape[:3] + (3,), bool)),
           dict(flow=fl[:1], n_used=1), dict(spacing=0.0), dict(spacing=float("nan"))]
    for b in bad:
        a = dict(flow=fl, mask=m, param=1, spacing=1 / 30, grad_f64=False, n_used=n)
        a.update(b)
        with pytest.raises(OpticalFlowCalculationError):
            engine.polar_project_param(a["flow"], a["mask"], a["param"], a["spacing"], a["grad_f64"], a["n_used"])
    # and the engine is untouched: the next call is exact
    st = A.FlowStudy(fl, {"all": m}, np.float64(z["stress/frame_rate"]), nframes=n)
    _same(A.calculate_3dhist(st, "velocity", "all", engine=engine), tuple(z[f"stress/velocity/all/{k}"] for k in OUTS), "after")
