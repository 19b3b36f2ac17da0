"""The polar steps of the consumer without a GPU: the float32 fma emulation against exact rational arithmetic, cart_to_polar on
hand-derived values, the float32 percentile mirror and the histogram rule of k_radlong_hist against numpy, the host calculate_3dhist
and angle_mode_series against tests/golden/reference_polar.npz (the reference's own calculate_3dhist and AngleDetector.detect,
make_reference_polar_fixtures.py), and the argument checks of tf_polar_project_param, which return before any GPU work."""
import ctypes as C
import logging
import os
from fractions import Fraction

import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A
from tests.stats_cases import device_hist_rule as _device_hist_rule

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTS = ("mag_freq", "ang_freq", "mag_edges", "ang_edges", "hi")
S = np.float32(np.pi / 180)                                  # (float)(CV_PI / 180)


@pytest.fixture(scope="module")
def z():
    with np.load(os.path.join(GOLD, "reference_polar.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def studies(z):
    """the fixture's two studies as FlowStudy, frame_rate a np.float64 as the reference's OpticalFlowDataset holds it"""
    with np.load(os.path.join(GOLD, "reference_study_stats.npz")) as f:
        st = A.FlowStudy(f["flow"], {"rv": f["rv"], "av": f["av"]}, np.float64(f["frame_rate"]))
    ss = A.FlowStudy(z["stress/flow"], {"all": z["stress/all"], "late": z["stress/late"]}, np.float64(z["stress/frame_rate"]),
                     nframes=int(z["stress/nframes"]))
    return {"study": (st, ("rv", "av")), "stress": (ss, ("all", "late"))}


def _round32(fr):
    """the float32 nearest the Fraction fr, ties to even"""
    f = np.float32(float(fr))
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - fr)
        if best is None or d < best[0] or (d == best[0] and int(np.float32(c).view(np.int32)) % 2 == 0):
            best = (d, c)
    return np.float32(best[1])


def test_fma32_equals_exact_rational_arithmetic():
    rng = np.random.default_rng(11)
    n = 30000
    a, b, c = ((rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32) for _ in range(3))
    # the first half: c chosen so that a*b + c lands on (or next to) a float32 midpoint, where a double rounding would go wrong
    half = n // 2
    p = a[:half].astype(np.float64) * b[:half]
    r = p.astype(np.float32)
    mid = r.astype(np.float64) + np.spacing(r).astype(np.float64) / 2
    c[:half] = (mid - p).astype(np.float32)
    c[:half:3] = np.nextafter(c[:half:3], np.float32(np.inf))
    c[1:half:3] = np.nextafter(c[1:half:3], np.float32(-np.inf))
    got = A.fma32(a, b, c)
    for i in range(n):
        want = _round32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i].view(np.int32) == want.view(np.int32), (i, a[i], b[i], c[i], got[i], want)
    # exact cancellation gives +0, as an IEEE fma in round-to-nearest does
    assert A.fma32(np.float32(3), np.float32(-1), np.float32(3)).view(np.int32) == 0


def test_cart_to_polar_on_hand_derived_values():
    x = np.float32([2.5, 0, -2.5, 0, 0, -0.0, 0, -0.0, -2.5, 1.5, -1.5, -1.5, 1.5])
    y = np.float32([0, 2.5, 0, -2.5, 0, 0, -0.0, -0.0, -0.0, 1.5, 1.5, -1.5, -1.5])
    mag, ang = A.cart_to_polar(x, y)
    assert mag.dtype == ang.dtype == np.float32
    want = np.float32([0, 90, 180, 270, 0, 0, 0, 0, 180]) * S                   # the axes: the polynomial is 0 (or 90 - 0) there
    assert np.array_equal(ang[:9].view(np.int32), want.view(np.int32))
    assert np.array_equal(mag[:9], np.float32([2.5, 2.5, 2.5, 2.5, 0, 0, 0, 0, 2.5]))
    # |x| = |y|: c = |x| / (|x| + eps) and the four quadrants mirror one value
    c = np.float32(1.5) / (np.float32(1.5) + np.float32(np.finfo(np.float64).eps))
    cc = c * c
    a = A.fma32(A.fma32(A.fma32(cc, A._P7, A._P5), cc, A._P3), cc, A._P1) * c
    assert np.array_equal(ang[9:], np.float32([a, np.float32(180) - a, np.float32(360) - (np.float32(180) - a), np.float32(360) - a]) * S)
    assert np.all(mag[9:] == np.sqrt(A.fma32(np.float32(1.5), np.float32(1.5), np.float32(2.25))))


def test_cart_to_polar_fuses_where_the_unfused_form_differs():
    """the magnitude's fma: the stress values include inputs whose unfused sqrt(x*x + y*y) rounds differently"""
    rng = np.random.default_rng(2)
    x = rng.normal(0, 3, 200000).astype(np.float32)
    y = rng.normal(0, 3, 200000).astype(np.float32)
    mag, _ = A.cart_to_polar(x, y)
    unfused = np.sqrt(x * x + y * y)
    assert (mag != unfused).any()
    assert np.array_equal(mag, np.sqrt(A.fma32(x, x, y * y)))


def test_float32_percentile_mirror_equals_numpy():
    rng = np.random.default_rng(7)
    lengths = [1, 2, 3, 99, 100, 101, 1000, 4097] + rng.integers(1, 20000, 300).tolist() + [65536, 262144, 480000]
    for n in lengths:
        a = (rng.standard_normal(n) * rng.uniform(0.01, 50)).astype(np.float32)
        srt = np.sort(a)
        for q in (99, 1, 50, 99.5):
            p, nx, g = A.percentile_index(n, q)
            got = A._lerp(srt[p], srt[nx], g)
            want = np.percentile(a, q)
            assert type(got) is type(want) and got.view(np.int32) == want.view(np.int32), (n, q, got, want)


def test_histogram_rule_of_the_device_equals_numpy_on_float32_edges():
    rng = np.random.default_rng(3)
    for t in range(60):
        v = np.abs(rng.standard_normal(int(rng.integers(1, 50000))) * rng.uniform(0.001, 100)).astype(np.float32)
        if t % 3 == 0:
            v = (v % np.float32(2 * np.pi)).astype(np.float32)
        mn, mx = np.min(v), np.max(v)
        nz = v[v != 0]
        edges = A._polar_edges(mn, mx, 1000)
        assert edges.dtype == np.float32
        freq, e2 = np.histogram(nz, bins=1000, range=(mn, mx))
        assert np.array_equal(edges, e2)
        assert np.array_equal(_device_hist_rule(nz, edges), freq), t


def test_fixture_covers_the_stress_cases(z):
    fl = z["stress/flow"]
    r0, c0, c1 = z["stress/case/signed"]
    assert np.signbit(fl[0, r0, c0:c1]).any() and (fl[0, r0, c0:c1] == 0).any()
    mag, ang = A.cart_to_polar(fl[..., 0] * z["stress/all"][..., 0], fl[..., 1] * z["stress/all"][..., 1])
    f = z["stress/case/no_angle"][0]
    assert (mag[f] != 0).any() and not (ang[f] != 0).any()
    r = ang[:3, 1:4] * np.float32(100)
    d = np.abs(r - (np.floor(r) + np.float32(0.5)))
    assert (d <= np.spacing(r)).all() and (d == 0).any()                     # near np.round's .5 tie, some exactly on it
    assert not z["stress/late"][z["stress/case/late_empty"][0]:].any()
    n = int(z["stress/nframes"])
    late_mode = z["stress/velocity/late/ang_mode"]
    assert np.isnan(late_mode[f]) and np.isnan(late_mode[4:n]).all() and not np.isnan(late_mode[:3]).any()   # no angle: NaN
    f = z["stress/case/mode_tie"][0]
    k, cnt = np.unique(np.rint(ang[f][ang[f] != 0] * np.float32(100)), return_counts=True)
    assert cnt.max() == cnt[k == 157][0] == cnt[k == 314][0]                 # a tie: the mode is the smaller value
    assert z["stress/velocity/all/ang_mode"][f] == np.float32(157) / np.float32(100)
    assert str(z["study/velocity/av/raises"]) == "IndexError"


def _check(got, z, key):
    if f"{key}/raises" in z:
        raise AssertionError(f"{key}: the reference raises here")
    for i, k in enumerate(OUTS):
        w = z[f"{key}/{k}"]
        g = np.asarray(got[i])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (key, k)


def test_host_calculate_3dhist_equals_the_reference(z, studies):
    for tag, (st, labels) in studies.items():
        for param in A.PARAMS:
            for label in labels:
                key = f"{tag}/{param}/{label}"
                if f"{key}/raises" in z:
                    with pytest.raises(IndexError):
                        A.calculate_3dhist(st, param, label)
                else:
                    _check(A.calculate_3dhist(st, param, label), z, key)


def test_host_angle_mode_equals_the_reference(z, studies):
    for tag, (st, labels) in studies.items():
        for param in A.PARAMS:
            for label in labels:
                got = A.angle_mode_series(st, param, label)
                w = z[f"{tag}/{param}/{label}/ang_mode"]
                assert got.dtype == w.dtype and np.array_equal(got, w, equal_nan=True), (tag, param, label)


def test_unknown_param_or_label(studies, caplog):
    st = studies["study"][0]
    with caplog.at_level(logging.ERROR):
        assert A.calculate_3dhist(st, "speed", "rv") is None
        assert A.calculate_3dhist(st, "velocity", "lv") is None
    assert len([r for r in caplog.records if r.levelno == logging.ERROR]) == 2
    with pytest.raises(ValueError):
        A.angle_mode_series(st, "speed", "rv")
    with pytest.raises(ValueError):
        A.angle_mode_series(st, "velocity", "lv")


def test_tf_polar_project_param_rejects_bad_arguments_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    flow = np.zeros((3, 4, 4, 2), np.float16)
    m = np.zeros((3, 4, 4, 2), np.uint8)
    mm = np.zeros(4, np.float32)
    nz = np.zeros(4, np.int64)
    mode = np.zeros(2, np.float32)
    fake = C.create_string_buffer(64)                     # never dereferenced: every check comes before the handle is used
    good = dict(h=C.addressof(fake), flow=flow.ctypes.data, f16=1, N=3, n=2, H=4, W=4, m=m.ctypes.data, C=2, param=1, sp=0.02,
                f64=0, mag=None, ang=None, mm=mm.ctypes.data, nz=nz.ctypes.data, mode=mode.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_polar_project_param(a["h"], a["flow"], a["f16"], a["N"], a["n"], a["H"], a["W"], a["m"], a["C"], a["param"],
                                        a["sp"], a["f64"], a["mag"], a["ang"], a["mm"], a["nz"], a["mode"])

    assert call(h=None) == 1
    for bad in (dict(flow=None), dict(m=None), dict(mm=None), dict(nz=None), dict(mode=None), dict(N=0), dict(n=0), dict(H=0),
                dict(W=-2), dict(n=4), dict(C=0), dict(C=3), dict(param=-1), dict(param=3), dict(N=1, n=1),
                dict(N=1, n=1, param=2), dict(sp=0.0), dict(sp=float("inf")), dict(sp=float("nan"))):
        assert call(**bad) == 1, bad
    assert not mm.any() and not nz.any() and not mode.any()
