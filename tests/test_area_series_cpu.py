"""The area detector's per-frame series without a GPU: the host twin of analysis.area_series against
tests/golden/reference_area_series.npz (the area_list the reference's own AreaDetector.detect handed to its smoother, on a study file
opened by its own OpticalFlowDataset; make_reference_area_fixtures.py), the carry rule, the mask dtypes, and the argument checks of
tf_first_region_areas, which return before any GPU work.  Every comparison is integer equality."""
import ctypes as C
import logging
import os

import numpy as np
import pytest
from scipy import ndimage

import tee_optical_flow_amd as T
from tee_optical_flow_amd import analysis as A

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_area_series.npz")
H, W = 70, 150
# case -> the area the reference recorded for its frame (None: whatever frame 4's blob gave, carried)
CASE_AREA = {"blob": 327, "lone_pixel": 1, "carry": None, "diagonal": 308, "checker": 200, "two_values": 120, "value_255": 327,
             "border": 120, "full": H * W}


@pytest.fixture(scope="module")
def z():
    with np.load(FIX) as f:
        return {k: f[k] for k in f.files}


class BareStudy:
    """the least area_series reads: get_mask(label) and nframes"""

    def __init__(self, mask, nframes):
        self._mask, self.nframes = mask, nframes

    def get_mask(self, label):
        return self._mask


def test_fixture_holds_arrays_only_and_covers_the_cases(z):
    with np.load(FIX, allow_pickle=False) as f:                       # an object array would refuse to load
        assert sorted(f.files) == sorted(["mask", "nframes", "area"] + [f"case/{k}" for k in ["empty", *CASE_AREA]])
    m, n, area = z["mask"], int(z["nframes"]), z["area"]
    assert m.shape == (16, H, W, 2) and m.dtype == np.uint8 and n == 14 and area.shape == (14,) and area.dtype == np.int64
    assert np.array_equal(m[..., 1], (m[..., 0] == 0).astype(np.uint8))   # channel 1 differs from channel 0 everywhere
    assert os.path.getsize(FIX) <= os.path.getsize(os.path.join(os.path.dirname(FIX), "reference_study_stats.npz"))
    m0 = m[..., 0]
    assert z["case/empty"].tolist() == [0, 1] and not m0[:2].any() and area[0] == 0 and area[1] == 0
    for name, want in CASE_AREA.items():
        (f,) = z[f"case/{name}"].tolist()
        assert area[f] == (area[f - 1] if want is None else want), name
    full, cross = np.ones((3, 3), bool), ndimage.generate_binary_structure(2, 1)
    f = int(z["case/lone_pixel"][0])                                 # the first region is not the largest
    assert m0[f, 2, 2] == 1 and np.flatnonzero(m0[f])[0] == 2 * W + 2 and np.bincount(ndimage.label(m0[f], full)[0].ravel())[1:].max() == 327
    f = int(z["case/carry"][0])
    assert 0 < f < n - 1 and not m0[f].any() and m0[f - 1].any()
    f = int(z["case/diagonal"][0])                                   # the join sits on a 64 x 16 tile corner, the seed above it
    assert m0[f, 15, 63] and m0[f, 16, 64] and not m0[f, 15, 64] and not m0[f, 16, 63] and np.flatnonzero(m0[f])[0] == 5 * W + 50
    assert np.bincount(ndimage.label(m0[f], cross)[0].ravel())[1] == 154 and np.bincount(ndimage.label(m0[f], full)[0].ravel())[1:].max() == 600
    f = int(z["case/checker"][0])
    assert ndimage.label(m0[f, 8:28, 54:74], cross)[1] == 200 and np.bincount(ndimage.label(m0[f], full)[0].ravel())[1:].max() == 600
    f = int(z["case/two_values"][0])                                 # the seed's value is 2; the region of != 0 is larger
    assert m0[f].ravel()[np.flatnonzero(m0[f])[0]] == 2 and (m0[f] == 2).sum() == 120 and ndimage.label(m0[f], full)[1] == 1
    f = int(z["case/value_255"][0])
    assert set(np.unique(m0[f])) == {0, 255} and np.array_equal(m0[f] != 0, m0[int(z["case/blob"][0])] != 0)
    f = int(z["case/border"][0])
    assert m0[f, 0, 0] == 1 and m0[f, H - 1, W - 1] == 1
    assert m0[int(z["case/full"][0])].all()


def test_host_series_equals_the_reference(z):
    n = int(z["nframes"])
    st = A.FlowStudy(np.zeros((16, 2, 2, 2), np.float16), {"rv": z["mask"]}, 29.97)
    assert st.nframes == n
    for ds in (st, BareStudy(z["mask"], n), BareStudy(z["mask"], np.int64(n))):
        got = T.area_series(ds, "rv")
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (n,)
        assert np.array_equal(got, z["area"])
    assert np.array_equal(A.area_series(BareStudy(z["mask"][..., :1], n), "rv"), z["area"])     # one channel


def test_carry_rule(caplog):
    m = np.zeros((6, 5, 7, 1), np.uint8)
    m[1, 1:3, 2:5] = 1
    m[4, 0, 0] = 3
    m[4, 3:5, 3:7] = 3
    with caplog.at_level(logging.WARNING):
        got = A.area_series(BareStudy(m, 6), "x")
    assert got.tolist() == [0, 6, 6, 6, 1, 1]
    assert sum("area carried over" in r.message for r in caplog.records) == 4        # one per frame without a region
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        got = A.area_series(BareStudy(np.zeros((4, 3, 3, 2), bool), 3), "x")
    assert got.tolist() == [0, 0, 0] and got.dtype == np.int64
    assert sum("area carried over" in r.message for r in caplog.records) == 3
    assert A.area_series(BareStudy(m, 0), "x").shape == (0,)


def test_mask_dtypes_agree():
    rng = np.random.default_rng(11)
    b = rng.random((5, 23, 41, 2)) < 0.3
    b[2] = False
    want = A.area_series(BareStudy(b, 5), "x")
    assert want[2] == want[1] and want.min() >= 1
    for dt in (np.uint8, np.int64, np.float32):
        assert np.array_equal(A.area_series(BareStudy(b.astype(dt), 5), "x"), want), dt
    # and the twin's rule, restated with an explicit flood of equal values: region of the first non-zero pixel
    v = (rng.integers(0, 4, (3, 19, 30, 1)) * (rng.random((3, 19, 30, 1)) < 0.7)).astype(np.int64)
    got = A.area_series(BareStudy(v, 3), "x")
    for i in range(3):
        fr = v[i, :, :, 0]
        p = np.flatnonzero(fr)[0]
        lab, _ = ndimage.label(fr == fr.ravel()[p], structure=np.ones((3, 3), bool))
        assert got[i] == np.count_nonzero(lab == lab.ravel()[p])


def test_errors():
    with pytest.raises(ValueError):
        A.area_series(BareStudy(np.zeros((4, 5, 6), bool), 2), "x")
    with pytest.raises(ValueError):
        A.area_series(A.FlowStudy(np.zeros((4, 2, 2, 2)), {"rv": np.zeros((4, 2, 2, 2), bool)}, 30.0), "lv")   # get_mask gives None
    with pytest.raises(IndexError):
        A.area_series(BareStudy(np.zeros((4, 5, 6, 1), bool), 5), "x")


def test_tf_first_region_areas_rejects_bad_arguments_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    m = np.zeros((2, 4, 4, 2), np.uint8)
    area = np.zeros(2, np.int64)
    fake = C.create_string_buffer(64)            # never dereferenced: every check comes before the handle is used
    good = dict(h=C.addressof(fake), m=m.ctypes.data, N=2, H=4, W=4, C=2, area=area.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_first_region_areas(a["h"], a["m"], a["N"], a["H"], a["W"], a["C"], a["area"])

    assert call(h=None) == 1
    for bad in (dict(m=None), dict(area=None), dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=3)):
        assert call(**bad) == 1, bad
    assert not area.any()
    assert "tf_first_region_areas" in _lib.EXPORTED_SYMBOLS and callable(T.DenseFlow.first_region_areas)
