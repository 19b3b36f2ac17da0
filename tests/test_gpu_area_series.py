"""The area detector's per-frame series on the device (tf_first_region_areas; DenseFlow.first_region_areas;
analysis.area_series(ds, label, engine=)): identical to tests/golden/reference_area_series.npz, which the reference's own
AreaDetector.detect produced, and to the host twin on frames made to break a tiled 8-connected labeller, on masks of several values,
in chunks, in turns with the other calls that label in the same device scratch, and on random masks.  Every comparison is integer
equality."""
import os

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib, analysis as A, masks
from tests.labelling_cases import stress_frames
from tests.test_masks_cpu import _Cfg, fixture_cases

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_area_series.npz")


@pytest.fixture(scope="module")
def z():
    with np.load(FIX) as f:
        return {k: f[k] for k in f.files}


class BareStudy:
    def __init__(self, mask, nframes):
        self._mask, self.nframes = mask, nframes

    def get_mask(self, label):
        return self._mask


def _host(m):
    """the host twin's raw areas of a stack [N,H,W,C]: 0 for a frame without a region"""
    return np.array([A._first_region_area(m[i, :, :, 0]) or 0 for i in range(m.shape[0])], np.int64)


def _with_channels(m0, Cn):
    """[N,H,W] uint8 or bool -> [N,H,W,Cn], channel 1 the complement of channel 0"""
    return m0[..., None] if Cn == 1 else np.stack([m0, (m0 == 0).astype(m0.dtype)], axis=-1)


def test_fixture_through_the_engine(engine, z):
    n = int(z["nframes"])
    got = engine.first_region_areas(z["mask"][:n])
    assert got.dtype == np.int64 and got.shape == (n,)
    raw = z["area"].copy()
    raw[int(z["case/carry"][0])] = 0                                          # the call reports an empty frame as 0; the caller carries
    assert np.array_equal(got, raw)
    st = A.FlowStudy(np.zeros((16, 2, 2, 2), np.float16), {"rv": z["mask"]}, 29.97)
    for ds in (st, BareStudy(z["mask"], n), BareStudy(z["mask"][..., :1], n)):
        s = T.area_series(ds, "rv", engine=engine)
        assert s.dtype == np.int64 and np.array_equal(s, z["area"])
    assert np.array_equal(engine.first_region_areas(z["mask"]), _host(z["mask"]))      # all 16 frames
    # a mask the device call does not take runs on the host twin, whatever the engine
    assert np.array_equal(A.area_series(BareStudy(z["mask"].astype(np.int64), n), "rv", engine=engine), z["area"])


def test_labelling_stress_equals_the_host_twin(engine):
    for name, fr in stress_frames().items():
        H, W = fr.shape
        bands = np.where(fr, 1 + (np.arange(W)[None, :] // 8) % 2, 0).astype(np.uint8)   # every other 8-pixel column band has value 2
        for form, f0 in (("bool", fr), ("255", fr.astype(np.uint8) * 255), ("bands", bands)):
            m0 = np.stack([f0, f0[::-1, ::-1]]) if H > 1 or W > 1 else f0[None]
            want = _host(m0[..., None])
            for Cn in (1, 2):
                got = engine.first_region_areas(_with_channels(m0, Cn))
                assert np.array_equal(got, want), (name, form, Cn, got, want)
            if form == "bands" and name == "full":
                assert want.tolist() == [H * 8, H * 2]                         # the bands do cut the region: columns [0, 8) and [128, 130) flipped


def test_first_region_is_not_the_largest(engine, z):
    f = int(z["case/lone_pixel"][0])
    m = z["mask"][f:f + 1]
    assert engine.first_region_areas(m).tolist() == [1]
    _, area = engine.av_centroids(m)
    assert area.tolist() == [327] and A._largest_component(m[0, :, :, 0])[1] == 327


def test_a_study_of_several_chunks():
    """Frames go through in chunks of at most 512 MiB of masks and labelling scratch, which no test-sized study fills: the
    area_chunk_kib knob shrinks the chunk.  7 frames of 37 x 53 take 6 + C bytes per pixel, 13.4 (C = 1) or 15.3 KiB (C = 2) a frame:
    16 KiB = one frame per chunk, 32 KiB = 2, 2, 2, 1, 48 KiB = 3, 3, 1; 1 KiB = less than a frame, so one at a time; 0 = the default."""
    rng = np.random.default_rng(7)
    m0 = (rng.integers(1, 4, (7, 37, 53)) * (rng.random((7, 37, 53)) < 0.55)).astype(np.uint8)
    m0[3] = 0
    m0[6, :, :] = 2
    eng = T.DenseFlow(device_id=0)
    try:
        for Cn in (1, 2):
            m = _with_channels(m0, Cn)
            want = _host(m)
            assert want[3] == 0 and want[6] == 37 * 53
            for kib in (0, 16, 32, 48, 1, 0):
                eng.set_tuning("area_chunk_kib", kib)
                assert np.array_equal(eng.first_region_areas(m), want), (Cn, kib)
    finally:
        eng.close()


def test_calls_that_share_the_labelling_scratch_do_not_see_each_other(engine):
    """tf_first_region_areas labels in the parents and tile-local roots tf_av_centroids and tf_clean_masks use, and keeps its mask and
    output in tf_av_centroids' slots: in turns on one handle, large and small, each call repeats its own first result."""
    frames = stress_frames()
    _, arr, mode, min_size, keys, _ = {c[0]: c for c in fixture_cases()}["rvio_9x37x53_min5"]
    big = np.repeat(np.stack([frames["snake"], frames["snake"][::-1, ::-1]])[..., None], 2, axis=3)      # 2 x 61 x 200
    small = np.repeat(frames["single_pixel"][None, :, :, None], 2, axis=3)                                # 37 x 70
    stair = frames["staircase"][None, :, :, None]                                                         # 70 x 200

    calls = {
        "areas_big": lambda: engine.first_region_areas(big),
        "cent_big": lambda: np.concatenate([a.ravel() for a in engine.av_centroids(big)]),
        "clean": lambda: np.stack([v for v in masks.clean_mask(arr, mode, config=_Cfg(min_size), engine=engine).values()]),
        "areas_small": lambda: engine.first_region_areas(small),
        "cent_stair": lambda: np.concatenate([a.ravel() for a in engine.av_centroids(stair)]),
        "areas_stair": lambda: engine.first_region_areas(stair),
    }
    first = {k: f() for k, f in calls.items()}
    assert np.array_equal(first["areas_big"], _host(big)) and np.array_equal(first["areas_stair"], _host(stair))
    assert first["areas_small"].tolist() == [1]
    for k in ("areas_stair", "clean", "areas_small", "cent_big", "areas_big", "cent_stair", "areas_small", "clean", "areas_big"):
        assert np.array_equal(calls[k](), first[k]), k


def test_random_masks_equal_the_host_twin(engine):
    rng = np.random.default_rng(20261019)
    for case in range(300):
        N, H, W = int(rng.integers(1, 10)), int(rng.integers(1, 81)), int(rng.integers(1, 201))
        density, nval, Cn = rng.uniform(0.02, 0.95), int(rng.integers(1, 4)), int(rng.integers(1, 3))
        vals = rng.choice(np.arange(1, 256), nval, replace=False)
        m0 = (vals[rng.integers(0, nval, (N, H, W))] * (rng.random((N, H, W)) < density)).astype(np.uint8)
        m = _with_channels(m0, Cn)
        got, want = engine.first_region_areas(m), _host(m)
        assert np.array_equal(got, want), (case, N, H, W, density, nval, Cn, got, want)


def test_invalid_arguments_leave_the_handle_usable(engine, z):
    L, h = engine._L, engine._h
    m = np.ascontiguousarray(z["mask"][2:4])
    area = np.full(2, -7, np.int64)
    good = dict(h=h, m=m.ctypes.data, N=2, H=70, W=150, C=2, area=area.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_first_region_areas(a["h"], a["m"], a["N"], a["H"], a["W"], a["C"], a["area"])

    for bad in (dict(h=None), dict(m=None), dict(area=None), dict(N=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=3)):
        assert call(**bad) == _lib.TF_ERR_INVALID_ARG, bad
    assert call(N=1, H=65536, W=32768) == _lib.TF_ERR_UNSUPPORTED              # 2^31 pixels a frame: refused before the masks are read
    assert b"tf_first_region_areas" in L.tf_last_error(h)
    assert (area == -7).all()
    with pytest.raises(T.OpticalFlowCalculationError):
        engine.first_region_areas(z["mask"].astype(np.int32))
    with pytest.raises(T.OpticalFlowCalculationError):
        engine.first_region_areas(np.zeros((2, 4, 4, 3), np.uint8))
    assert call() == _lib.TF_OK and area.tolist() == z["area"][2:4].tolist() == [327, 1]
