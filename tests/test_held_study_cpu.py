"""The host side of a held study without a GPU or the library: which path the analysis functions take for a HeldStudy (the held
calls, and only for the engine that holds it), what they raise otherwise, and the label -> slot bookkeeping of DenseFlow."""
import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.dense_flow import HeldShape, _HeldLabels
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError


class FakeEngine:
    """what the analysis functions use of a DenseFlow that holds a study: `held` and the held_* calls, which record their arguments;
    every host-pointer call fails the test"""

    def __init__(self, n=14, H=6, W=7):
        self.shape = HeldShape(n, H, W, n, 3, {"rv": (n, 2), "av": (n, 1)})
        self.calls = []

    @property
    def held(self):
        return self.shape

    def held_av_centroids(self, label, n):
        self.calls.append(("held_av_centroids", label, n))
        cent = np.stack([np.arange(n) + 0.5, np.arange(n) * 2.0], 1)
        area = np.full(n, 5, np.int64)
        area[1] = 0                                           # an empty frame: the previous centroid is carried over
        return cent, area

    def held_first_region_areas(self, label, n):
        self.calls.append(("held_first_region_areas", label, n))
        area = np.arange(n, dtype=np.int64) + 3
        area[0] = 0
        return area

    def held_polar_project_param(self, label, param, spacing, grad_f64, n_used, return_arrays=False):
        self.calls.append(("held_polar_project_param", label, param, spacing, grad_f64, n_used))
        return np.array([0, 1, 0, 6], np.float32), np.ones((n_used, 2), np.int64), np.linspace(0.5, 6, n_used).astype(np.float32), None, None

    def __getattr__(self, name):                              # av_centroids, first_region_areas, polar_project_param, ...
        raise AssertionError(f"the host-pointer call {name} was taken for a held study")


def test_the_held_calls_are_taken_for_the_owning_engine():
    e = FakeEngine()
    hs = A.HeldStudy(e, np.float64(50.0))
    assert hs.nframes == 12 and hs.generation == 3 and hs.shape == (14, 6, 7) and hs.n_echo == 14
    assert hs.accepted_labels == ["rv", "av"]
    m = hs.get_mask("av")
    assert isinstance(m, A.HeldMask) and m.label == "av" and m.shape == (14, 6, 7, 1) and hs.get_mask("lv") is None
    cent = A.av_centroids(m, 12, filter=False, engine=e)
    assert e.calls[-1] == ("held_av_centroids", "av", 12)
    assert cent[0] == (0.5, 0.0) and cent[1] == cent[0] and cent[2] == (2.5, 4.0)
    assert A.av_centroids(hs, 5, filter=False, engine=e) == cent[:5] and e.calls[-1] == ("held_av_centroids", "av", 5)
    area = A.area_series(hs, "rv", engine=e)
    assert e.calls[-1] == ("held_first_region_areas", "rv", 12)
    assert area.tolist() == [0] + list(range(4, 15))
    mode = A.angle_mode_series(hs, "PWR", "rv", engine=e)
    assert e.calls[-1] == ("held_polar_project_param", "rv", 2, 1 / np.float64(50.0), A.gradient_is_f64(np.float64(50.0)), 12)
    assert mode.dtype == np.float32 and mode.shape == (12,)
    with pytest.raises(IndexError):
        A.av_centroids(m, 15, engine=e)
    with pytest.raises(ValueError, match="not a valid key"):
        A.angle_mode_series(hs, "velocity", "lv", engine=e)


def _every_function(hs, engine):
    return [lambda: A.calculate_3dhist_radlong(hs, "velocity", engine=engine), lambda: A.calculate_3dhist(hs, "velocity", "rv", engine=engine),
            lambda: A.angle_mode_series(hs, "velocity", "rv", engine=engine), lambda: A.area_series(hs, "rv", engine=engine),
            lambda: A.av_centroids(hs, 3, engine=engine), lambda: A.av_centroids(A.HeldMask(hs, "av", (14, 6, 7, 1)), 3, engine=engine),
            lambda: A.radlong_overlay(hs, "velocity", engine=engine),
            lambda: A.visualize_radlong(hs, "velocity", "nowhere", engine=engine, writer_factory=lambda *a, **k: None)]


def test_no_engine_or_another_engine_raises():
    e, other = FakeEngine(), FakeEngine()
    hs = A.HeldStudy(e, 50.0)
    for call in _every_function(hs, None):
        with pytest.raises(ValueError, match="there is no host path"):
            call()
    for call in _every_function(hs, other):
        with pytest.raises(ValueError, match="another engine"):
            call()
    assert e.calls == [] and other.calls == []


def test_a_stale_generation_raises():
    e = FakeEngine()
    hs = A.HeldStudy(e, 50.0)
    e.shape = e.shape._replace(generation=4)                  # replaced
    for call in _every_function(hs, e):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    assert hs.accepted_labels == []
    e.shape = None                                            # released
    for call in _every_function(hs, e):
        with pytest.raises(RuntimeError, match="stale"):
            call()
    with pytest.raises(ValueError, match="holds no study"):
        A.HeldStudy(e, 50.0)
    assert e.calls == []


def test_from_study_takes_the_files_types_only():
    class Holder(FakeEngine):
        def hold_study(self, flow, echo=None):
            self.calls.append(("hold_study", flow.dtype, None if echo is None else echo.dtype))

        def hold_mask(self, label, mask):
            self.calls.append(("hold_mask", label))
    e = Holder()
    flow = np.zeros((14, 6, 7, 2), np.float16)
    masks = {"rv": np.ones((14, 6, 7, 2), bool), "av": np.ones((14, 6, 7, 1), bool)}
    hs = A.HeldStudy.from_study(e, A.FlowStudy(flow, masks, 25.0, nframes=9, echo=np.ones((14, 6, 7), np.float16), filename="f"))
    assert e.calls == [("hold_study", np.float16, np.float16), ("hold_mask", "rv"), ("hold_mask", "av")]
    assert (hs.nframes, hs.frame_rate, hs.filename, hs.mode) == (9, 25.0, "f", "RVIO_2class")
    with pytest.raises(ValueError, match="float16"):
        A.HeldStudy.from_study(e, A.FlowStudy(flow.astype(np.float32), masks, 25.0))
    with pytest.raises(ValueError, match="float16"):
        A.HeldStudy.from_study(e, A.FlowStudy(flow, masks, 25.0, echo=np.ones((14, 6, 7), np.uint8)))


def test_labels_map_to_slots_and_a_13th_raises():
    hl = _HeldLabels()
    hl.sync(1)
    assert [hl.slot_for(f"m{i}") for i in range(12)] == list(range(12))
    assert hl.slot_for("m3") == 3 and hl.slot_of("m11") == 11       # a label held already keeps its slot
    with pytest.raises(OpticalFlowCalculationError, match="no slot left for label 'm12'"):
        hl.slot_for("m12")
    assert len(hl.slots) == 12
    with pytest.raises(OpticalFlowCalculationError, match="no mask is held under label 'rv'"):
        hl.slot_of("rv")
    hl.sync(1)                                                # the same study: nothing is forgotten
    assert hl.slot_of("m5") == 5
    hl.sync(2)                                                # replaced or released: every label goes
    assert hl.slots == {} and hl.slot_for("rv") == 0
