"""analysis.py's engine glue without a GPU: every analysis function given tests/numpy_engine.NumpyEngine -- whose device steps are the
package's own host twins, its histogram the device's rule and its select the device's radix walk -- against the same call without an
engine, np.array_equal with dtype and shape, on the committed studies.  What differs between the two routes is the glue alone: the
percentile ranks and _lerp, numpy's edge rules, the refusals, the reference's carry-over quirks, and which engine calls are taken for
arrays on the host and for a held study."""
import os

import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A
from tests.numpy_engine import NumpyEngine
from tests.overlay_cases import Recorder
from tests.stats_cases import nonfinite_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HELD_CALLS = {"held_av_centroids", "held_first_region_areas", "held_radlong_project_param", "held_polar_project_param", "held_radlong_overlay"}


def _echo(shape):
    """a float16 echo for the overlay (the fixtures have none): integers in [0, 255], as rgb2gray of 8-bit frames gives"""
    return np.random.default_rng(5).integers(0, 256, shape).astype(np.float16)


@pytest.fixture(scope="module")
def studies():
    """{name: (FlowStudy, labels, whether it has the 'rv' / 'av' masks of the rad/long functions)}"""
    with np.load(os.path.join(GOLD, "reference_study_stats.npz")) as f:
        flow, masks, fr = f["flow"], {"rv": f["rv"], "av": f["av"]}, f["frame_rate"][()]
    with np.load(os.path.join(GOLD, "reference_polar.npz")) as f:
        ss = A.FlowStudy(f["stress/flow"], {"all": f["stress/all"], "late": f["stress/late"]}, np.float64(f["stress/frame_rate"]),
                         nframes=int(f["stress/nframes"]))
    echo = _echo(flow.shape[:3])
    return {"study/float": (A.FlowStudy(flow, masks, float(fr), echo=echo, filename="glue"), ("rv", "av"), True),
            "study/float64": (A.FlowStudy(flow, masks, np.float64(fr), echo=echo, filename="glue"), ("rv", "av"), True),
            "stress": (ss, ("all", "late"), False)}


def _same(a, b, what):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        a, b = tuple(a[k] for k in sorted(a)), tuple(b[k] for k in sorted(b))
    if isinstance(a, tuple):
        assert isinstance(b, tuple) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
        return
    a, b = np.asarray(a), np.asarray(b)                       # (a list is the centroid list, or the edges of a study without angles)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, int((a != b).sum()))


def _results(ds, labels, radlong, engine):
    """[(name, result)] of every analysis function on `ds`; a call that raises gives the exception's type"""
    out = []

    def add(name, call):
        try:
            out.append((name, call()))
        except (IndexError, ValueError) as e:
            out.append((name + "/raises", type(e).__name__))

    if radlong:
        cent = A.av_centroids(ds.get_mask("av"), ds.nframes, engine=engine)
        out.append(("av_centroids", cent))
        add("av_centroids/nofilter", lambda: A.av_centroids(ds.get_mask("av"), ds.nframes, filter=False, engine=engine))
        for param in A.PARAMS:
            add(f"radlong/{param}", lambda: A.calculate_3dhist_radlong(ds, param, nbins=200, engine=engine))
            add(f"radlong/{param}/centroids", lambda: A.calculate_3dhist_radlong(ds, param, perc_lo=2.5, perc_hi=97.5, engine=engine, centroids=cent))
            add(f"overlay/{param}", lambda: A.radlong_overlay(ds, param, engine=engine, return_info=True))
        rec = Recorder()
        path = A.visualize_radlong(ds, "PWR", "unused_dir_of_the_recorder", engine=engine, centroids=cent, writer_factory=rec)
        out += [("video/frames", np.stack(rec.frames)), ("video/path", path), ("video/events", "".join(e[0] for e in rec.events))]
    for param in A.PARAMS:
        for label in labels:
            add(f"3dhist/{param}/{label}", lambda: A.calculate_3dhist(ds, param, label, nbins=300, engine=engine))
            add(f"angle_mode/{param}/{label}", lambda: A.angle_mode_series(ds, param, label, engine=engine))
    for label in labels:
        add(f"area/{label}", lambda: A.area_series(ds, label, engine=engine))
    return out


def _same_results(got, ref, what):
    assert [k for k, _ in got] == [k for k, _ in ref], what
    for (k, a), (_, b) in zip(got, ref):
        if k.endswith("/raises") or k in ("video/path", "video/events"):
            assert a == b, (what, k, a, b)
        else:
            _same(a, b, f"{what}: {k}")


@pytest.fixture(scope="module")
def host_results(studies):
    """the engine=None results, computed once"""
    return {name: _results(ds, labels, radlong, None) for name, (ds, labels, radlong) in studies.items()}


@pytest.mark.parametrize("name", ["study/float", "study/float64", "stress"])
def test_every_function_with_an_engine_equals_its_host_twin(studies, host_results, name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                               # (visualize_radlong makes its save_dir)
    ds, labels, radlong = studies[name]
    ref = host_results[name]
    raising = [k for k, _ in ref if k.endswith("/raises")]
    # the 'av' mask's first frame is empty: calculate_3dhist raises IndexError there, and nothing else raises
    assert raising == ([f"3dhist/{p}/av/raises" for p in A.PARAMS] if radlong else []) and all(v == "IndexError" for k, v in ref if k in raising)
    e = NumpyEngine()
    _same_results(_results(ds, labels, radlong, e), ref, name)
    assert not HELD_CALLS & set(e.calls) and {"polar_project_param", "first_region_areas", "radlong_hist", "radlong_select"} <= set(e.calls)
    if radlong:
        assert {"av_centroids", "radlong_project_param", "radlong_overlay"} <= set(e.calls)


@pytest.mark.parametrize("name", ["study/float", "study/float64"])
def test_a_held_study_gives_the_same_through_the_held_calls_alone(studies, host_results, name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ds, labels, radlong = studies[name]
    e = NumpyEngine()
    hs = A.HeldStudy.from_study(e, ds)
    assert e.calls == ["hold_study", "hold_mask", "hold_mask"] and hs.nframes == ds.nframes and hs.accepted_labels == list(labels)
    del e.calls[:]
    _same_results(_results(hs, labels, radlong, e), host_results[name], f"held {name}")
    assert set(e.calls) == HELD_CALLS | {"radlong_hist", "radlong_select"}


def test_radlong_stats_device_equals_the_host_statistics(studies):
    ds = studies["study/float64"][0]
    n = ds.nframes
    cent = A.av_centroids(ds.get_mask("av"), n)
    field = A.param_field(ds.flow, ds.get_mask("rv"), "PWR", ds.frame_rate, n)
    e = NumpyEngine()
    _same(A.radlong_stats_device(e, field, cent, nbins=100, return_arrays=True),
          A.param_radlong_stats(ds.flow, ds.get_mask("rv"), "PWR", ds.frame_rate, n, cent, nbins=100, return_arrays=True), "radlong_stats_device")
    assert e.calls[0] == "radlong_project" and set(e.calls[1:]) == {"radlong_hist", "radlong_select"}


@pytest.mark.parametrize("case", nonfinite_cases(), ids=lambda c: c.name)
def test_non_finite_flow_raises_on_the_engine_route_what_the_host_twin_raises(case):
    e = NumpyEngine()
    if case.path == "radlong":
        kw = dict(perc_lo=case.perc_lo, perc_hi=case.perc_hi, nbins=case.nbins)
        args = (case.flow, case.mask, case.param, case.frame_rate, case.n_used, case.cent)
        calls = [lambda: A.param_radlong_stats(*args, **kw), lambda: A.param_radlong_stats(*args, engine=e, **kw),
                 lambda: A.radlong_stats_device(e, case.field(), case.cent, **kw)]
    else:
        st = case.study()
        calls = [lambda eng=eng: A.calculate_3dhist(st, case.param, "m", nbins=case.nbins, percentile=case.percentile, engine=eng) for eng in (None, e)]
    raised = []
    for call in calls:
        with pytest.raises(Exception) as ei:
            call()
        raised.append(type(ei.value))
    assert raised == [case.raises] * len(calls)
    assert "radlong_hist" not in e.calls and "radlong_select" not in e.calls      # refused before the device histogram would run
