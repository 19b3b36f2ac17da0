"""The magnitude overlay (the reference's single-component video, example_peak_plots.py:459-513) without a GPU: the numpy twin equals
tests/golden/reference_single_overlay.npz, the frames the reference's own example handed to its video writer, byte for byte; its norm
and lookup equal matplotlib's own Normalize and colormap where matplotlib is importable; the shipped 'hot' table equals matplotlib's;
analysis.magnitude_overlay's engine glue, on a numpy engine, equals the twin on host arrays and on a held study; every refusal; the
video writer protocol.  No tolerance anywhere."""
import logging

import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A

from tests.numpy_engine_magnitude import MagnitudeNumpyEngine
from tests.single_overlay_cases import FIXTURE_CASES, Recorder, cases, every_index_field, fixture_study, hot, load_fixture, tie_case


@pytest.fixture(scope="module")
def z():
    return load_fixture()


@pytest.fixture(scope="module")
def all_cases():
    return cases()


def _host(st, param, **kw):
    return A.magnitude_overlay(st, param, "rv", return_info=True, **kw)


@pytest.mark.parametrize("case", FIXTURE_CASES)
def test_twin_equals_the_reference_frames(z, case):
    name, param = case.split("/")
    st = fixture_study(z, name)
    out, info, finfo = _host(st, param, norm_f64=False)
    ref = z[f"{case}/frames"]
    assert out.dtype == np.uint8 and out.shape == ref.shape
    assert np.array_equal(out, ref), (case, int((out != ref).sum()))
    N = st.flow.shape[0]
    mag = np.sqrt((A.param_field(st.flow, st.masks["rv"], param, st.frame_rate, N) ** 2).sum(-1, dtype=np.float64))
    if name == "main":
        assert mag[st.nframes:].max() > mag[:st.nframes].max()         # the norm's range comes from the frames that are not rendered
    if name == "full":
        assert info[0] > 0
        # the other division rule gives another t in this case (the file carries the float32-divisor rule)
        field = A.param_field(st.flow, st.masks["rv"], param, st.frame_rate, N)
        m = np.sqrt(field[..., 0] ** 2 + field[..., 1] ** 2)
        assert any((A.magnitude_norm_index(m[i], info[0], info[1], False)[0] != A.magnitude_norm_index(m[i], info[0], info[1], True)[0]).any()
                   for i in range(st.nframes))
    if name == "emptymask":
        assert finfo[1, 1] == hot()[0].max() and (out[1, ..., 1] == out[1, ..., 2]).all()
    if name == "zeroecho":
        assert finfo[2, 0] == 0
    assert finfo.shape == (st.nframes, 2)


def test_the_fixture_shows_the_half_round_trip(z):
    assert int(z["main/half_changed"]) > 0 and int(z["full/t_differs"]) > 0


def test_shipped_hot_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps["hot"]
    assert cmap.N == 256
    assert np.array_equal(A.committed_magnitude_luts()["hot"], np.array(cmap(np.arange(256))[:, :3], np.float64))
    assert list(A.committed_magnitude_luts()) == ["hot"]
    assert np.array_equal(A.magnitude_colormap_lut("hot"), A.committed_magnitude_luts()["hot"])
    assert A.committed_magnitude_luts()["hot"][0, 0] > 0               # row 0 is not black


def test_hot_without_matplotlib(monkeypatch):
    import builtins
    real = builtins.__import__

    def no_mpl(name, *a, **k):
        if name.split(".")[0] == "matplotlib":
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_mpl)
    assert np.array_equal(A.magnitude_colormap_lut("hot"), A.committed_magnitude_luts()["hot"])
    assert np.array_equal(A.magnitude_colormap_lut("bwr"), A.committed_colormap_luts()["bwr"])
    with pytest.raises(ValueError, match="not among the committed"):
        A.magnitude_colormap_lut("jet")


@pytest.mark.parametrize("vmin_zero", [True, False])
def test_norm_and_lookup_equal_matplotlib(vmin_zero):
    matplotlib = pytest.importorskip("matplotlib")
    import matplotlib.colors
    rng = np.random.default_rng(3 + vmin_zero)
    mag = np.abs(rng.normal(0, 3, (4, 37, 53))).astype(np.float32) + (0 if vmin_zero else np.float32(0.3))
    if vmin_zero:
        mag[:, 5:9] = 0
    norm = matplotlib.colors.Normalize(vmin=np.min(mag), vmax=np.max(mag))
    cmap = matplotlib.colormaps["hot"]
    lut = A.magnitude_colormap_lut("hot")
    f64 = A.norm_is_f64()
    for i in range(4):
        t_ref = norm(mag[i])
        t, idx = A.magnitude_norm_index(mag[i], np.min(mag), np.max(mag), f64)
        assert t_ref.dtype == np.float32 and np.array_equal(np.asarray(t_ref), t)
        assert np.array_equal(cmap(t_ref)[..., :3], lut[idx])
    assert (np.min(mag) == 0) == vmin_zero


def test_norm_rules_and_edges():
    _, x = every_index_field()
    for f64 in (False, True):
        t, idx = A.magnitude_norm_index(x, 0, 64, f64)
        assert sorted(set(idx.ravel())) == list(range(256)) and idx[x == 64] == 255 and t.max() == 1
        t, idx = A.magnitude_norm_index(x, 5, 5, f64)
        assert not t.any() and not idx.any()
    # the probe's own numbers: (1 + 2^-22) / (1 + 2^-24) by the two rules; the probe says which one this numpy follows
    s, d = np.array([1 + 2.0 ** -22], np.float32), np.float64(1 + 2.0 ** -24)
    by_f64, by_f32 = (s.astype(np.float64) / d).astype(np.float32)[0], (s / np.float32(d))[0]
    assert by_f64 == np.float32(1 + 2.0 ** -23) and by_f32 == np.float32(1 + 2.0 ** -22)
    q = s.copy()
    q /= d
    assert q[0] == (by_f64 if A.norm_is_f64() else by_f32)


def test_tie_case_hits_ties():
    st, lut, ties, mid, v = tie_case()
    assert ties > 100
    out, info, finfo = _host(st, "velocity", colormap=lut)
    assert finfo[0, 0] == 0 and finfo[0, 1] == 1 and tuple(info) == (0, 64)
    hit = v == mid
    # rows 0..254 are pixels 0..254 of the frame; a tie just below an integer goes up to it, one just above goes down to it
    px = out.reshape(-1, 3)[:255]
    assert np.array_equal(px[hit[:, 0], 0], np.ceil(mid[hit[:, 0], 0]).astype(np.uint8))
    assert np.array_equal(px[hit[:, 1], 1], np.floor(mid[hit[:, 1], 1]).astype(np.uint8))
    assert np.array_equal(px[hit[:, 2], 2], np.ceil(mid[hit[:, 2], 2]).astype(np.uint8))
    assert (px[hit[:, 0], 0] != v[hit[:, 0], 0].astype(np.uint8)).all()       # the direct cast truncates to the integer below


def test_glue_on_the_numpy_engine_equals_the_twin(all_cases):
    for name, st, param, kw, _ in all_cases:
        host = _host(st, param, **kw)
        eng = MagnitudeNumpyEngine()
        dev = A.magnitude_overlay(st, param, "rv", return_info=True, engine=eng, **kw)
        assert eng.calls == ["magnitude_overlay"], name
        for a, b in zip(dev, host):
            assert np.array_equal(a, b), name
        if st.flow.dtype == np.float16 and st.echo.dtype == np.float16:
            held = A.HeldStudy.from_study(eng, st)
            dev = A.magnitude_overlay(held, param, "rv", return_info=True, engine=eng, **kw)
            assert eng.calls[-1] == "held_magnitude_overlay", name
            for a, b in zip(dev, host):
                assert np.array_equal(a, b), name
        assert np.array_equal(A.magnitude_overlay(st, param, "rv", **kw), host[0])


def test_quirks_of_the_cases(all_cases):
    by = {c[0]: c for c in all_cases}
    _, st, param, kw, _ = by["constant-magnitude"]
    out, info, finfo = _host(st, param, **kw)
    assert info[0] == info[1] > 0 and (finfo[:, 1] == hot()[0].max()).all()
    _, st, param, kw, _ = by["black-row"]
    out, info, finfo = _host(st, param, **kw)
    assert finfo[1, 1] == 0 and finfo[0, 1] > 0
    _, st, param, kw, _ = by["echo-subnormal-and-65504"]
    out, info, finfo = _host(st, param, **kw)
    assert 0 < finfo[0, 0] < 6.2e-5 and finfo[1, 0] == 65504
    _, st, param, kw, _ = by["every-index"]
    field = A.param_field(st.flow, st.masks["rv"], param, st.frame_rate, 1)
    idx = A.magnitude_norm_index(np.sqrt(field[0, ..., 0] ** 2 + field[0, ..., 1] ** 2), 0, 64, False)[1]
    assert sorted(set(idx.ravel())) == list(range(256))


def test_refusals(z, caplog):
    st = fixture_study(z, "main")
    with caplog.at_level(logging.ERROR):
        assert A.magnitude_overlay(st, "speed", "rv") is None
        assert A.magnitude_overlay(st, "velocity", "lv") is None
        st.mode = "otsu"
        assert A.magnitude_overlay(st, "velocity", "rv") is None
        st.mode = "RVIO_2class"
        st.echo = None
        assert A.magnitude_overlay(st, "velocity", "rv") is None
        assert A.visualize_magnitude(st, "velocity", "rv", "/nonexistent/never-made") is None
    assert len(caplog.records) >= 5
    for v in (np.nan, np.inf, -1.0):
        bad = fixture_study(z, "main")
        bad.echo = bad.echo.copy()
        bad.echo[bad.nframes - 1, 3, 4] = v
        with pytest.raises(ValueError, match="negative or non-finite"):
            A.magnitude_overlay(bad, "velocity", "rv")
    bad = fixture_study(z, "main")
    bad.echo = bad.echo.copy()
    bad.echo[bad.nframes, 3, 4] = np.nan                              # past the frames rendered: not read
    assert A.magnitude_overlay(bad, "velocity", "rv") is not None
    bad = fixture_study(z, "main")
    bad.flow = bad.flow.astype(np.float32)
    bad.flow[bad.flow.shape[0] - 1, 15, 22, 0] = np.inf                # in a frame that is not rendered: the range is over all of them
    with pytest.raises(ValueError, match="NaN or inf"):
        A.magnitude_overlay(bad, "velocity", "rv")
    for echo in (st.flow[..., 0].astype(np.float32), fixture_study(z, "main").echo[:2], fixture_study(z, "main").echo[:, :4]):
        bad = fixture_study(z, "main")
        bad.echo = echo
        with pytest.raises(ValueError, match="echo must be"):
            A.magnitude_overlay(bad, "velocity", "rv")
    bad = fixture_study(z, "main")
    bad.masks["rv"] = bad.masks["rv"][:bad.nframes]
    with pytest.raises(ValueError, match="fewer than the flow"):
        A.magnitude_overlay(bad, "velocity", "rv")
    good = fixture_study(z, "main")
    for lut in (np.zeros((200, 3)), -hot(), np.where(hot() == hot()[0, 0], np.inf, hot())):
        with pytest.raises(ValueError):
            A.magnitude_overlay(good, "velocity", "rv", colormap=lut)
    with pytest.raises(ValueError):
        A.magnitude_overlay(good, "velocity", "rv", colormap="no-such-colormap")
    # a held study without an engine, and one without echo
    eng = MagnitudeNumpyEngine()
    held = A.HeldStudy.from_study(eng, good)
    with pytest.raises(ValueError, match="engine"):
        A.magnitude_overlay(held, "velocity", "rv")
    good.echo = None
    held = A.HeldStudy.from_study(eng, good)
    with caplog.at_level(logging.ERROR):
        assert A.magnitude_overlay(held, "velocity", "rv", engine=eng) is None
    with pytest.raises(ValueError):
        A.magnitude_overlay_host(np.zeros((2, 3, 3, 2), np.float64), 1, np.zeros((2, 3, 3), np.uint8), hot())
    with pytest.raises(ValueError):
        A.magnitude_overlay_host(np.zeros((2, 3, 3, 2), np.float32), 3, np.zeros((2, 3, 3), np.uint8), hot())


def test_video_writer_protocol(z, tmp_path):
    for engine in (None, MagnitudeNumpyEngine()):
        rec = Recorder()
        st = fixture_study(z, "main")
        path = A.visualize_magnitude(st, "PWR", "rv", str(tmp_path / "videos"), fps=24, norm_f64=False, engine=engine, writer_factory=rec)
        assert path == rec.path and path.endswith(str(z["main/PWR/path"])) and rec.fps == int(z["main/PWR/fps"])
        assert rec.events == ["append"] * st.nframes + ["close"]
        assert np.array_equal(np.stack(rec.frames), z["main/PWR/frames"])
    assert str(z["main/PWR/path"]) == "main_rv_PWR_single_overlay.mp4"
