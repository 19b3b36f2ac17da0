"""A study held on the device (tf_hold_study, tf_hold_mask, tf_hold_next, the tf_held_* calls; DenseFlow.hold_study & co.;
analysis.HeldStudy): every held tail call against its host-pointer original on the same arrays, np.array_equal and no tolerance.  The
yardstick is the originals, which the reference fixtures pin; the held path is never compared with itself.  Small frames (40 x 52 and
the odd 37 x 53, where every second flow of the payload starts on an odd 4-byte word), 8 frames, sub-batches of 3 pairs so that the 7
pairs of a solve cross sub-batches on the lanes."""

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests.overlay_cases import Recorder

pytestmark = pytest.mark.gpu

N = 8
SHAPES = [(40, 52), (37, 53)]
LUT_RAD, LUT_LONG = A.committed_colormap_luts()["bwr"], A.committed_colormap_luts()["BrBG"]
SPACING = 1 / 50.0


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0, max_batch=3)
    yield e
    e.close()


def _frames(n, H, W, seed=0):
    from tee_optical_flow_amd.synth import speckle_sequence
    return np.ascontiguousarray(np.repeat(speckle_sequence(seed + n * 1000 + H + W, n, H, W)[..., None], 3, axis=3))


def _masks(n, H, W, Cm, seed=0):
    """{'rv': a drifting disc, 'av': two blobs of different size}, bool [n,H,W,Cm]"""
    yy, xx = np.mgrid[:H, :W]
    rv = np.zeros((n, H, W), bool)
    av = np.zeros((n, H, W), bool)
    for f in range(n):
        rv[f] = ((yy - H / 2 - f / 3) / (0.35 * H)) ** 2 + ((xx - W / 2 + f / 3 + seed) / (0.4 * W)) ** 2 < 1
        av[f] = ((yy - H / 3 - f / 2) ** 2 + (xx - W / 3) ** 2 < 30 + f) | ((yy - 3 * H / 4) ** 2 + (xx - 3 * W / 4 + seed) ** 2 < 9)
    return {k: np.ascontiguousarray(np.repeat(m[..., None], Cm, axis=3)) for k, m in (("rv", rv), ("av", av))}


def _payload(seed, n, H, W):
    """(flow16 [n,H,W,2] quiet in frame 0, echo16 [n,H,W])"""
    rng = np.random.default_rng(seed)
    amp = np.concatenate([[0.5], rng.uniform(1, 6, n - 1)])[:, None, None, None]
    flow = (rng.normal(0, 1, (n, H, W, 2)) * amp).astype(np.float16)
    echo = rng.integers(1, 256, (n, H, W)).astype(np.float16)
    return flow, echo


def _bkgd(H, W, seed):
    return np.random.default_rng(seed).random((2, H, W, 2)) < 0.3


def _same(a, b, what):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(b)]
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (what, int((a != b).sum()))


def _tail(e, n, grad_f64, held, flow=None, masks=None, echo=None):
    """The whole tail for frames [0, n): [(name, result)] from the held calls, or from the originals on the given arrays."""
    out = []
    cent, area = e.held_av_centroids("av", n) if held else e.av_centroids(masks["av"][:n])
    out += [("centroids", cent), ("areas", area)]
    out.append(("first_region_areas", e.held_first_region_areas("rv", n) if held else e.first_region_areas(masks["rv"][:n])))
    for p, name in enumerate(A.PARAMS):
        if held:
            mm, nz, rad, lon = e.held_radlong_project_param("rv", p, SPACING, grad_f64, n, cent, return_arrays=True)
        else:
            mm, nz, rad, lon = e.radlong_project_param(flow, masks["rv"], p, SPACING, grad_f64, n, cent, return_arrays=True)
        out += [(f"radlong/{name}/{k}", v) for k, v in (("minmax", mm), ("nonzero", nz), ("rad", rad), ("long", lon))]
        st = A._radlong_stats_resident(e, n, mm, nz, 1, 99, 40)               # tf_radlong_hist and tf_radlong_select on the planes
        out += [(f"radlong/{name}/{k}", st[k]) for k in ("radial", "longitudinal")]
        frames, info = e.held_radlong_overlay(LUT_RAD, LUT_LONG) if held else e.radlong_overlay(echo, LUT_RAD, LUT_LONG)
        out += [(f"overlay/{name}/frames", frames), (f"overlay/{name}/info", info)]
    for p, name in enumerate(A.PARAMS):
        if held:
            mm, nz, mode, mag, ang = e.held_polar_project_param("rv", p, SPACING, grad_f64, n, return_arrays=True)
        else:
            mm, nz, mode, mag, ang = e.polar_project_param(flow, masks["rv"], p, SPACING, grad_f64, n, return_arrays=True)
        out += [(f"polar/{name}/{k}", v) for k, v in (("minmax", mm), ("nonzero", nz), ("ang_mode", mode), ("mag", mag), ("ang", ang))]
        out.append((f"polar/{name}/hist", A._hist_device(e, n, mm, nz, 40, 99)))
    return out


def _same_tail(got, ref, what):
    assert [k for k, _ in got] == [k for k, _ in ref]
    for (k, a), (_, b) in zip(got, ref):
        _same(a, b, f"{what}: {k}")


def _hold_masks(e, masks):
    for label, m in masks.items():
        e.hold_mask(label, m)


# ---- 1. the file route -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cm", [1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
def test_file_route_every_held_call_equals_its_original(eng, H, W, Cm):
    flow, echo = _payload(H * W + Cm, N, H, W)
    masks = _masks(N, H, W, Cm)
    shape = eng.hold_study(flow, echo)
    _hold_masks(eng, masks)
    assert (shape.N, shape.H, shape.W, shape.n_echo) == (N, H, W, N)
    assert eng.held.masks == {"rv": (N, Cm), "av": (N, Cm)}
    for n in (N - 2, N):                                     # n = N: the gradient reads the last frame one-sided
        for grad_f64 in (False, True):
            ref = _tail(eng, n, grad_f64, False, flow, masks, echo)
            got = _tail(eng, n, grad_f64, True)
            _same_tail(got, ref, f"{H}x{W} C={Cm} n={n} grad_f64={grad_f64}")


# ---- 2. the solve route ------------------------------------------------------------------------------------------------------------
def _solve(e, form, rgb, bkgd, **kw):
    if form == "rgb":
        return e.calc_study_payload(rgb, scale=0.7, **kw)
    if form == "saliency":
        return e.calc_study_saliency_payload(rgb, scale=0.7, **kw)
    if form == "rgb_wase":
        return e.calc_study_wase_payload(rgb, bkgd, scale=0.7, **kw)
    return e.calc_study_saliency_wase_payload(rgb, bkgd, scale=0.7, **kw)


def _check_solve_route(e, form, H, W):
    rgb, bkgd, masks = _frames(N, H, W), _bkgd(H, W, H), _masks(N, H, W, 2)
    base = {pad: _solve(e, form, rgb, bkgd, pad_last=pad) for pad in (True, False)}
    flow, echo = base[True][0], base[True][1]
    assert flow.shape == (N, H, W, 2) and flow.dtype == np.float16 and np.array_equal(flow[N - 1], flow[N - 2])
    ref = _tail(e, N, True, False, flow, masks, echo)
    for pad in (True, False):
        g0 = e.held.generation if e.held else -1
        got = _solve(e, form, rgb, bkgd, pad_last=pad, hold=True)
        _same(got, base[pad], f"{form} pad_last={pad}: the call's own results with hold")
        h = e.held
        assert (h.N, h.H, h.W, h.n_echo) == (N, H, W, N) and h.generation > g0 and h.masks == {}
        _hold_masks(e, masks)
        _same_tail(_tail(e, N, True, True), ref, f"{form} {H}x{W} pad_last={pad}")
    assert e.counter("queue_units_done") > 0                  # the sub-batches went through the lanes


@pytest.mark.parametrize("form", ["rgb", "saliency", "rgb_wase", "saliency_wase"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_solve_route_holds_what_the_call_returns(eng, H, W, form):
    _check_solve_route(eng, form, H, W)


def test_solve_route_deepflow():
    e = T.createOptFlow_DeepFlow(max_batch=3)
    try:
        _check_solve_route(e, "rgb", 40, 52)
    finally:
        e.close()


def test_solve_route_without_echo(eng):
    H, W = SHAPES[1]
    rgb, masks = _frames(N, H, W), _masks(N, H, W, 1)
    flow, echo = eng.calc_study_payload(rgb, echo=False, hold=True)
    assert echo is None and eng.held.n_echo == 0
    _hold_masks(eng, masks)
    cent = np.full((N, 2), 10.0)
    _same(eng.held_radlong_project_param("rv", 2, SPACING, True, N, cent, return_arrays=True),
          eng.radlong_project_param(flow, masks["rv"], 2, SPACING, True, N, cent, return_arrays=True), "PWR without echo")


# ---- 3. residency ------------------------------------------------------------------------------------------------------------------
def test_the_upload_counter_shows_residency(eng):
    H, W = SHAPES[1]
    Cm, n = 2, N - 2
    flow, echo = _payload(3, N, H, W)
    masks = _masks(N, H, W, Cm)
    c0 = eng.counter("tail_upload_bytes")
    assert c0 >= 0
    eng.hold_study(flow, echo)
    assert eng.counter("tail_upload_bytes") - c0 == flow.nbytes + echo.nbytes
    c1 = eng.counter("tail_upload_bytes")
    _hold_masks(eng, masks)
    assert eng.counter("tail_upload_bytes") - c1 == sum(m.nbytes for m in masks.values())
    c2 = eng.counter("tail_upload_bytes")
    _tail(eng, n, True, True)
    assert eng.counter("tail_upload_bytes") == c2, "a held tail call uploaded flow, mask or echo bytes"
    _tail(eng, n, True, False, flow, masks, echo)
    frame_mask, frame_flow, frame_echo = H * W * Cm, H * W * 2 * 2, H * W * 2
    per_param = {0: n, 1: n + 1, 2: n + 1}                    # flow frames a projection of [0, n) reads (n < N)
    want = 2 * n * frame_mask                                 # centroids, first-region areas
    for p in range(3):
        want += 2 * (per_param[p] * frame_flow + n * frame_mask)   # rad/long and polar
        want += n * frame_echo                                # the overlay after each rad/long projection
    assert eng.counter("tail_upload_bytes") - c2 == want


# ---- 4. lifetime -------------------------------------------------------------------------------------------------------------------
def test_held_results_survive_other_calls_and_jobs_in_flight(eng):
    H, W = SHAPES[0]
    flow, echo = _payload(5, N, H, W)
    masks = _masks(N, H, W, 2)
    eng.hold_study(flow, echo)
    _hold_masks(eng, masks)
    n = N - 2
    ref = _tail(eng, n, True, False, flow, masks, echo)
    # other work of the handle in between: a solve without hold, both mask makers, an original projection of other data
    H2, W2 = 33, 47
    rgb2 = _frames(6, H2, W2, seed=9)
    sync = eng.calc_study_payload(rgb2)
    eng.otsu_masks(rgb2, 4)
    eng.clean_masks((rgb2[..., 0] > 128).astype(np.uint8), [1], 4)
    flow2, _ = _payload(6, 6, H2, W2)
    eng.radlong_project_param(flow2, _masks(6, H2, W2, 1)["rv"], 1, SPACING, True, 5, np.full((5, 2), 7.0))
    _same_tail(_tail(eng, n, True, True), ref, "after other calls")
    # ... and while a submitted study is in flight
    t = eng.submit_study_payload(rgb2)
    got = _tail(eng, n, True, True)
    _same(eng.wait(t), sync, "the submitted job's results")
    _same_tail(got, ref, "with a job in flight")
    # a second hold_study of another size replaces the first and empties the slots
    g = eng.held.generation
    eng.hold_study(flow2)
    h = eng.held
    assert (h.N, h.H, h.W, h.n_echo, h.masks) == (6, H2, W2, 0, {}) and h.generation > g
    with pytest.raises(OpticalFlowCalculationError, match="no mask is held under label 'rv'"):
        eng.held_first_region_areas("rv", 2)
    area = np.zeros(2, np.int64)
    assert eng._L.tf_held_first_region_areas(eng._h, 0, 2, area.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert b"slot 0 is empty" in eng._L.tf_last_error(eng._h)
    # a HeldStudy made now goes stale with the release, and the held calls are refused
    hs = A.HeldStudy(eng, 50.0)
    eng.hold_mask("rv", _masks(6, H2, W2, 1)["rv"])
    assert A.area_series(hs, "rv", engine=eng).shape == (4,)
    eng.release_study()
    assert eng.held is None
    with pytest.raises(RuntimeError, match="stale"):
        A.area_series(hs, "rv", engine=eng)
    assert eng._L.tf_held_first_region_areas(eng._h, 0, 2, area.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert b"no study is held" in eng._L.tf_last_error(eng._h)
    with pytest.raises(OpticalFlowCalculationError, match="no study is held"):
        eng.hold_mask("rv", masks["rv"])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _refused(e, rc, text, code=_lib.TF_ERR_INVALID_ARG):
    msg = e._L.tf_last_error(e._h).decode()
    assert rc == code and text in msg, (rc, msg)


def test_refusals_name_their_cause_and_leave_everything_usable(eng):
    H, W = SHAPES[1]
    L, h = eng._L, eng._h
    flow, echo = _payload(7, N, H, W)
    masks = _masks(N, H, W, 2)
    n = N - 2
    eng.hold_study(flow, echo)
    _hold_masks(eng, masks)                                   # rv -> slot 0, av -> slot 1
    eng.hold_mask("short", masks["rv"][:n - 1])               # slot 2: fewer frames than n
    cent = np.full((N, 2), 11.5)
    mm, nz = np.zeros(4), np.zeros((N, 2), np.int64)
    mm32, mode = np.zeros(4, np.float32), np.zeros(N, np.float32)
    area = np.zeros(N, np.int64)
    c2 = np.zeros((N, 2))
    ref = eng.held_radlong_project_param("rv", 1, SPACING, True, n, cent[:n], return_arrays=True)
    stats = A._radlong_stats_resident(eng, n, ref[0], ref[1], 1, 99, 40)
    gen = eng.held.generation

    def radlong(n_used, slot, param=0, spacing=SPACING):
        return L.tf_held_radlong_project_param(h, n_used, slot, param, spacing, 1, cent.ctypes.data, None, None, mm.ctypes.data, nz.ctypes.data)

    def polar(n_used, slot, param=0, spacing=SPACING):
        return L.tf_held_polar_project_param(h, n_used, slot, param, spacing, 1, None, None, mm32.ctypes.data, nz.ctypes.data, mode.ctypes.data)

    for call in (radlong, polar):
        _refused(eng, call(n, -1), "slot -1 is out of range")
        _refused(eng, call(n, 12), "slot 12 is out of range")
        _refused(eng, call(n, 5), "slot 5 is empty")
        _refused(eng, call(0, 0), f"n_used 0 is outside [1, {N}]")
        _refused(eng, call(N + 1, 0), f"n_used {N + 1} is outside [1, {N}]")
        _refused(eng, call(n, 2), f"slot 2 has {n - 1} frames, fewer than the {n} asked for")
        for bad in (0.0, float("nan"), float("inf")):
            for param in (1, 2):
                _refused(eng, call(n, 0, param, bad), "finite, non-zero spacing")
        _refused(eng, call(n, 0, 3), "param 3")
    _refused(eng, L.tf_held_av_centroids(h, 7, n, c2.ctypes.data, area.ctypes.data), "slot 7 is empty")
    _refused(eng, L.tf_held_av_centroids(h, 2, n, c2.ctypes.data, area.ctypes.data), "fewer than")
    _refused(eng, L.tf_held_av_centroids(h, 0, 0, c2.ctypes.data, area.ctypes.data), "need at least 1")
    _refused(eng, L.tf_held_first_region_areas(h, 12, n, area.ctypes.data), "out of range")
    _refused(eng, L.tf_held_first_region_areas(h, 2, n, area.ctypes.data), "fewer than")
    _refused(eng, L.tf_hold_mask(h, 12, masks["rv"].ctypes.data, N, 2), "out of range")
    _refused(eng, L.tf_hold_mask(h, 3, masks["rv"].ctypes.data, N, 3), "C=3")
    # the refused calls touched neither the resident planes nor the held study
    assert eng.held.generation == gen
    _same(A._radlong_stats_resident(eng, n, ref[0], ref[1], 1, 99, 40), stats, "the resident planes after the refusals")
    _same(eng.held_radlong_project_param("rv", 1, SPACING, True, n, cent[:n], return_arrays=True), ref, "the held study after the refusals")
    # the overlay's echo
    out, info = np.zeros((n, H, 2 * W, 3), np.uint8), np.zeros(3)
    ov = lambda: L.tf_held_radlong_overlay(h, LUT_RAD.ctypes.data, LUT_LONG.ctypes.data, out.ctypes.data, info.ctypes.data)  # noqa: E731
    eng.hold_study(flow, echo[:2])
    eng.hold_mask("rv", masks["rv"])
    eng.held_radlong_project_param("rv", 0, SPACING, True, n, cent[:n])
    _refused(eng, ov(), f"the held echo has 2 frames, fewer than the planes' {n}")
    eng.hold_study(flow)
    _refused(eng, ov(), "the held study has no echo")
    eng.hold_study(flow, echo)
    eng.hold_mask("rv", masks["rv"])
    assert ov() == 0                                          # the planes of the projection before are still there
    _same((out, info), eng.radlong_overlay(echo, LUT_RAD, LUT_LONG), "the overlay after its refusals")
    # a study of one frame has no gradient
    eng.hold_study(flow[:1], echo[:1])
    eng.hold_mask("rv", masks["rv"][:1])
    for call in (radlong, polar):
        for param in (1, 2):
            _refused(eng, call(1, 0, param), "at least 2 held frames")
        assert call(1, 0, 0) == 0
    eng.release_study()
    for rc in (radlong(n, 0), polar(n, 0), ov(), L.tf_held_av_centroids(h, 0, n, c2.ctypes.data, area.ctypes.data),
               L.tf_held_first_region_areas(h, 0, n, area.ctypes.data), L.tf_hold_mask(h, 0, masks["rv"].ctypes.data, N, 2)):
        _refused(eng, rc, "no study is held")


def test_an_armed_flag_is_spent_by_the_next_study_call(eng):
    H, W = SHAPES[0]
    rgb = _frames(N, H, W)
    flow, echo = _payload(8, N, H, W)
    eng.hold_study(flow, echo)
    gen = eng.held.generation
    for refused in (lambda: eng.submit_study_payload(rgb), lambda: eng.submit_study(rgb), lambda: eng.calc_study(rgb),
                    lambda: eng.calc_study_wase(rgb, _bkgd(H, W, 1))):
        eng.hold_next()
        with pytest.raises(OpticalFlowCalculationError, match="held") as ei:
            refused()
        assert ei.value.code == _lib.TF_ERR_UNSUPPORTED
        assert eng.counter("queue_outstanding") == 0
        eng.calc_study_payload(rgb)                           # the flag is spent: this call holds nothing
        assert eng.held.generation == gen
    eng.hold_next()                                           # a call refused for its arguments spends the flag too
    out16 = np.zeros((N, H, W, 2), np.float16)
    rc = eng._L.tf_calc_seq_rgb_f16(eng._h, rgb.ctypes.data, 1, H, W, 1.0, out16.ctypes.data, None, None)
    _refused(eng, rc, "at least 2 frames")
    eng.calc_study_payload(rgb)
    assert eng.held.generation == gen
    eng.hold_next()
    eng.hold_next(False)
    eng.calc_study_payload(rgb)
    assert eng.held.generation == gen
    assert eng.held.N == N and eng.held.n_echo == N
    with pytest.raises(OpticalFlowCalculationError, match="float16 study call that is waited for"):
        eng._study(rgb, 1.0, True, hold=True)


# ---- 6. the analysis functions with a HeldStudy ------------------------------------------------------------------------------------
def _flow_study(H, W, n=14):
    flow, echo = _payload(H + W, n, H, W)
    masks = _masks(n, H, W, 2)
    return A.FlowStudy(flow, masks, np.float64(50.0), echo=echo, filename="held")


def _analysis(ds, e):
    out = []
    cent = A.av_centroids(ds.get_mask("av"), ds.nframes, engine=e)
    out.append(("av_centroids", np.asarray(cent)))
    for param in A.PARAMS:
        st = A.calculate_3dhist_radlong(ds, param, nbins=60, engine=e)
        assert sorted(st) == ["longitudinal", "radial"]
        out += [(f"radlong/{param}/{k}", st[k]) for k in sorted(st)]
        out.append((f"radlong_shared_centroids/{param}", A.calculate_3dhist_radlong(ds, param, nbins=60, engine=e, centroids=cent)["radial"]))
        out.append((f"3dhist/{param}", A.calculate_3dhist(ds, param, "rv", nbins=60, engine=e)))
        out.append((f"overlay/{param}", A.radlong_overlay(ds, param, engine=e, return_info=True)))
    out.append(("angle_mode", A.angle_mode_series(ds, "velocity", "rv", engine=e)))
    out.append(("area/rv", A.area_series(ds, "rv", engine=e)))
    out.append(("area/av", A.area_series(ds, "av", engine=e)))
    rec = Recorder()
    path = A.visualize_radlong(ds, "PWR", "unused_dir_of_the_recorder", engine=e, writer_factory=rec)
    out += [("video/frames", np.stack(rec.frames)), ("video/path", np.frombuffer(path.encode(), np.uint8))]
    assert A.calculate_3dhist(ds, "velocity", "nolabel", engine=e) is None and A.calculate_3dhist_radlong(ds, "speed", engine=e) is None
    return out


@pytest.mark.parametrize("H,W", SHAPES)
def test_analysis_functions_with_a_held_study(eng, H, W, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                               # (visualize_radlong makes its save_dir)
    st = _flow_study(H, W)
    ref = _analysis(st, eng)
    hs = A.HeldStudy.from_study(eng, st)
    assert hs.nframes == st.nframes == 12 and hs.accepted_labels == ["rv", "av"]
    c = eng.counter("tail_upload_bytes")
    _same_tail(_analysis(hs, eng), ref, f"HeldStudy {H}x{W}")
    assert eng.counter("tail_upload_bytes") == c
    other = T.DenseFlow(device_id=0)
    try:
        for e in (None, other):
            with pytest.raises(ValueError, match="engine"):
                A.calculate_3dhist_radlong(hs, "velocity", engine=e)
            with pytest.raises(ValueError, match="engine"):
                A.area_series(hs, "rv", engine=e)
    finally:
        other.close()
    eng.hold_study(st.flow)                                   # replaced: the HeldStudy is stale
    for call in (lambda: A.calculate_3dhist(hs, "velocity", "rv", engine=eng), lambda: A.av_centroids(hs, 3, engine=eng),
                 lambda: A.radlong_overlay(hs, "velocity", engine=eng)):
        with pytest.raises(RuntimeError, match="stale"):
            call()


def test_held_study_from_hdf5(eng, tmp_path):
    h5py = pytest.importorskip("h5py")
    H, W = SHAPES[1]
    st = _flow_study(H, W)
    path = str(tmp_path / "study.hdf5")
    with h5py.File(path, "w") as f:
        d = f.create_dataset("flow", data=st.flow)
        d.attrs["frame_rate"], d.attrs["units_converted"], d.attrs["nframes"] = 50.0, True, st.flow.shape[0]
        d.attrs["mode"], d.attrs["labels"] = "RVIO_2class", ["rv", "av"]
        f.create_dataset("echo", data=st.echo)
        for k, m in st.masks.items():
            f.create_dataset(k, data=m)
    fs = A.FlowStudy.from_hdf5(path)
    hs = A.HeldStudy.from_hdf5(eng, path)
    assert hs.filename == fs.filename and hs.nframes == fs.nframes
    for param in A.PARAMS:
        a, b = A.calculate_3dhist_radlong(hs, param, engine=eng), A.calculate_3dhist_radlong(fs, param, engine=eng)
        for k in ("radial", "longitudinal"):
            _same(a[k], b[k], f"{param}/{k}")
