"""clean_mask on the device (tf_clean_masks, DenseFlow.clean_masks): byte-equal to the reference's own clean_mask
(tests/golden/reference_clean_mask.npz) and to the host path at study sizes, beside submitted solves on the same engine,
through process_video's segmentor branch, and in turns with the other calls that label in the same device scratch."""
import numpy as np
import pytest

from tee_optical_flow_amd import analysis, masks
from tests.labelling_cases import corner_diagonals, load_fuzzer, stress_frames
from tests.test_masks_cpu import _Cfg, fixture_cases
from tests.test_otsu_cpu import fixture_cases as otsu_fixture_cases

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == np.bool_ and a[k].shape == b[k].shape and a[k].flags.c_contiguous, k
        assert np.array_equal(a[k], b[k]), k


def _class_map(seed, N, H, W, n_cls):
    """blobs with holes that drift over time, salt noise, a border-touching band"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((N, H, W), np.uint8)
    shapes = [(int(rng.integers(1, n_cls + 1)), rng.uniform(0, H), rng.uniform(0, W), rng.uniform(5, H / 4), rng.uniform(5, W / 4),
               rng.uniform(-2, 2, 2)) for _ in range(3 * n_cls)]
    for f in range(N):
        m = out[f]
        for c, cy, cx, ry, rx, v in shapes:
            d = ((yy - cy - v[0] * f) / ry) ** 2 + ((xx - cx - v[1] * f) / rx) ** 2
            m[d < 1.0] = c
            m[d < 0.08] = 0
        m[: H // 10, : W // 3] = 1
        salt = rng.random((H, W)) < 0.002
        m[salt] = rng.integers(0, n_cls + 1, int(salt.sum()))
    return out


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_device_equals_reference_fixture(engine, case):
    name, arr, mode, min_size, keys, ref = case
    got = masks.clean_mask(arr, mode, config=_Cfg(min_size), engine=engine)
    assert list(got) == keys
    for k in keys:
        assert got[k].dtype == np.bool_ and got[k].flags.c_contiguous
        assert np.array_equal(got[k][..., 0], ref[k]) and np.array_equal(got[k][..., 1], ref[k]), k
    planes = engine.clean_masks(arr, list(masks._MODE_LABELS[mode].values()), min_size)
    assert planes.shape == (len(keys),) + arr.shape + (2,)
    assert np.array_equal(planes.view(np.uint8)[..., 0], np.stack([ref[k] for k in keys]).astype(np.uint8))   # bytes 0 / 1


def test_calls_that_share_the_labelling_scratch_do_not_see_each_other(engine):
    """tf_av_centroids, tf_clean_masks and tf_otsu_masks label in the same parents, sizes / areas and tile-local roots of the handle.
    Large, small, large on one engine: a smaller call finds another call's stale words beyond and inside its own extent."""
    frames = stress_frames()
    mask_cases = {c[0]: c for c in fixture_cases()}

    def centroids(fr, flipped=False):
        m = np.repeat(fr[None, :, :, None], 2, axis=3)
        m = np.concatenate([m, m[:, ::-1, ::-1]], axis=0) if flipped else m
        cent, area = engine.av_centroids(m)
        for f in range(m.shape[0]):
            want = analysis._largest_component(m[f, :, :, 0])
            assert (area[f] == 0) if want is None else (area[f] == want[1] and tuple(cent[f]) == want[0]), f

    def clean(name):
        _, arr, mode, min_size, keys, ref = mask_cases[name]
        got = masks.clean_mask(arr, mode, config=_Cfg(min_size), engine=engine)
        assert list(got) == keys
        for k in keys:
            assert np.array_equal(got[k][..., 0], ref[k]) and np.array_equal(got[k][..., 1], ref[k]), (name, k)

    centroids(frames["snake"], flipped=True)                                  # 2 x 61 x 200
    clean("hard_checker1_min5")                                               # 3 x 150 x 170, two labels
    centroids(frames["single_pixel"])                                         # 37 x 70
    centroids(frames["empty"])                                                # 20 x 20
    _, rgb, min_size, ref, thr = min(otsu_fixture_cases(), key=lambda c: c[1].size)
    got, got_thr = engine.otsu_masks(rgb, min_size, return_thresholds=True)
    assert np.array_equal(got_thr, thr) and np.array_equal(got[..., 0], ref) and np.array_equal(got[..., 1], ref)
    clean("rvio_9x37x53_min5")
    centroids(frames["staircase"])                                            # 70 x 200


def test_stress_frames_through_the_four_connected_calls(engine):
    """The frames made to break a tiled labeller, through the 4-connected instantiation: each frame and its 180-degree flip as a
    2-frame class map through clean_masks (min_size 1 and 2) and, where it has both levels and H, W >= 2, as a built RGB study through
    otsu_masks, against the scipy references of tools/fuzz_labelling.py.  The staircases and the tile-corner pixels touch only
    diagonally: 4-connected they fall apart (min_size 2 drops every staircase pixel), 8-connected (av_centroids) they hold together.
    tile_corners has 2 x 2 blocks on its corners, which either rule joins, so corner_diagonals() walks with the stress frames."""
    F = load_fuzzer()
    rng = np.random.default_rng(11)
    built = []
    for name, fr in {**stress_frames(), "corner_diagonals": corner_diagonals()}.items():
        pair = np.stack([fr, fr[::-1, ::-1]])
        cmap = pair.astype(np.uint8)
        for min_size in (1, 2):
            got = engine.clean_masks(cmap, [1], min_size)
            F._same_planes(got, F.ref_clean(cmap, [1], min_size), (name, min_size))
        if name in ("tile_corners", "staircase", "corner_diagonals"):
            n4, n8 = F.ref_sizes(fr)[1].size - 1, len(F.ref_components(fr))
            assert n4 > 1 and n4 >= n8 >= 1, (name, n4, n8)
            cent, area = engine.av_centroids(pair[:, :, :, None])
            for f in range(2):
                (r, c), a = F.ref_centroid(pair[f])
                assert int(area[f]) == a and tuple(cent[f]) == (r, c), (name, f)
                if name != "tile_corners":                                    # larger than any 4-connected component
                    assert n4 > n8 and a > F.ref_sizes(pair[f])[1][1:].max(), (name, n4, n8, a)
        if name in ("staircase", "corner_diagonals"):
            assert F.ref_clean(cmap, [1], 1)[0, 1].sum() == fr.sum() and not F.ref_clean(cmap, [1], 2)[0, 1].any()
        if min(fr.shape) < 2:
            continue
        frames = [F.build_rgb(rng, m) for m in pair]
        if any(f is None for f in frames):
            continue
        built.append(name)
        rgb = np.stack(frames)
        for min_size in (1, 2):
            got, thr = engine.otsu_masks(rgb, min_size, return_thresholds=True)
            assert all(F.between_levels(rgb[f], pair[f], thr[f]) for f in range(2)), (name, thr)
            F._same_planes(got.copy(), F.ref_otsu(pair, min_size), (name, "otsu", min_size))
    assert built == ["single_pixel", "checkerboard", "snake", "staircase", "tile_corners", "random_17x65", "random_129x63", "random_100x257",
                     "corner_diagonals"]


@pytest.mark.parametrize("N,H,W,mode,min_size", [
    (65, 512, 512, "RVIO_2class", 500),
    (33, 256, 256, "A4C", 500),
    (45, 512, 512, "A4C", 500),                     # three chunks of frames (the 512 MiB scratch bound)
    (3, 600, 800, "RVIO_2class", 500),
    (2, 1080, 1920, "RVIO_2class", 500),
    (2, 97, 131, "RVIO_2class", 500),
    (3, 97, 131, "A4C", 30),
    (9, 97, 131, "RVIO_2class", 0),
    (9, 97, 131, "RVIO_2class", 1),
    (9, 97, 131, "RVIO_2class", 97 * 131 + 1),
    (9, 97, 131, "MouseRV_A4C", -3),
])
def test_device_equals_host(engine, N, H, W, mode, min_size):
    arr = _class_map(N * 1000 + H, N, H, W, len(masks._MODE_LABELS[mode]))
    cfg = _Cfg(min_size)
    _same(masks.clean_mask(arr, mode, config=cfg, engine=engine), masks.clean_mask(arr, mode, config=cfg))


@pytest.mark.parametrize("shape", [(1, 40, 50), (5, 1, 50), (5, 40, 1), (1, 1, 9)])
def test_degenerate_shapes_behave_like_the_host_path(engine, shape):
    arr = _class_map(7, *shape, 2) if min(shape[1:]) > 1 else np.random.default_rng(7).integers(0, 3, shape).astype(np.uint8)
    try:
        want = masks.clean_mask(arr, "RVIO_2class")
    except Exception as e:
        with pytest.raises(type(e)):
            masks.clean_mask(arr, "RVIO_2class", engine=engine)
        return
    _same(masks.clean_mask(arr, "RVIO_2class", engine=engine), want)


@pytest.mark.parametrize("algo", ["TVL1", "deepflow"])
def test_masks_beside_a_submitted_study(algo):
    """a study submitted and still in flight on the engine's lanes, masks cleaned on the same engine before the wait: both results
    equal their serial runs (what process_folder(studies_in_flight=2) does)"""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(31, 24, 256, 256)
    rgb = np.ascontiguousarray(np.repeat(g[..., None], 3, axis=3))
    arr = _class_map(5, 65, 512, 512, 2)
    host = masks.clean_mask(arr, "RVIO_2class")
    eng = T.DenseFlow(device_id=0, algo=algo)
    try:
        serial = eng.calc_study(rgb).copy()
        aborts0 = eng.counter("coop_aborts")
        t = eng.submit_study(rgb)
        got = masks.clean_mask(arr, "RVIO_2class", engine=eng)
        flows = eng.wait(t)
        aborts = eng.counter("coop_aborts") - aborts0
    finally:
        eng.close()
    print(f"{algo}: coop_aborts during the overlapped call: {aborts}")
    _same(got, host)
    assert np.array_equal(flows, serial)


def test_process_video_segmentor_branch_cleans_on_the_flow_model(engine, monkeypatch):
    """process_video(mode='RVIO_2class', segmentor_model=stand-in) cleans its masks on the flow model (given or its own) and returns
    the flows and hands the writer the mask datasets of a run given mask_dict= from the host path"""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.pipeline import process_video
    from tee_optical_flow_amd.synth import speckle_sequence
    from tests.test_study_driver_cpu import _FakeSam
    g = speckle_sequence(12, 8, 96, 128)
    nparr = np.repeat(g[..., None], 3, axis=3)
    sam = _FakeSam()
    md = {"pixel_spacing": 0.04, "frame_rate": 50.0, "R_wave_data_present": False, "R_times": None}
    calls = []
    real = T.DenseFlow.clean_masks

    def counted(self, *a, **k):
        calls.append(a[0].shape)
        return real(self, *a, **k)
    monkeypatch.setattr(T.DenseFlow, "clean_masks", counted)
    host_masks = masks.predict_movie(nparr, sam, mode="RVIO_2class")
    assert calls == []
    jobs = {}
    kw = dict(verbose=False, mode="RVIO_2class", bkgd_comp="WASE", no_saliency=True, nparr=nparr, metadata=md)
    ref = process_video(None, "ref.hdf5", sam, flow_model=engine, mask_dict=host_masks, _defer_save=lambda j: jobs.setdefault("ref", j), **kw)
    assert calls == []
    dev = process_video(None, "dev.hdf5", sam, flow_model=engine, _defer_save=lambda j: jobs.setdefault("dev", j), **kw)
    assert calls == [(8, 96, 128)]
    own = process_video(None, "own.hdf5", sam, _defer_save=lambda j: jobs.setdefault("own", j), **kw)      # the call makes its own model
    assert len(calls) == 2
    assert np.array_equal(dev, ref) and np.array_equal(own, ref)
    for name in ("dev", "own"):
        _same(jobs[name].mask_dict, jobs["ref"].mask_dict)
        assert np.array_equal(jobs[name].flow, jobs["ref"].flow)
