"""The Otsu mode's host path against the reference's own predict_movie_thres (tests/golden/reference_otsu.npz, made by
make_reference_otsu_fixtures.py), the choice between host and device path, and tf_otsu_masks' argument checks, which return before
any GPU work."""
import ctypes as C
import os

import numpy as np
import pytest

from tee_optical_flow_amd import masks
from tee_optical_flow_amd.frames import rgb2gray

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_otsu.npz")


def fixture_cases():
    """(name, frames uint8 [N,H,W,3], min_size, mask channel 0 bool [N,H,W], thresholds float64 [N])"""
    z = np.load(FIX)
    names = sorted({k.split("/")[0] for k in z.files})
    out = []
    for n in names:
        src = n if f"{n}/in" in z.files else str(z[f"{n}/in_of"])
        out.append((n, z[f"{src}/in"], int(z[f"{n}/min_size"]), z[f"{n}/otsu"].astype(bool), z[f"{n}/thr"]))
    return out


class _Cfg:
    def __init__(self, min_size):
        self.min_mask_size = min_size


def test_fixture_covers_the_issue_cases():
    cases = fixture_cases()
    names = [c[0] for c in cases]
    for part in ("grey", "rgb_noise", "sector", "odd", "constant_frame", "two_valued", "n2_", "n3_"):
        assert any(part in n for n in names), part
    sizes = {c[2] for c in cases if c[0].startswith("minsize")}
    n, h, w = next(c[1].shape[:3] for c in cases if c[0].startswith("minsize"))
    assert {0, 1, 500} <= sizes and any(s > h * w for s in sizes)
    assert {c[1].shape[0] for c in cases} >= {2, 3}
    assert any(c[1].shape[1] % 16 and c[1].shape[2] % 64 for c in cases)                  # not multiples of the device's tile
    assert any((c[1][..., 0] != c[1][..., 1]).any() for c in cases)                       # true RGB
    const = next(c for c in cases if c[0].startswith("constant_frame"))
    assert any(np.ptp(f) == 0 for f in const[1])
    assert os.path.getsize(FIX) < 411854                                                  # the largest fixture committed before it


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_host_predict_movie_thres_equals_reference(case):
    name, frames, min_size, ref, thr = case
    got = masks.predict_movie_thres(frames, config=_Cfg(min_size))
    assert list(got) == ["otsu"]
    v = got["otsu"]
    assert v.dtype == np.bool_ and v.shape == frames.shape[:3] + (2,)
    assert np.array_equal(v[..., 0], ref) and np.array_equal(v[..., 1], ref)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_host_threshold_otsu_equals_reference(case):
    name, frames, min_size, ref, thr = case
    got = np.array([masks.threshold_otsu(rgb2gray(f)) for f in frames], dtype=np.float64)
    assert np.array_equal(got, thr)


def test_threshold_otsu_of_a_one_valued_image_is_that_value():
    assert masks.threshold_otsu(np.full((5, 7), 0.25)) == 0.25
    assert masks.threshold_otsu(np.zeros((3, 3))) == 0.0


def test_engine_without_otsu_masks_stays_on_the_host():
    """a flow model that lacks otsu_masks (the CPU tests' fakes) is not asked for it"""
    class NoMasks:
        pass
    frames = fixture_cases()[0][1]
    a = masks.predict_movie_thres(frames, config=_Cfg(50), engine=NoMasks())
    b = masks.predict_movie_thres(frames, config=_Cfg(50))
    assert list(a) == list(b) == ["otsu"] and np.array_equal(a["otsu"], b["otsu"])


def test_only_uint8_rgb_stacks_of_at_least_two_in_every_axis_go_to_the_engine():
    calls = []

    class Spy:
        def otsu_masks(self, nparr, min_size):
            calls.append((nparr.shape, min_size))
            return np.zeros(nparr.shape[:3] + (2,), bool)

    rng = np.random.default_rng(3)
    for shape in ((1, 9, 9, 3), (4, 1, 9, 3), (4, 9, 1, 3)):               # np.squeeze changes what the reference computes: host path
        arr = rng.integers(0, 255, shape).astype(np.uint8)
        try:
            want = masks.predict_movie_thres(arr, config=_Cfg(2))
        except Exception as e:                                              # (the host path raises for some of them; so must the call)
            with pytest.raises(type(e)):
                masks.predict_movie_thres(arr, config=_Cfg(2), engine=Spy())
        else:
            got = masks.predict_movie_thres(arr, config=_Cfg(2), engine=Spy())
            assert np.array_equal(got["otsu"], want["otsu"])
    masks.predict_movie_thres(rng.random((4, 9, 9, 3)), config=_Cfg(2), engine=Spy())                          # not uint8
    masks.predict_movie_thres(rng.integers(0, 255, (4, 9, 9, 4)).astype(np.uint8), config=_Cfg(2), engine=Spy())   # RGBA
    assert calls == []
    got = masks.predict_movie_thres(np.zeros((2, 3, 4, 3), np.uint8), config=_Cfg(7), engine=Spy())
    assert calls == [((2, 3, 4, 3), 7)] and list(got) == ["otsu"] and got["otsu"].shape == (2, 3, 4, 2)


def test_tf_otsu_masks_rejects_bad_arguments_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    rgb = np.zeros((2, 4, 4, 3), np.uint8)
    out = np.zeros((2, 4, 4, 2), np.uint8)
    thr = np.full(2, -1.0)
    fake = C.create_string_buffer(64)            # never dereferenced: every check comes before the handle is used
    h = C.addressof(fake)
    good = dict(h=h, rgb=rgb.ctypes.data, N=2, H=4, W=4, min_size=500, out=out.ctypes.data, thr=thr.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_otsu_masks(a["h"], a["rgb"], a["N"], a["H"], a["W"], a["min_size"], a["out"], a["thr"])

    assert call(h=None) == 1
    for bad in (dict(rgb=None), dict(out=None), dict(N=1), dict(N=0), dict(H=1), dict(W=1), dict(W=-1), dict(N=-5),
                dict(rgb=None, thr=None)):
        assert call(**bad) == 1, bad
    assert call(H=65536, W=65536) == 2           # more than 2^31 - 1 pixels per frame
    assert call(H=46341, W=46341, thr=None) == 2
    assert call(N=65536) == 2                    # frames are a grid dimension
    assert not out.any() and (thr == -1.0).all()


def test_process_folder_rejects_an_unknown_otsu_masks_value(tmp_path):
    from tee_optical_flow_amd.exceptions import ConfigurationError
    from tee_optical_flow_amd.pipeline import process_folder
    with pytest.raises(ConfigurationError):
        process_folder(str(tmp_path), str(tmp_path / "out"), mode="otsu", otsu_masks="bogus")
    assert not (tmp_path / "out").exists()
