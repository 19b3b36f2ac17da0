"""clean_mask's host path against the reference's own clean_mask (tests/golden/reference_clean_mask.npz, made by
make_reference_clean_mask_fixtures.py), and tf_clean_masks' argument checks, which return before any GPU work."""
import ctypes as C
import os

import numpy as np
import pytest

from tee_optical_flow_amd import masks

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_clean_mask.npz")


def fixture_cases():
    z = np.load(FIX)
    names = sorted({k.split("/")[0] for k in z.files})
    out = []
    for n in names:
        keys = [str(k) for k in z[f"{n}/keys"]]
        out.append((n, z[f"{n}/in"], str(z[f"{n}/mode"]), int(z[f"{n}/min_size"]), keys, {k: z[f"{n}/{k}"].astype(bool) for k in keys}))
    return out


class _Cfg:
    def __init__(self, min_size):
        self.min_mask_size = min_size


def test_fixture_covers_the_issue_cases():
    names = [c[0] for c in fixture_cases()]
    assert len(names) >= 20
    for part in ("spiral", "serpentine", "diagonal", "corner", "exact", "checker", "empty_full", "borders", "a4c_5x129x257", "rvio_9x37x53"):
        assert any(part in n for n in names), part
    modes = {c[2] for c in fixture_cases()}
    assert {"A4C", "RVIO_2class", "MouseRV_A4C"} <= modes


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_host_clean_mask_equals_reference(case):
    name, arr, mode, min_size, keys, ref = case
    got = masks.clean_mask(arr, mode, config=_Cfg(min_size))
    assert list(got) == keys
    for k in keys:
        v = got[k]
        assert v.dtype == np.bool_ and v.shape == arr.shape + (2,) and v.flags.c_contiguous
        assert np.array_equal(v[..., 0], ref[k]) and np.array_equal(v[..., 1], ref[k]), k


def test_engine_without_clean_masks_stays_on_the_host():
    """a flow model that lacks clean_masks (the CPU tests' fakes) is not asked for it"""
    class NoMasks:
        pass
    arr = fixture_cases()[0][1]
    a = masks.clean_mask(arr, "RVIO_2class", config=_Cfg(50), engine=NoMasks())
    b = masks.clean_mask(arr, "RVIO_2class", config=_Cfg(50))
    assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_only_uint8_maps_of_at_least_two_in_every_axis_go_to_the_engine():
    calls = []

    class Spy:
        def clean_masks(self, class_map, class_ids, min_size):
            calls.append((class_map.shape, list(class_ids), min_size))
            n, h, w = class_map.shape
            return np.zeros((len(class_ids) + 1, n, h, w, 2), bool)

    rng = np.random.default_rng(3)
    for shape in ((1, 9, 9), (4, 1, 9), (4, 9, 1)):                      # np.squeeze changes what the reference computes: host path
        arr = rng.integers(0, 3, shape).astype(np.uint8)
        try:
            want = masks.clean_mask(arr, "RVIO_2class")
        except Exception as e:                                             # (the host path raises for some of them; so must the call)
            with pytest.raises(type(e)):
                masks.clean_mask(arr, "RVIO_2class", engine=Spy())
        else:
            got = masks.clean_mask(arr, "RVIO_2class", engine=Spy())
            assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want)
    masks.clean_mask(rng.integers(0, 3, (4, 9, 9)).astype(np.int64), "RVIO_2class", engine=Spy())   # not uint8
    assert calls == []
    assert masks.clean_mask(np.zeros((2, 2, 2), np.uint8), "nonsense", engine=Spy()) is None
    got = masks.clean_mask(np.zeros((2, 3, 4), np.uint8), "A4C", config=_Cfg(7), engine=Spy())
    assert calls == [((2, 3, 4), [1, 2, 3, 4, 5, 6, 7, 8], 7)]
    assert list(got) == ["lv_inner", "lv", "la_inner", "la", "rv_inner", "ra_inner", "rv", "ra", "bkgd"]


def test_tf_clean_masks_rejects_bad_arguments_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    cmap = np.zeros((2, 4, 4), np.uint8)
    ids = np.array([1, 2], np.uint8)
    out = np.zeros((3, 2, 4, 4, 2), np.uint8)
    fake = C.create_string_buffer(64)            # never dereferenced: every check comes before the handle is used
    h = C.addressof(fake)
    good = dict(h=h, cmap=cmap.ctypes.data, N=2, H=4, W=4, ids=ids.ctypes.data, n=2, min_size=500, out=out.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_clean_masks(a["h"], a["cmap"], a["N"], a["H"], a["W"], a["ids"], a["n"], a["min_size"], a["out"])

    assert call(h=None) == 1
    for bad in (dict(cmap=None), dict(ids=None), dict(out=None), dict(N=0), dict(H=0), dict(W=-1), dict(n=0), dict(N=-5)):
        assert call(**bad) == 1, bad
    assert not out.any()
