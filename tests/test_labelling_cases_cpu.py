"""The labelling fuzzer (tools/fuzz_labelling.py) before a GPU sees it: its scipy references equal the host twins (masks.clean_mask's host
path, masks.predict_movie_thres, analysis._largest_component, scipy's binary_fill_holes) on the first 150 draws of seeds 1 and 2, and
the 300 draws of each seed cover what they are meant to: filled holes, a min_size that both drops and keeps a component, frames of more
than one 64 x 16 tile, tied largest areas, repeated and absent ids."""
import functools
import hashlib

import numpy as np
import pytest
from scipy.ndimage import binary_fill_holes

from tee_optical_flow_amd import analysis, masks
from tests import labelling_cases as LC

SEEDS = (1, 2)


F = LC.load_fuzzer()


@functools.lru_cache(maxsize=None)
def draws(seed):
    return [F.draw(seed, c) for c in range(300)]


def test_the_windows_float_rule_is_the_integer_rule():
    assert all((k / 4 > 0.49) == (k >= 2) for k in range(5))
    rng = np.random.default_rng(0)
    for N in (1, 2, 3, 4, 7):
        planes = rng.random((N, 5, 6)) < 0.5
        assert np.array_equal(F.ref_window(planes), masks.moving_avg_mask(planes))


def test_stress_frames_are_the_frames_they_were():
    fr = LC.stress_frames()
    assert list(fr) == ["full", "single_pixel", "checkerboard", "snake", "staircase", "tile_corners", "random_1x300", "random_300x1",
                        "random_1x1", "random_17x65", "random_129x63", "random_100x257", "empty"]
    assert [int(v.sum()) for v in fr.values()] == [5200, 1, 3500, 3014, 140, 13, 123, 148, 1, 503, 3671, 11508, 0]
    h = hashlib.sha256()
    for k, v in fr.items():
        h.update(k.encode() + str(v.shape).encode() + np.packbits(v).tobytes())
    assert h.hexdigest() == "8f7b02ebdd2e681a5f25443a0bdb8b41680235e08b3544a50f2005b1af301274"     # taken before adversarial() was added


@pytest.mark.parametrize("family", LC.FAMILIES)
def test_families_draw_every_size(family):
    for s, (H, W) in enumerate([(1, 1), (1, 2), (2, 2), (1, 9), (9, 1), (2, 3), (3, 3), (16, 64), (17, 65), (33, 129), (80, 200)]):
        if family == "twins" and max(H, W) < 3:
            with pytest.raises(ValueError):
                LC.adversarial(np.random.default_rng([s, 1]), H, W, family)
            continue
        m = LC.adversarial(np.random.default_rng([s, 1]), H, W, family)
        assert m.dtype == np.bool_ and m.shape == (H, W)
        assert np.array_equal(m, LC.adversarial(np.random.default_rng([s, 1]), H, W, family))      # the rng alone decides
        if family == "maze":
            assert F.ref_sizes(m)[1].size <= 2                                                     # one 4-connected component
        if family == "twins":
            assert F.tied_at_the_maximum(m)


def test_down_left_twins_put_the_later_copy_at_the_smaller_column():
    for s in range(10):
        m = LC.twins(np.random.default_rng(s), 30, 90, down_left=True)
        t = F.ref_components(m)
        a, b = sorted((r for r in t.tolist() if r[0] == t[:, 0].max()), key=lambda r: r[1])[:2]
        assert a[0] == b[0] and a[1] < b[1] and b[3] / b[0] < a[3] / a[0] and b[2] / b[0] > a[2] / a[0]


@pytest.mark.parametrize("seed", SEEDS)
def test_references_equal_the_host_twins(seed, monkeypatch):
    whole = {"clean": 0, "otsu": 0, "centroids": 0}
    for case in draws(seed)[:150]:
        N, H, W = case.shape
        if case.call == "clean":
            for cls in set(case.ids):
                m = F.ref_window(case.cmap == cls)
                assert np.array_equal(m, masks.moving_avg_mask(case.cmap == cls)), case
                for f in range(N):
                    filled = F.ref_fill(m[f])[0]
                    assert np.array_equal(filled, binary_fill_holes(m[f])), (case, cls, f)
                    assert np.array_equal(F.ref_small(filled, case.min_size)[0], masks.remove_small_objects(filled, case.min_size)), (case, cls, f)
            if min(N, H, W) >= 2:                                         # (below that the reference's np.squeeze changes what clean_mask computes)
                keys = [f"p{i}" for i in range(len(case.ids))]
                monkeypatch.setitem(masks._MODE_LABELS, "fuzz", dict(zip(keys, case.ids)))
                host = masks.clean_mask(case.cmap, "fuzz", config=F._Cfg(case.min_size))
                assert list(host) == keys + ["bkgd"]
                for k, want in zip(host, case.want):
                    assert np.array_equal(host[k][..., 0], want) and np.array_equal(host[k][..., 1], want), (case, k)
                whole["clean"] += 1
        elif case.call == "otsu":
            host = masks.predict_movie_thres(case.rgb, config=F._Cfg(case.min_size))["otsu"]
            assert host.shape == case.want.shape + (2,)
            assert np.array_equal(host[..., 0], case.want) and np.array_equal(host[..., 1], case.want), case
            if case.cover["built"]:
                for f in range(N):
                    assert np.array_equal(F.ref_fill(case.fmasks[f])[0], binary_fill_holes(case.fmasks[f])), (case, f)
            whole["otsu"] += 1
        else:
            for f in range(N):
                host = analysis._largest_component(case.mask[f, :, :, 0])
                (r, c), a = case.want[f]
                assert (a == 0) if host is None else (host[1] == a and host[0] == (r, c)), (case, f)
            whole["centroids"] += 1
    assert min(whole.values()) >= 25, whole


@pytest.mark.parametrize("seed", SEEDS)
def test_the_draw_covers_what_it_is_meant_to(seed):
    cases = draws(seed)
    masks_cases = [c for c in cases if c.call in ("clean", "otsu")]
    otsu = [c for c in cases if c.call == "otsu"]
    count = {
        "hole_filled": sum(c.cover["hole_filled"] for c in masks_cases),
        "drops_and_keeps": sum(c.cover["drops_and_keeps"] for c in masks_cases),
        "more_than_a_tile": sum(c.shape[1] > 16 or c.shape[2] > 64 for c in cases),
        "odd_ids": sum(c.cover["odd_ids"] for c in cases),
        "twins": sum(len(c.cover["twins_tied"]) for c in cases),
        "redraws": sum(c.cover["redraws"] for c in otsu),
        "otsu": len(otsu),
    }
    print(seed, count)
    assert count["hole_filled"] >= 100
    assert count["drops_and_keeps"] >= 75
    assert count["more_than_a_tile"] >= 240
    assert count["twins"] > 0 and all(all(c.cover["twins_tied"]) for c in cases)
    assert count["odd_ids"] >= 10
    assert count["redraws"] < 0.05 * count["otsu"]
    assert {c.call for c in cases} == set(F.CALLS)
    exact = [c.cover["min_kind"] for c in cases if c.call == "clean" and c.cover["min_kind"] != "edge"]
    assert 2 * len(exact) >= sum(c.call == "clean" for c in cases)       # a component's exact size or one above it: at least half
    assert {"size", "size+1"} <= set(exact)
    sizes = {(c.shape[1] in (1, 2) or c.shape[2] in (1, 2)) for c in cases}
    assert sizes == {True, False}
