"""The statistics tail on the device against plain numpy, on the cases of tests/stats_cases.py: ties, values on the bin edges, bin
counts from 1 to 10000, percentiles at both ends, keys that differ in one digit only, empty frames, degenerate ranges, angle-mode
ties.  Every comparison is np.array_equal on values, dtypes and shapes.  tf_radlong_select is also driven directly (four slots,
inactive slots, repeated ranks, rank 0 and count - 1), calls of different sizes follow each other on one engine, and a NaN or inf
in the flow raises ValueError before any device histogram runs, the next call being exact."""
import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import analysis as A
from tests import stats_cases as S

pytestmark = pytest.mark.gpu

RAD = S.radlong_cases()
POL = S.polar_cases()
NONFINITE = S.nonfinite_cases()


def _ids(cases):
    return [c.name for c in cases]


def _by_name(name):
    return next(c for c in RAD + POL if c.name == name)


@pytest.mark.parametrize("case", RAD, ids=_ids(RAD))
def test_radlong_statistics_equal_numpy(engine, case):
    S.check_radlong(engine, case)


@pytest.mark.parametrize("case", POL, ids=_ids(POL))
def test_polar_statistics_equal_numpy(engine, case):
    S.check_polar(engine, case)


def _select(engine, which, ranks):
    ranks = np.ascontiguousarray(ranks, np.int64)
    vals = np.full(ranks.shape, -7.0, np.float64)
    _lib.check(engine._L.tf_radlong_select(engine._h, which, ranks.ctypes.data, vals.ctypes.data), engine._h, "tf_radlong_select")
    return vals


SELECT_CASES = [c for c in RAD if c.raises is None and ({"ties", "keys", "percentiles", "degenerate", "big"} & c.tags) and c.param == "velocity"]


@pytest.mark.parametrize("case", SELECT_CASES, ids=_ids(SELECT_CASES))
def test_select_directly_equals_sort(engine, case):
    """four slots with four ranks, inactive slots (-1 -> 0.0), one rank in two slots, rank 0 and count - 1"""
    n = case.n_used
    mm, nz, rad, lon = engine.radlong_project_param(case.flow, case.mask, 0, 1 / case.frame_rate, False, n, case.cent, return_arrays=True)
    rng = np.random.default_rng(n)
    for which, arr in ((0, rad), (1, lon)):
        srt = [np.sort(arr[f].ravel()[arr[f].ravel() != 0]) for f in range(n)]
        assert [len(s) for s in srt] == list(nz[:, which])
        plans = []
        for kind in range(4):
            ranks = np.full((n, 4), -1, np.int64)
            for f in range(n):
                c = len(srt[f])
                if c == 0:
                    continue
                if kind == 0:
                    ranks[f] = [0, c - 1, c // 2, min(c - 1, 1)]
                elif kind == 1:
                    ranks[f] = [c - 1, -1, 0, -1]
                elif kind == 2:
                    r = int(rng.integers(0, c))
                    ranks[f] = [r, r, -1, (r + 1) % c]
                else:
                    ranks[f] = np.sort(rng.integers(0, c, 4))[::-1]
            plans.append(ranks)
        for ranks in plans:
            got = _select(engine, which, ranks)
            want = np.zeros((n, 4), np.float64)
            for f in range(n):
                for j in range(4):
                    if ranks[f, j] >= 0:
                        want[f, j] = srt[f][ranks[f, j]]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (case.name, which, ranks, got, want)


def test_back_to_back_calls_do_not_contaminate_each_other(engine):
    """the resident planes and their frame count belong to the handle: a large call, then smaller ones of another N, size and path, each
    exact, and the statistics of `which` 0 and 1 read the planes of the last projection"""
    order = ["r_image_300x250_velocity", "r_percentiles_0_100", "p_image_300x250_velocity", "r_image_1x1", "p_nbins_7", "r_keys_rays_share_48_key_bits",
             "a_single_pixel", "r_image_300x250_velocity"]
    for name in order:
        c = _by_name(name)
        (S.check_radlong if c.path == "radlong" else S.check_polar)(engine, c)
    # statistics straight after a projection of another shape: which = 1 first, then 0
    big, small = _by_name("r_image_300x250_velocity"), _by_name("r_ties_three_values")
    for first, second in ((big, small), (small, big)):
        engine.radlong_project_param(first.flow, first.mask, 0, 1 / first.frame_rate, False, first.n_used, first.cent)
        n = second.n_used
        _, nz, rad, lon = engine.radlong_project_param(second.flow, second.mask, 0, 1 / second.frame_rate, False, n, second.cent, return_arrays=True)
        for which, arr in ((1, lon), (0, rad)):
            ranks = np.full((n, 4), -1, np.int64)
            ranks[:, 0] = np.where(nz[:, which] > 0, 0, -1)
            ranks[:, 3] = nz[:, which] - 1
            got = _select(engine, which, ranks)
            flat = arr.reshape(n, -1)
            for f in range(n):
                v = flat[f][flat[f] != 0]
                if len(v) == 0:                                              # rank -1 everywhere: nothing is selected
                    assert not got[f].any(), (second.name, which, f)
                    continue
                assert got[f, 0] == v.min() and got[f, 3] == v.max() and got[f, 1] == got[f, 2] == 0.0, (second.name, which, f)
            e = np.linspace(arr.min(), arr.max(), 8)
            freq = np.zeros((n, 7), np.int64)
            _lib.check(engine._L.tf_radlong_hist(engine._h, which, e.ctypes.data, 7, freq.ctypes.data), engine._h, "tf_radlong_hist")
            for f in range(n):
                v = flat[f][flat[f] != 0]
                assert np.array_equal(freq[f], np.histogram(v, bins=7, range=(arr.min(), arr.max()))[0]), (second.name, which, f)


class _Forbidden:
    """stands in for a library entry that must not be reached"""

    def __init__(self, name):
        self.name = name

    def __call__(self, *a):
        raise AssertionError(f"{self.name} was called")


@pytest.mark.parametrize("case", NONFINITE, ids=_ids(NONFINITE))
def test_non_finite_flow_raises_before_the_histogram_and_the_next_call_is_exact(engine, case):
    L = engine._L
    real = L.tf_radlong_hist, L.tf_radlong_select
    L.tf_radlong_hist, L.tf_radlong_select = _Forbidden("tf_radlong_hist"), _Forbidden("tf_radlong_select")
    try:
        if case.path == "radlong":
            with pytest.raises(ValueError, match="not finite"):
                A.param_radlong_stats(case.flow, case.mask, case.param, case.frame_rate, case.n_used, case.cent, nbins=case.nbins, engine=engine)
            with np.errstate(invalid="ignore"):
                field = case.field()
            with pytest.raises(ValueError, match="not finite"):
                A.radlong_stats_device(engine, field, case.cent, nbins=case.nbins)
        else:
            with pytest.raises(ValueError, match="not finite"):
                A.calculate_3dhist(case.study(), case.param, "m", nbins=case.nbins, percentile=case.percentile, engine=engine)
            with pytest.raises(ValueError, match="NaN or inf"):
                A.angle_mode_series(case.study(), case.param, "m", engine=engine)
    finally:
        L.tf_radlong_hist, L.tf_radlong_select = real
    after = _by_name("r_ties_three_values" if case.path == "radlong" else "a_tie_across_waves")
    (S.check_radlong if after.path == "radlong" else S.check_polar)(engine, after)


def test_non_finite_in_a_later_plane_only(engine):
    """a finite radial plane beside a non-finite longitudinal one cannot be planted (inf * 0 is NaN in both), but an overflowing
    float32 magnitude beside finite angles can: the host histogram refuses the range, and so does the device"""
    c = _by_name("p_nbins_7")
    flow = c.flow.astype(np.float32)
    flow[1, 3, 0] = (3e38, 3e38)
    st = A.FlowStudy(flow, {"m": c.mask}, c.frame_rate, nframes=c.n_used)
    with np.errstate(over="ignore"):
        with pytest.raises(ValueError, match="not finite"):
            A.calculate_3dhist(st, "velocity", "m", nbins=7)
    with pytest.raises(ValueError, match="not finite"):
        A.calculate_3dhist(st, "velocity", "m", nbins=7, engine=engine)
    S.check_polar(engine, c)
