"""oracle/deepflow_oracle.c's whole solve against the independent float64 reference tests/deepflow_ref64.py: the 3 x 3 blur, the pyramid
size rule, the pyramid, the flow hand-down, the refinement at the shapes where the device's SOR forms run, then whole solves (identical
level counts, flow within the criterion), and the proof that the comparison would notice each of ten deliberate errors.  No GPU.

Every tolerance is 4 x the oracle-vs-reference deviation recorded in tests/golden/deepflow_ref64_measured.json (deepflow_ref64_cases.tol),
or the north-star rule of the multi-level solves (mean EPE <= 1e-3 px, at most 2 % of the pixels beyond 1e-3 px); the size rule is
integer-exact.  test_tolerances_hold keeps the record honest.  The default pyramids of 97x131 and 150x301 (27 and 36 levels) are not
compared point by point, on purpose: see tests/deepflow_ref64_cases.py."""
import numpy as np
import pytest

from tests import deepflow_ref64 as R
from tests import deepflow_ref64_cases as K

_measured = {}


def measured(oracle, cid):
    if cid not in _measured:
        _measured[cid] = K.measure(oracle, cid)
    return _measured[cid]


def test_tolerances_hold(oracle):
    """The record holds every case of this file and of the GPU file, and what the oracle deviates from the reference by today is at most
    twice what was recorded (the oracle is deterministic: this guards the reference, and the record, against drift)."""
    rec = K.record()
    assert sorted(rec) == sorted(K.all_ids())
    for cid in K.all_ids():
        now = measured(oracle, cid)
        assert sorted(now) == sorted(rec[cid]), cid
        for key, v in now.items():
            assert v <= K.DRIFT_FACTOR * rec[cid][key], f"{cid} {key}: {v:.3g} now, {rec[cid][key]:.3g} recorded"


STAGE_IDS = list(K.BLUR) + list(K.PYR) + list(K.UP) + list(K.REFINE)


@pytest.mark.parametrize("cid", STAGE_IDS)
def test_oracle_stage_matches_reference(oracle, cid):
    """The blur at three sigmas (also on a single row and on an image narrower than the kernel), pyramid levels 0, 1, 2 and the coarsest
    of uint8 and of float frames at three factors, the flow hand-down, and one refinement at the tiled, narrow and co-resident shapes."""
    K.within(cid, measured(oracle, cid))


def test_refinement_cases_move_the_flow():
    """...or their bound would be met by doing nothing"""
    for cid, (shape, _) in K.REFINE.items():
        u = K.refine_case_inputs(shape)[2]
        assert np.abs(K.ref_refine(cid)[0] - u).max() > K.MUTATION_FACTOR * K.tol(cid, "uv"), cid


@pytest.mark.parametrize("sigma", [1 / 3, 0.34, 0.5, 0.6, 0.66])
def test_blur_taps_are_the_oracles_float32_values(oracle, sigma):
    k0, k1 = R.gauss3(sigma)
    ok = oracle.deepflow_gauss3(sigma)
    assert (np.float32(k0), np.float32(k1)) == (ok[0], ok[1])
    assert k0 == float(np.float32(k0)) and k1 == float(np.float32(k1))      # they ARE float32 values: the rounding is in the specification
    assert abs(k0 + 2 * k1 - 1) < 1e-7 and k0 > k1 > 0


def test_blur_border_is_reflect_101():
    a = np.array([[1.0, 2.0, 4.0, 8.0]])
    k0, k1 = R.gauss3(0.6)
    out = R.blur3(a, 0.6)
    row = k0 + 2 * k1                                                        # a single row reflects onto itself
    assert np.allclose(out[0, 0], row * (k0 * 1 + k1 * (2 + 2)), rtol=1e-15)   # the neighbour beyond the edge is the pixel one inside
    assert np.allclose(out[0, 3], row * (k0 * 8 + k1 * (4 + 4)), rtol=1e-15)


# ---- the size rule: integer-exact ---------------------------------------------------------------------------------------------------
def _oracle_sizes(oracle, W, H, **kw):
    return oracle.deepflow_pyramid_sizes(W, H, oracle.deepflow_default_params(**kw))


def test_pyramid_sizes_equal_the_oracle_at_the_default_factor(oracle):
    """every width from 26 to 1100, by a height that follows it at another pace"""
    for W in range(26, 1101):
        H = 26 + (W * 7) % 700
        assert R.pyramid_sizes(W, H, K.params()) == _oracle_sizes(oracle, W, H), (W, H)


@pytest.mark.parametrize("factor", [0.11, 0.5, 0.55, 0.7, 0.8, 0.9, 0.95, 0.97, 0.985])
def test_pyramid_sizes_equal_the_oracle_at_other_factors(oracle, factor):
    for W, H in [(26, 26), (30, 30), (64, 80), (97, 131), (150, 301), (333, 141), (512, 512), (1000, 27), (1920, 1080)]:
        for min_size in (1, 5, 25, 60):
            got = R.pyramid_sizes(W, H, K.params(downscale_factor=factor, min_size=min_size))
            assert got == _oracle_sizes(oracle, W, H, downscale_factor=factor, min_size=min_size), (W, H, factor, min_size)


def test_pyramid_sizes_stop_at_the_cap(oracle):
    """a size rule with a fixed point above min_size never ends by itself: 201 levels, as the oracle and the engine have it"""
    assert R.MAX_LEVELS == oracle.deepflow_max_levels()
    for kw in (dict(min_size=5), dict(downscale_factor=0.985)):
        s = R.pyramid_sizes(64, 64, K.params(**kw))
        assert len(s) == R.MAX_LEVELS and s == _oracle_sizes(oracle, 64, 64, **kw)
    assert R.pyramid_sizes(64, 64, K.params(min_size=5))[-1] == (10, 10)
    assert len(R.pyramid_sizes(1024, 1024, K.params(downscale_factor=0.98))) == 179


# ---- solves -------------------------------------------------------------------------------------------------------------------------
SOLVE_IDS = [(c, b) for c in K.SOLVE for b in range(len(K.SOLVE[c][2]))]


@pytest.mark.parametrize("case,b", SOLVE_IDS, ids=[K.solve_id(c, b) for c, b in SOLVE_IDS])
def test_oracle_solve_matches_reference(oracle, case, b):
    over, (H, W), _, kind, criterion = K.SOLVE[case]
    I0s, I1s = K.solve_pairs(case)
    assert I0s.dtype == (np.float32 if kind == "f32" else np.uint8)
    flow, nl = oracle.deepflow_calc(I0s[b], I1s[b], params=oracle.deepflow_default_params(**over), return_levels=True)
    rf, rl = K.ref_solve(case, b)
    assert nl == rl, "pyramid depth"
    K.check_flow(K.solve_id(case, b), criterion, flow, rf)
    assert np.abs(rf).max() > 0.1                                            # there is a flow to find (one level alone finds little of it)
    if kind == "f32":
        assert 0 <= I0s.min() and I0s.max() <= 1
    # the depths the cases are there for
    assert rl == {"one-level-64x80": 1, "f0.8-96x120": 7, "f0.5-97x131": 2, "defaults-64x80": 19, "f0.8-150x301": 9,
                  "defaults-64x80-f32": 19}[case]


# ---- sensitivity --------------------------------------------------------------------------------------------------------------------
# mutation -> (the smallest case that exercises it, the output it must move); the two size mutations: see the test
MUTATION_CASES = {
    "no_blur": ("blur-30x27-s0.6", "plane"), "sigma_plus_0.05": ("blur-30x27-s0.6", "plane"), "border_reflect": ("blur-3x2-s0.6", "plane"),
    "resize_no_half_pixel": ("pyr-64x80-f0.8-u8", "level1"),
    "no_gain": ("up-33x47-41x59", "plane"), "gain_is_factor": ("up-33x47-41x59", "plane"),
    "nonzero_start": ("one-level-64x80/seed0", "flow_max"), "level0_not_refined": ("one-level-64x80/seed0", "flow_max"),
    "sizes_truncated": None, "sizes_float64": None,
}
FLOAT64_SIZE_DIFFERS_AT = 30          # the first width from 26 on at which the size rule in float64 gives another size (28, not 29)


def _mutated_dev(oracle, mutate, cid, key):
    if cid in K.BLUR:
        _, sigma = K.BLUR[cid]
        src = K.blur_input(cid)
        return K.plane_rel(oracle.deepflow_gauss_blur3(src, sigma), R.blur3(src, sigma, mutate=mutate), 255.0)
    if cid in K.PYR:
        _, f, kind = K.PYR[cid]
        img = K.pyr_input(cid)
        level = int(key[5:])
        ref = R.pyramid(img, K.params(**K.PYR_PARAMS[f]), mutate=mutate)[level]
        return K.plane_rel(oracle.deepflow_pyramid_level(img, level, oracle.deepflow_default_params(**K.PYR_PARAMS[f])), ref, 255.0 if kind == "u8" else 1.0)
    if cid in K.UP:
        _, (dh, dw), f = K.UP[cid]
        u, v = K.up_input(cid)
        ou, _ = oracle.deepflow_upsample(u, v, dw, dh, oracle.deepflow_default_params(downscale_factor=f))
        return K.plane_rel(ou, R.upsample(u, v, dw, dh, f, mutate=mutate)[0], K.UP_AMP)
    case, seed = cid.split("/seed")
    b = K.SOLVE[case][2].index(int(seed))
    I0s, I1s = K.solve_pairs(case)
    flow = oracle.deepflow_calc(I0s[b], I1s[b], params=oracle.deepflow_default_params(**K.SOLVE[case][0]))
    return K.dev_flow(flow, K.ref_solve(case, b, mutate)[0])[key]


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_reference_tells_each_mutation_apart(oracle, mutate):
    """The reference with one deliberate error differs from the oracle by more than 100 x the case's tolerance: the standing proof that
    a kernel and an oracle sharing that error would not pass.  The size rule is compared exactly, so for its two mutations any other
    size is a failure: truncation loses a level of the 96x120 / 0.8 pyramid, and float64 arithmetic gives 30 -> 28 where float32
    gives 30 -> 29 (30 * 0.95f is 28.49999964 before and 28.5 after its rounding to float32)."""
    assert sorted(MUTATION_CASES) == sorted(R.MUTATIONS)
    if mutate == "sizes_truncated":
        P = K.params(downscale_factor=0.8)
        good, bad = R.pyramid_sizes(120, 96, P), R.pyramid_sizes(120, 96, P, mutate=mutate)
        assert good == _oracle_sizes(oracle, 120, 96, downscale_factor=0.8) and len(good) == 7 and len(bad) == 6 and bad[1] != good[1]
        return
    if mutate == "sizes_float64":
        differs = [W for W in range(26, 1101) if R.pyramid_sizes(W, W, K.params(), mutate=mutate) != R.pyramid_sizes(W, W, K.params())]
        W = FLOAT64_SIZE_DIFFERS_AT
        assert differs[0] == W and len(differs) > 100
        good, bad = R.pyramid_sizes(W, W, K.params()), R.pyramid_sizes(W, W, K.params(), mutate=mutate)
        assert good == _oracle_sizes(oracle, W, W) and good[1] == (29, 29) and bad[1] == (28, 28) and len(good) == 5 and len(bad) == 4
        return
    cid, key = MUTATION_CASES[mutate]
    dev = _mutated_dev(oracle, mutate, cid, key)
    need = K.MUTATION_FACTOR * K.tol(cid, key)
    print(f"{mutate} on {cid}: {key} moves by {dev:.3g}, {dev / K.tol(cid, key):.3g} x the tolerance")
    assert dev > need, f"{mutate} on {cid}: {key} moves by {dev:.3g}, needs more than {need:.3g}"


def test_unknown_mutation_is_refused():
    with pytest.raises(ValueError):
        R.blur3(np.zeros((4, 4)), 0.6, mutate="nothing")
    with pytest.raises(ValueError):
        R.solve(np.zeros((4, 4)), np.zeros((4, 4)), K.params(), mutate="nothing")
