"""oracle/tvl1_oracle.c against the independent float64 reference tests/tvl1_ref64.py: operator by operator, then whole single-stage and
short solves (identical iteration counts and pyramid depth, flow within tolerance), and the proof that the comparison would notice each
of eleven deliberate errors.  No GPU.

Every tolerance is 4 x the oracle-vs-reference deviation recorded in tests/golden/tvl1_ref64_measured.json (tvl1_ref64_cases.tol), or
the north-star rule of the short CPU-form solves (mean EPE <= 1e-3 px, at most 2 % of the pixels beyond 1e-3 px).  test_tolerances_hold
keeps the record honest.  There is no 5-level x 5-warp point-wise comparison, on purpose: cv::remap quantises sample positions to
1/32 px, a 1e-6 difference in u flips that at a few pixels per warp, and over 25 stages the two trajectories part (iteration counts
differed in 3 of 4 seeds, mean EPE 2e-4 to 1.4e-2 px); the cases here stop at 6 stages."""
import numpy as np
import pytest

from tests import tvl1_ref64 as R
from tests import tvl1_ref64_cases as K

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
            if key != "min_margin":
                assert v <= K.DRIFT_FACTOR * rec[cid][key], f"{cid} {key}: {v:.3g} now, {rec[cid][key]:.3g} recorded"


OPERATOR_IDS = list(K.WARP) + list(K.ITER) + list(K.PYR) + list(K.UP) + list(K.CUDA_WARP) + list(K.CUDA_RESIZE)


@pytest.mark.parametrize("cid", OPERATOR_IDS)
def test_oracle_operator_matches_reference(oracle, cid):
    """Warp (also narrower than the 4-tap window, also far outside), k iterations at three (lambda, theta, tau) from a random and from
    a zero dual state over a patch of zero gradient, pyramid levels 1-3 at three scale steps, the flow upsampling, and the CUDA-class
    variant's warp and resize."""
    for key, v in measured(oracle, cid).items():
        print(f"{cid} {key}: {v:.3g} (tolerance {K.tol(cid, key):.3g})")
        assert v <= K.tol(cid, key), f"{cid} {key}: {v:.3g} > {K.tol(cid, key):.3g}"


def test_iterate_cases_take_all_three_threshold_branches():
    """...or the iterate cases would not test the thresholding step"""
    for t in K.TRIPLES:
        st, _, (lam, theta, _), _ = K.iter_inputs(K.iter_id(97, 131, 1, t, 0))
        wx, wy, rho_c, u1, u2 = (a.astype(np.float64) for a in st[:5])
        grad, rho = wx * wx + wy * wy, rho_c + wx * u1 + wy * u2
        lt = lam * theta
        below, above = rho < -lt * grad, rho > lt * grad
        assert below.sum() > 20 and above.sum() > 20 and (~below & ~above & (grad > R.FLT_EPSILON)).sum() > 20, t
        assert (grad <= R.FLT_EPSILON).sum() >= 18


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("shape", [(64, 64), (97, 131), (5, 7), (1, 40)])
def test_median_is_exactly_equal(oracle, shape, ksize):
    src = np.random.default_rng(6).uniform(-3, 3, shape).astype(np.float32)
    src[::7, ::5] = 0.0     # ties
    assert np.array_equal(oracle.median_blur(src, ksize), R.median(src.astype(np.float64), ksize))
    assert R.median(src, 1) is src


def test_centered_gradient_and_size_rule(oracle):
    a = np.random.default_rng(2).integers(0, 256, (9, 13)).astype(np.float32)
    gx, gy = R.centered_gradient(a)
    ox, oy = oracle.centered_gradient(a)
    assert np.array_equal(ox, gx) and np.array_equal(oy, gy)            # differences of whole numbers are exact in float32
    assert np.array_equal(gx[:, 0], 0.5 * (a[:, 1].astype(np.float64) - a[:, 0]))
    for n in (5, 15, 25, 35, 97, 131, 250):
        for step in (0.5, 0.55, 0.8, 0.9):
            assert R.scaled_size(n, step) == oracle.scaled_size(n, step)
    assert R.scaled_size(5, 0.5) == 2 and R.scaled_size(15, 0.5) == 8     # half to even


SOLVE_IDS = [(c, b) for c in K.SOLVE for b in range(len(K.SOLVE[c][2]))]


@pytest.mark.parametrize("case,b", SOLVE_IDS, ids=[K.solve_id(c, b) for c, b in SOLVE_IDS])
def test_oracle_solve_matches_reference(oracle, case, b):
    over, _, _, _, criterion = K.SOLVE[case]
    I0s, I1s = K.solve_pairs(case)
    flow, it, nl = oracle.tvl1_calc(I0s[b], I1s[b], K.oracle_params(oracle, over), return_iters=True)
    rf, rit, margin = K.ref_solve(case, b)
    assert margin >= K.MIN_MARGIN, f"a stop test of the reference comes within {margin:.2g} of its threshold: choose another seed"
    assert nl == rit.shape[0], "pyramid depth"
    assert np.array_equal(it[:nl], rit), f"iteration counts:\n{it[:nl].tolist()}\n{rit.tolist()}"
    K.check_flow(K.solve_id(case, b), criterion, flow, rf)
    # what the case is there for
    P = K.params(**over)
    if case == "one-cap-reached":
        assert rit[0, 0].tolist() == [P.inner_iterations * P.outer_iterations, P.outer_iterations]
    if case == "one-first-outer":
        assert rit[0, 0, 1] == 1 and rit[0, 0, 0] < P.inner_iterations
    if case == "one-odd-inner":
        assert P.inner_iterations % 2 == 1 and rit[0, 0, 0] > P.inner_iterations
    if case == "truncated-24x40":
        assert nl == 2 < P.nscales
    if case.startswith("short") or case == "cuda-3-levels":
        assert nl == P.nscales and (rit[..., 0] > 0).all()


# mutation -> (the smallest case that exercises it, the output it must move)
MUTATION_CASES = {
    "div_first_row": ("iter-15x60-k6-lo-pz0", "u"), "div_first_col": ("iter-15x60-k6-lo-pz0", "u"),
    "taut_product": ("iter-15x60-k6-lo-pz0", "u"), "lt_lambda_only": ("iter-15x60-k6-lo-pz0", "u"),
    "threshold_sign": ("iter-15x60-k6-lo-pz0", "u"), "fwd_grad_wraps": ("iter-15x60-k6-lo-pz0", "u"),
    "grad_border_full": ("warp-5x7-a3", "wxy"), "cubic_a_-0.5": ("warp-5x7-a3", "wxy"),
    "median_after": ("one-defaults/seed0", "flow_max"), "duals_reset_per_warp": ("one-two-warps/seed0", "flow_max"),
    "no_upsample_gain": ("truncated-24x40/seed7", "flow_max"),
}


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_reference_tells_each_mutation_apart(oracle, mutate):
    """The reference with one deliberate error differs from the oracle by more than 100 x the case's tolerance: the standing proof that
    a kernel and an oracle sharing that error would not pass."""
    assert sorted(MUTATION_CASES) == sorted(R.MUTATIONS)
    cid, key = MUTATION_CASES[mutate]
    if cid in K.ITER:
        st, k, (lam, theta, tau), _ = K.iter_inputs(cid)
        o = oracle.iterate(st[0], st[1], st[0] * st[0] + st[1] * st[1], *st[2:], k, lam, theta, tau)
        dev = K.dev_iter((*o[:6], K.err_sums(o[6])), R.iterate(*st, k, lam, theta, tau, mutate=mutate))[key]
    elif cid in K.WARP:
        I0, I1, u1, u2 = K.warp_inputs(cid)
        wx, wy, _, rho = oracle.warp(I0, I1, u1, u2)
        dev = K.dev_warp((wx, wy, rho), R.warp(I0, I1, u1, u2, mutate=mutate))[key]
    else:
        case, seed = cid.split("/seed")
        b = K.SOLVE[case][2].index(int(seed))
        I0s, I1s = K.solve_pairs(case)
        flow = oracle.tvl1_calc(I0s[b], I1s[b], K.oracle_params(oracle, K.SOLVE[case][0]))
        dev = K.dev_flow(flow, K.ref_solve(case, b, mutate)[0])[key]
    need = K.MUTATION_FACTOR * K.tol(cid, key)
    print(f"{mutate} on {cid}: {key} moves by {dev:.3g}, {dev / K.tol(cid, key):.3g} x the tolerance")
    assert dev > need, f"{mutate} on {cid}: {key} moves by {dev:.3g}, needs more than {need:.3g}"


def test_unknown_mutation_is_refused():
    z = np.zeros((4, 4))
    with pytest.raises(ValueError):
        R.iterate(z, z, z, z, z, z, z, z, z, 1, mutate="nothing")
