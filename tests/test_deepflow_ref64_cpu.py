"""oracle/deepflow_oracle.c's VariationalRefinement::calcUV against an independent float64 restatement (tests/deepflow_ref64.py), at
non-default parameters and iteration counts; and the pyramid depth cap the oracle and the HIP engine share.

The GPU path is built to equal the oracle bit for bit, so these tests are what would catch an error made in both.  They compare
float32 arithmetic with float64 within 1e-4 px.  The inputs are chosen so the comparison is well-conditioned.  The fixed-point loop
re-linearises the robust penalties at the current increment.  Where a residual passes near zero, their slope grows like 1/eps^2,
and rounding can then grow over the loop.  This happens with a small epsilon over several loops, or with one over-relaxed sweep per
loop.  A small epsilon is therefore compared over one fixed-point iteration, where the system itself is what is checked, and a large
omega with several sweeps per iteration."""
import os
import re

import numpy as np
import pytest

from tests import deepflow_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4     # px; float32 against float64 on these inputs stays near 1e-5


def smooth_field(rng, h, w, amp):
    from scipy import ndimage
    a = ndimage.gaussian_filter(rng.standard_normal((h, w)), 4, mode="wrap")
    return (a / np.abs(a).max() * amp).astype(np.float32)


def refine_inputs(h, w, seed):
    """A smooth textured frame spanning 0..255, its neighbour shifted by (0.7, -1.2) px, and a smooth initial flow of up to 1.5 px."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    I0 = ndimage.gaussian_filter(rng.uniform(0, 255, (h, w)), 3)
    I0 = (I0 - I0.min()) / (I0.max() - I0.min()) * 255
    I1 = ndimage.shift(I0, (0.7, -1.2), order=1, mode="nearest")
    return I0.astype(np.float32), I1.astype(np.float32), smooth_field(rng, h, w, 1.5), smooth_field(rng, h, w, 1.5)


def oracle_refine(oracle, I0, I1, u, v, p):
    """One calcUV with the constants OpticalFlowDeepFlow derives from its parameters, in float32 as the engine computes them."""
    f = np.float32
    return oracle.deepflow_variational_refine(I0, I1, u, v, alpha=f(4) * f(p.alpha), delta=f(p.delta) / f(3),
                                              gamma=f(p.gamma) / f(3), params=p)


SHAPES = [(40, 48), (33, 57), (1, 37), (23, 2)]

CASES = [
    {},                                                           # the defaults: 5 fixed-point iterations x 25 sweeps, omega 1.6
    *[dict(fixed_point_iterations=fp, sor_iterations=sor) for fp in (1, 2, 7) for sor in (1, 2, 7, 26)],
    dict(omega=1.0), dict(omega=1.0, fixed_point_iterations=2, sor_iterations=7),
    dict(omega=1.9), dict(omega=1.9, fixed_point_iterations=2, sor_iterations=26), dict(omega=1.9, fixed_point_iterations=7, sor_iterations=7),
    dict(alpha=2.0), dict(alpha=0.5), dict(alpha=0.5, fixed_point_iterations=2, sor_iterations=7),
    dict(delta=0.0), dict(delta=1.0, fixed_point_iterations=2, sor_iterations=7),
    dict(gamma=0.0), dict(gamma=10.0, fixed_point_iterations=2, sor_iterations=7),
    dict(delta=0.0, gamma=0.0, sor_iterations=7),
    dict(zeta=0.01), dict(zeta=0.01, fixed_point_iterations=7, sor_iterations=2),
    dict(epsilon=1e-5, fixed_point_iterations=1, sor_iterations=26), dict(zeta=0.01, epsilon=1e-5, fixed_point_iterations=1, sor_iterations=7),
    dict(fixed_point_iterations=0), dict(sor_iterations=0),
]


def _id(kw):
    return ",".join(f"{k[:3]}={v}" for k, v in kw.items()) or "defaults"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kw", CASES, ids=_id)
def test_refinement_matches_float64_red_black_sor(oracle, kw, shape):
    h, w = shape
    I0, I1, u, v = refine_inputs(h, w, seed=h * w)
    p = oracle.deepflow_default_params(**kw)
    ou, ov = oracle_refine(oracle, I0, I1, u, v, p)
    ru, rv = R.refine_params(I0, I1, u, v, p)
    err = max(np.abs(ou - ru).max(), np.abs(ov - rv).max())
    assert err <= TOL, f"oracle vs float64: {err:.3g} px (the refinement moved the flow by up to {np.abs(ru - u).max():.3g} px)"
    if p.fixed_point_iterations and p.sor_iterations:
        assert np.abs(ru - u).max() > 100 * TOL                  # the case did move the flow: the bound is not met by doing nothing


@pytest.mark.parametrize("shape,seed", [((40, 48), 5), ((29, 35), 6)])
def test_refinement_converges_to_the_exact_solution_of_its_system(oracle, shape, seed):
    """One fixed-point iteration of 3000 sweeps against a sparse direct solve of the same system: checks the assembled system alone,
    whatever the sweep order."""
    h, w = shape
    I0, I1, u, v = refine_inputs(h, w, seed)
    p = oracle.deepflow_default_params(fixed_point_iterations=1, sor_iterations=3000)
    ou, ov = oracle_refine(oracle, I0, I1, u, v, p)
    ru, rv = R.refine_params(I0, I1, u, v, p, exact=True)
    err = max(np.abs(ou - ru).max(), np.abs(ov - rv).max())
    assert err <= TOL, f"oracle after 3000 sweeps vs the exact solution: {err:.3g} px"
    su, sv = R.refine_params(I0, I1, u, v, oracle.deepflow_default_params(fixed_point_iterations=1, sor_iterations=3))
    assert max(np.abs(su - ru).max(), np.abs(sv - rv).max()) > 100 * TOL   # 3 sweeps are far from it: the solve is not trivial


def test_reference_warp_and_derivatives_match_the_oracle_planes(oracle):
    """The reference's own building blocks against the oracle's (float32 against float64 of the same formulas)."""
    I0, I1, u, v = refine_inputs(31, 45, 3)
    u = u * 3
    mine = R.derivatives(I0, I1, u, v)
    theirs = oracle.deepflow_derivatives(I0, I1, u, v)
    for name, t in zip(("Ix", "Iy", "Iz", "Ixx", "Ixy", "Iyy", "Ixz", "Iyz"), theirs):
        assert np.abs(mine[name] - t).max() <= 1e-3, name       # values up to a few hundred
    assert np.abs(oracle.deepflow_warp_linear(I1, u, v) - R.warp_bilinear(I1, u, v)).max() <= 1e-4


# ---- the pyramid depth cap ----------------------------------------------------------------------------------------------------
def test_pyramid_depth_cap(oracle):
    """At most 200 downscales (201 levels).  A size rule with a fixed point above min_size never ends by itself; the default pyramids
    are far from the cap."""
    cap = oracle.deepflow_max_levels()
    assert cap == 201
    s = oracle.deepflow_pyramid_sizes(64, 64, oracle.deepflow_default_params(min_size=5))
    assert len(s) == cap and s[-1] == (10, 10) and s[-2] == (10, 10)          # (int)(10 * 0.95 + 0.5) = 10
    assert len(oracle.deepflow_pyramid_sizes(64, 64, oracle.deepflow_default_params(downscale_factor=0.985))) == cap
    assert len(oracle.deepflow_pyramid_sizes(1024, 1024, oracle.deepflow_default_params(downscale_factor=0.98))) == 179
    assert len(oracle.deepflow_pyramid_sizes(512, 512)) == 60
    assert len(oracle.deepflow_pyramid_sizes(2048, 2048)) == 87


def test_deep_pyramid_solve_stops_at_the_cap(oracle):
    from tee_optical_flow_amd.synth import speckle_pair
    I0, I1, _ = speckle_pair(3, 64, 64)
    f, n = oracle.deepflow_calc(I0, I1, params=oracle.deepflow_default_params(min_size=5), return_levels=True)
    assert n == oracle.deepflow_max_levels() and np.isfinite(f).all()


def test_hip_engine_caps_the_pyramid_at_the_same_depth(oracle):
    """The engine's DF_MAXLEV and the oracle's cap are one rule written in two files."""
    src = open(os.path.join(ROOT, "tee_optical_flow_amd", "csrc", "teeflow_engine.hip.h")).read()
    m = re.search(r"constexpr int DF_MAXLEV = (\d+);", src)
    assert m and int(m.group(1)) == oracle.deepflow_max_levels()
