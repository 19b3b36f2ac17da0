"""DeepFlow on the GPU at non-default parameters, against oracle/deepflow_oracle.c run with the same parameters: bit-exact.

The default-parameter tests (test_gpu_deepflow.py) only ever cut 25 sweeps into SOR launches.  Here the sweep and fixed-point counts
move through every branch of df_refine_level / launch_sor_rt: the fuse cap, the 6-sweep cap of 128 x 32 regions, the narrow levels'
single launch, the co-resident form's `left > S` guard and phase parity, and the du / du2 parity after the tiled loop.  The other nine
parameters are moved one at a time through full solves; the lanes must carry them; creation refuses what the engine cannot do."""
import ctypes as C

import numpy as np
import pytest

from tests import deepflow_ref64 as R

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def handles():
    """DeepFlow handles by (fixed_point_iterations, sor_iterations), made on first use."""
    import tee_optical_flow_amd as T
    made = {}

    def get(fp, sor):
        if (fp, sor) not in made:
            made[(fp, sor)] = T.DenseFlow(algo="deepflow", fixed_point_iterations=fp, sor_iterations=sor)
        return made[(fp, sor)]
    yield get
    for e in made.values():
        e.close()


def refine_inputs(h, w, seed):
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    I0 = ndimage.gaussian_filter(rng.uniform(0, 255, (h, w)), 1.5).astype(np.float32)
    I1 = ndimage.shift(I0, (0.7, -1.2), order=1, mode="nearest").astype(np.float32)
    return I0, I1, rng.uniform(-2, 2, (h, w)).astype(np.float32), rng.uniform(-2, 2, (h, w)).astype(np.float32)


def gpu_refine(eng, I0, I1, u, v, knobs):
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    h, w = I0.shape
    gu, gv = u.copy(), v.copy()
    for k, val in knobs.items():
        eng.set_tuning(k, val)
    try:
        _lib.check(L.tf_dbg_df_refine(eng._h, _ptr(I0), _ptr(I1), w, h, _ptr(gu), _ptr(gv)), eng._h)
    finally:
        for k, val in DEFAULT_KNOBS.items():
            eng.set_tuning(k, val)
    return gu, gv


def oracle_refine(oracle, I0, I1, u, v, p):
    f = np.float32
    return oracle.deepflow_variational_refine(I0, I1, u, v, alpha=f(4) * f(p.alpha), delta=f(p.delta) / f(3),
                                              gamma=f(p.gamma) / f(3), params=p)


DEFAULT_KNOBS = {"sor_fuse": 5, "sor_rt_shape": 3, "sor_coop": 1, "sor_coop_s": 5, "sor_plain_div": 0}
TILED = (97, 131)          # two regions across, several down: a tiled level
NARROW = (40, 52)          # w <= 62: two bands per wave, all sweeps in one launch
NARROW_TALL = (100, 33)
COOP = (150, 301)          # 3 x 3 co-resident 128 x 64 regions

# (fixed_point_iterations, sor_iterations, shape, knobs): chosen so every branch sees remainders, caps and both parities
FORMS = [
    # one colour per launch, in place (sor_fuse 0)
    (1, 1, TILED, dict(sor_fuse=0)), (3, 2, TILED, dict(sor_fuse=0)), (1, 7, TILED, dict(sor_fuse=0)),
    # 128 x 64 regions, n sweeps per launch: remainders of 1..4 after full launches, the fuse cap of 8 (12 -> 8)
    (1, 2, TILED, dict(sor_fuse=1, sor_rt_shape=1)), (3, 5, TILED, dict(sor_fuse=1, sor_rt_shape=1)),
    (1, 0, TILED, dict(sor_fuse=5, sor_rt_shape=1)), (0, 26, TILED, dict(sor_fuse=5, sor_rt_shape=1)),
    (3, 1, TILED, dict(sor_fuse=5, sor_rt_shape=1)), (1, 5, TILED, dict(sor_fuse=5, sor_rt_shape=1)),
    (1, 7, TILED, dict(sor_fuse=5, sor_rt_shape=1)), (3, 9, TILED, dict(sor_fuse=5, sor_rt_shape=1)),
    (1, 26, TILED, dict(sor_fuse=5, sor_rt_shape=1)), (1, 41, TILED, dict(sor_fuse=5, sor_rt_shape=1)),
    (1, 7, TILED, dict(sor_fuse=8, sor_rt_shape=1)), (1, 8, TILED, dict(sor_fuse=8, sor_rt_shape=1)),
    (1, 9, TILED, dict(sor_fuse=8, sor_rt_shape=1)), (3, 24, TILED, dict(sor_fuse=8, sor_rt_shape=1)),
    (1, 41, TILED, dict(sor_fuse=8, sor_rt_shape=1)), (1, 26, TILED, dict(sor_fuse=12, sor_rt_shape=1)),
    # 128 x 32 regions: at most 6 sweeps per launch once 8 are asked for (9 = 6 + 3, 26 = 4 x 6 + 2, 41 = 6 x 6 + 5); 7 runs as one
    (1, 5, TILED, dict(sor_fuse=8, sor_rt_shape=2)), (1, 7, TILED, dict(sor_fuse=8, sor_rt_shape=2)),
    (1, 9, TILED, dict(sor_fuse=8, sor_rt_shape=2)), (3, 26, TILED, dict(sor_fuse=8, sor_rt_shape=2)),
    (1, 41, TILED, dict(sor_fuse=8, sor_rt_shape=2)), (1, 24, TILED, dict(sor_fuse=5, sor_rt_shape=2)),
    # the launcher's own choice, tiled
    (3, 9, TILED, dict(sor_coop=0)), (1, 41, TILED, dict(sor_coop=0)),
    # narrow levels: every sweep in one launch, out of place (du / du2 parity after one launch per fixed-point iteration)
    (1, 1, NARROW, {}), (3, 2, NARROW, {}), (1, 41, NARROW, {}), (0, 9, NARROW, {}), (3, 8, NARROW_TALL, {}), (1, 26, NARROW_TALL, {}),
    # co-resident regions (sor_coop 2: even for one pair): skipped while sor_iterations <= S, else ceil(sor / S) phases, odd or even
    (1, 1, COOP, dict(sor_coop=2, sor_coop_s=1)), (3, 2, COOP, dict(sor_coop=2, sor_coop_s=1)), (1, 9, COOP, dict(sor_coop=2, sor_coop_s=1)),
    (1, 2, COOP, dict(sor_coop=2, sor_coop_s=3)), (1, 7, COOP, dict(sor_coop=2, sor_coop_s=3)), (3, 24, COOP, dict(sor_coop=2, sor_coop_s=3)),
    (1, 8, COOP, dict(sor_coop=2, sor_coop_s=4)), (3, 9, COOP, dict(sor_coop=2, sor_coop_s=4)), (1, 24, COOP, dict(sor_coop=2, sor_coop_s=4)),
    (1, 5, COOP, dict(sor_coop=2, sor_coop_s=5)), (1, 26, COOP, dict(sor_coop=2, sor_coop_s=5)), (3, 41, COOP, dict(sor_coop=2, sor_coop_s=5)),
    (0, 26, COOP, dict(sor_coop=2, sor_coop_s=5)),
]


def _form_id(f):
    fp, sor, shape, knobs = f
    return f"fp{fp}-sor{sor}-{shape[0]}x{shape[1]}-" + ("-".join(f"{k}{v}" for k, v in knobs.items()) or "auto")


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_refinement_in_every_sor_form_at_non_default_counts(handles, oracle, form):
    fp, sor, (h, w), knobs = form
    eng = handles(fp, sor)
    I0, I1, u, v = refine_inputs(h, w, seed=fp * 100 + sor)
    ru, rv = oracle_refine(oracle, I0, I1, u, v, oracle.deepflow_default_params(fixed_point_iterations=fp, sor_iterations=sor))
    before = eng.counter("coop_launches")
    gu, gv = gpu_refine(eng, I0, I1, u, v, knobs)
    if knobs.get("sor_coop") == 2:
        runs = sor > knobs["sor_coop_s"]
        assert eng.counter("coop_launches") == before + (fp if runs else 0)     # the form ran once per fixed-point iteration, or not at all
        assert eng.counter("coop_aborts") == 0
    assert np.array_equal(gu, ru), f"u: {np.sum(gu != ru)} differ, max {np.abs(gu - ru).max()}"
    assert np.array_equal(gv, rv), f"v: {np.sum(gv != rv)} differ, max {np.abs(gv - rv).max()}"
    if fp and sor:
        assert not np.array_equal(gu, u)


def test_refinement_converges_to_the_float64_exact_solution(handles):
    """Ties the GPU to an independent reference, not only to the oracle: one fixed-point iteration of 2000 sweeps."""
    I0, I1, u, v = refine_inputs(40, 48, seed=77)
    eng = handles(1, 2000)
    gu, gv = gpu_refine(eng, I0, I1, u, v, {})
    p = type("P", (), dict(alpha=1.0, delta=0.5, gamma=5.0, zeta=0.1, epsilon=0.001, omega=1.6,
                           fixed_point_iterations=1, sor_iterations=2000))
    ru, rv = R.refine_params(I0, I1, u, v, p, exact=True)
    err = max(np.abs(gu - ru).max(), np.abs(gv - rv).max())
    assert err <= 1e-4, f"GPU after 2000 sweeps vs the float64 exact solution: {err:.3g} px"
    assert np.abs(ru - u).max() > 0.05


# ---- full solves, one parameter changed at a time --------------------------------------------------------------------------------
SOLVES = [
    (dict(min_size=1), 64, 64), (dict(min_size=5), 64, 64), (dict(min_size=60), 96, 120),
    (dict(downscale_factor=0.5), 160, 200), (dict(downscale_factor=0.8), 120, 160), (dict(downscale_factor=0.97), 96, 96),
    (dict(sigma=0.34), 97, 131), (dict(sigma=0.66), 97, 131),
    (dict(omega=1.0), 96, 96), (dict(omega=1.9), 96, 96),
    (dict(zeta=0.01), 96, 96), (dict(epsilon=1e-5), 96, 96),
    (dict(alpha=0.0), 80, 96), (dict(alpha=2.0), 80, 96),
    (dict(delta=0.0), 80, 96), (dict(delta=1.0), 80, 96),
    (dict(gamma=0.0), 80, 96), (dict(gamma=10.0), 80, 96),
    (dict(fixed_point_iterations=3), 80, 96), (dict(sor_iterations=9), 80, 96),
]


def _solve(oracle, kw, H, W, knobs=None, seed=0):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_pairs
    I0s, I1s = speckle_pairs(range(seed, seed + 2), H, W)
    p = oracle.deepflow_default_params(**kw)
    eng = T.DenseFlow(algo="deepflow", **kw)
    try:
        for k, v in (knobs or {}).items():
            eng.set_tuning(k, v)
        flows = eng.calc_pairs(I0s, I1s)
        nl = eng.last_stats["nscales_used"]
    finally:
        eng.close()
    for b in range(2):
        ref, rl = oracle.deepflow_calc(I0s[b], I1s[b], params=p, return_levels=True)
        assert nl == rl, f"pyramid levels: engine {nl}, oracle {rl}"
        assert np.array_equal(flows[b], ref), f"pair {b}: {np.sum(flows[b] != ref)} values differ, max {np.abs(flows[b] - ref).max()}"
    return flows, nl


@pytest.mark.parametrize("kw,H,W", SOLVES, ids=lambda x: str(x) if isinstance(x, int) else ",".join(f"{k}={v}" for k, v in x.items()))
def test_full_solve_with_one_parameter_changed(oracle, kw, H, W):
    flows, nl = _solve(oracle, kw, H, W)
    assert nl == len(oracle.deepflow_pyramid_sizes(W, H, oracle.deepflow_default_params(**kw)))
    default = oracle.deepflow_calc(*[a[0] for a in _pairs(H, W)])
    assert not np.array_equal(flows[0], default), "the parameter did not move the result"


def _pairs(H, W):
    from tee_optical_flow_amd.synth import speckle_pairs
    return speckle_pairs(range(0, 2), H, W)


def test_zeta_small_with_plain_division(oracle):
    """zeta = 0.01 drives the SOR diagonals toward the range where the pre-scaled division is not exact; the plain path, forced."""
    _solve(oracle, dict(zeta=0.01), 96, 96, knobs={"sor_plain_div": 1})


def test_deep_pyramid_stops_where_the_oracle_stops(oracle):
    """64^2 with min_size 5: the size rule reaches 10 x 10 and stays there, so only the depth cap ends the pyramid (201 levels)."""
    _, nl = _solve(oracle, dict(min_size=5), 64, 64, seed=4)
    assert nl == oracle.deepflow_max_levels() == 201


# ---- parameters through the lanes ----------------------------------------------------------------------------------------------
def test_non_default_parameters_reach_every_lane(oracle):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_sequence
    kw = dict(sor_iterations=9, fixed_point_iterations=3, downscale_factor=0.9)
    fr = speckle_sequence(9, 7, 72, 80)                      # 7 frames: 6 pairs
    I0s, I1s = np.ascontiguousarray(fr[:-1]), np.ascontiguousarray(fr[1:])
    out = {}
    for name, mb, knobs in (("alone", 128, {"queue_lanes": 0}), ("two lanes", 128, {}), ("sub-batches", 2, {}), ("sequence", 128, {})):
        eng = T.DenseFlow(algo="deepflow", max_batch=mb, **kw)
        try:
            for k, v in knobs.items():
                eng.set_tuning(k, v)
            if name == "sequence":
                out[name] = np.array(eng.wait(eng.submit_batch(fr)))
            else:
                out[name] = np.array(eng.calc_pairs(I0s, I1s))
            if name == "sub-batches":
                assert eng.counter("queue_units_done") >= 3
        finally:
            eng.close()
    for name, f in out.items():
        assert np.array_equal(f, out["alone"]), f"{name} differs from the handle solving alone"
    p = oracle.deepflow_default_params(**kw)
    for b in (0, 3, 5):
        assert np.array_equal(out["alone"][b], oracle.deepflow_calc(I0s[b], I1s[b], params=p)), f"pair {b}"


def test_float_frames_with_small_zeta(oracle):
    """Saliency maps in [0, 1] go in as they are; zeta is then the knob that matters (0.01 here)."""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_pairs
    I0s, I1s = speckle_pairs(range(20, 22), 96, 112)
    f0, f1 = (I0s / np.float32(255)).astype(np.float32), (I1s / np.float32(255)).astype(np.float32)
    p = oracle.deepflow_default_params(zeta=0.01)
    eng = T.DenseFlow(algo="deepflow", zeta=0.01)
    try:
        flows = np.array(eng.calc_pairs(f0, f1))
        one = np.array(eng.calc(f0[1], f1[1], None))
    finally:
        eng.close()
    for b in range(2):
        assert np.array_equal(flows[b], oracle.deepflow_calc(f0[b], f1[b], params=p)), f"pair {b}"
    assert np.array_equal(one, flows[1])
    assert not np.array_equal(flows[0], oracle.deepflow_calc(f0[0], f1[0]))


# ---- refusals at creation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(sigma=0.333), dict(sigma=2 / 3), dict(downscale_factor=0.1), dict(downscale_factor=1.0),
                                dict(min_size=0), dict(fixed_point_iterations=-1), dict(sor_iterations=-1),
                                dict(fixed_point_iterations=1001), dict(sor_iterations=10001), dict(lambda_=0.15)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refused_at_creation(kw):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
    with pytest.raises(OpticalFlowCalculationError):
        T.DenseFlow(algo="deepflow", **kw).close()


@pytest.mark.parametrize("kw", [dict(sigma=1 / 3), dict(sigma=0.66), dict(fixed_point_iterations=1000, sor_iterations=10000),
                                dict(fixed_point_iterations=0, sor_iterations=0, min_size=1)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_accepted_at_creation(kw):
    import tee_optical_flow_amd as T
    T.DenseFlow(algo="deepflow", **kw).close()
