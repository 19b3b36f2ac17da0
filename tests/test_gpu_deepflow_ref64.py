"""The DeepFlow kernels against the independent float64 reference tests/deepflow_ref64.py, and bit-equal to the oracle run with the same
parameters: the 3 x 3 blur (tf_dbg_df_blur), the pyramid of uint8 and of float frames with the engine's own level table
(tf_dbg_df_pyramid), the flow hand-down k_df_up (tf_dbg_df_up), one refinement in a representative of every SOR form family
(tf_dbg_df_refine), and whole solves through calc_pairs.

Every tolerance comes from tests/golden/deepflow_ref64_measured.json, which records what the ORACLE deviates from the reference by on
the CPU (deepflow_ref64_cases.tol: 4 x the record); none comes from a device run.  The reference results are computed here, once per
case.  Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import deepflow_ref64 as R
from tests import deepflow_ref64_cases as K

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def handles():
    """DeepFlow handles by their non-default parameters, made on first use."""
    import tee_optical_flow_amd as T
    made = {}

    def get(**params):
        key = tuple(sorted(params.items()))
        if key not in made:
            made[key] = T.DenseFlow(algo="deepflow", **params)
        return made[key]
    yield get
    for e in made.values():
        e.close()


# ---- tf_dbg_df_blur -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(K.BLUR))
def test_blur_against_reference(handles, oracle, cid):
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    (h, w), sigma = K.BLUR[cid]
    eng = handles(sigma=sigma)
    src = K.blur_input(cid)
    out = np.empty_like(src)
    _lib.check(L.tf_dbg_df_blur(eng._h, _ptr(src), w, h, _ptr(out)), eng._h)
    K.within(cid, {"plane": K.plane_rel(out, R.blur3(src, sigma), 255.0)})
    assert np.array_equal(out, oracle.deepflow_gauss_blur3(src, sigma))


# ---- tf_dbg_df_pyramid --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(K.PYR))
def test_pyramid_against_reference(handles, oracle, cid):
    """levels 0, 1, 2 and the coarsest of a uint8 frame (0..255) and of a float frame in [0, 1] (taken as it is); the engine's level
    table has the reference's sizes and ends where the reference's does"""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    (h, w), f, kind = K.PYR[cid]
    over = K.PYR_PARAMS[f]
    eng = handles(**over)
    img = K.pyr_input(cid)
    ref = R.pyramid(img, K.params(**over))
    p = oracle.deepflow_default_params(**over)
    ow, oh = C.c_int(), C.c_int()
    dev = {}
    for level in K.pyr_levels(cid):
        _lib.check(L.tf_dbg_df_pyramid(eng._h, _ptr(img), int(kind == "f32"), h, w, level, None, C.byref(ow), C.byref(oh)), eng._h)
        assert (oh.value, ow.value) == ref[level].shape
        out = np.empty(ref[level].shape, np.float32)
        _lib.check(L.tf_dbg_df_pyramid(eng._h, _ptr(img), int(kind == "f32"), h, w, level, _ptr(out), C.byref(ow), C.byref(oh)), eng._h)
        dev[f"level{level}"] = K.plane_rel(out, ref[level], 255.0 if kind == "u8" else 1.0)
        assert np.array_equal(out, oracle.deepflow_pyramid_level(img, level, p)), f"level {level} differs from the oracle"
    K.within(cid, dev)
    assert L.tf_dbg_df_pyramid(eng._h, _ptr(img), int(kind == "f32"), h, w, len(ref), None, C.byref(ow), C.byref(oh)) == _lib.TF_ERR_INVALID_ARG, \
        "the engine's pyramid is deeper than the reference's"


# ---- tf_dbg_df_up -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(K.UP))
def test_flow_hand_down_against_reference(handles, oracle, cid):
    """k_df_up from one level geometry to the next: widths that are no multiple of 64, heights that are no multiple of 4, one block and
    several, a single row; times 1.0f / downscale_factor"""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    (sh, sw), (dh, dw), f = K.UP[cid]
    eng = handles(downscale_factor=f)
    u, v = K.up_input(cid)
    ou, ov = np.empty((dh, dw), np.float32), np.empty((dh, dw), np.float32)
    _lib.check(L.tf_dbg_df_up(eng._h, _ptr(u), _ptr(v), sw, sh, _ptr(ou), _ptr(ov), dw, dh), eng._h)
    ru, rv = R.upsample(u, v, dw, dh, f)
    K.within(cid, {"plane": max(K.plane_rel(ou, ru, K.UP_AMP), K.plane_rel(ov, rv, K.UP_AMP))})
    qu, qv = oracle.deepflow_upsample(u, v, dw, dh, oracle.deepflow_default_params(downscale_factor=f))
    assert np.array_equal(ou, qu) and np.array_equal(ov, qv)


# ---- tf_dbg_df_refine ---------------------------------------------------------------------------------------------------------------
DEFAULT_KNOBS = {"sor_fuse": 5, "sor_rt_shape": 3, "sor_coop": 1, "sor_coop_s": 5, "sor_plain_div": 0}
# one representative per form family of test_gpu_deepflow_params.FORMS: (shape, knobs)
REFINE_FORMS = {
    "single-colour": ((97, 131), dict(sor_fuse=0)),
    "fused-128x64": ((97, 131), dict(sor_fuse=5, sor_rt_shape=1)),
    "fused-128x32": ((97, 131), dict(sor_fuse=8, sor_rt_shape=2)),
    "narrow": ((40, 52), {}),
    "narrow-tall": ((100, 33), {}),
    "coop-s3": ((150, 301), dict(sor_coop=2, sor_coop_s=3)),
    "coop-s5": ((150, 301), dict(sor_coop=2, sor_coop_s=5)),
    "coop-s3-65x129": ((65, 129), dict(sor_coop=2, sor_coop_s=3)),
    "coop-s5-65x129": ((65, 129), dict(sor_coop=2, sor_coop_s=5)),
}
_oracle_refined = {}


@pytest.mark.parametrize("pid", list(K.REFINE_PARAMS))
@pytest.mark.parametrize("form", list(REFINE_FORMS))
def test_refinement_against_reference(handles, oracle, form, pid):
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    shape, knobs = REFINE_FORMS[form]
    cid = K.refine_id(shape, pid)
    over = K.REFINE_PARAMS[pid]
    eng = handles(**over)
    I0, I1, u, v = K.refine_case_inputs(shape)
    P = K.params(**over)
    h, w = shape
    gu, gv = u.copy(), v.copy()
    before = eng.counter("coop_launches")
    for k, val in knobs.items():
        eng.set_tuning(k, val)
    try:
        _lib.check(L.tf_dbg_df_refine(eng._h, _ptr(I0), _ptr(I1), w, h, _ptr(gu), _ptr(gv)), eng._h)
    finally:
        for k, val in DEFAULT_KNOBS.items():
            eng.set_tuning(k, val)
    if knobs.get("sor_coop") == 2:
        runs = P.sor_iterations > knobs["sor_coop_s"]
        assert eng.counter("coop_launches") == before + (P.fixed_point_iterations if runs else 0)   # once per fixed-point iteration, or not at all
        assert eng.counter("coop_aborts") == 0
    K.within(cid, K.dev_uv((gu, gv), K.ref_refine(cid)))
    if cid not in _oracle_refined:
        _oracle_refined[cid] = K.oracle_refine(oracle, I0, I1, u, v, oracle.deepflow_default_params(**over))
    ru, rv = _oracle_refined[cid]
    assert np.array_equal(gu, ru), f"u: {np.sum(gu != ru)} differ from the oracle, max {np.abs(gu - ru).max()}"
    assert np.array_equal(gv, rv), f"v: {np.sum(gv != rv)} differ from the oracle, max {np.abs(gv - rv).max()}"


# ---- solves -------------------------------------------------------------------------------------------------------------------------
def solve_case(oracle, case, knobs):
    import tee_optical_flow_amd as T
    over, _, seeds, _, criterion = K.SOLVE[case]
    I0s, I1s = K.solve_pairs(case)
    eng = T.DenseFlow(algo="deepflow", **over)
    try:
        for k, val in knobs.items():
            eng.set_tuning(k, val)
        flows = eng.calc_pairs(I0s, I1s)
        levels = eng.last_stats["nscales_used"]
        if knobs.get("sor_coop") == 2:
            assert eng.counter("coop_launches") > 0 and eng.counter("coop_aborts") == 0
    finally:
        eng.close()
    p = oracle.deepflow_default_params(**over)
    for b in range(len(seeds)):
        rf, rl = K.ref_solve(case, b)
        assert levels == rl, "pyramid depth"
        K.check_flow(K.solve_id(case, b), criterion, flows[b], rf)
        assert np.array_equal(flows[b], oracle.deepflow_calc(I0s[b], I1s[b], params=p)), f"pair {b} differs from the oracle"


@pytest.mark.parametrize("case", list(K.SOLVE))
def test_solve_against_reference(oracle, case):
    """The case's two pairs as one batch, the launcher's own choice of SOR forms: the reference's level count exactly, its flow within
    the case's criterion, and the oracle's flow bit for bit."""
    solve_case(oracle, case, {})


def test_solve_against_reference_on_coresident_regions(oracle):
    solve_case(oracle, K.GPU_SOLVE_COOP_TOO, {"sor_coop": 2})
