"""The DualTVL1 kernels against the independent float64 reference tests/tvl1_ref64.py, and -- new at non-default constants -- bit-equal
to the oracle: tf_dbg_iterate in all four forms on handles with other (lambda, theta, tau), tf_dbg_pyramid / tf_dbg_resize at other
scale steps, tf_dbg_warp in its three staging forms and the CUDA-class form, and single-stage and short solves through calc_pairs.

Every tolerance comes from tests/golden/tvl1_ref64_measured.json, which records what the ORACLE deviates from the reference by on the
CPU (tvl1_ref64_cases.tol: 4 x the record); none comes from a device run.  The reference results are computed here, once per case.
Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import tvl1_ref64 as R
from tests import tvl1_ref64_cases as K
from tests.tvl1_forms import iter_form

pytestmark = pytest.mark.gpu


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def handles():
    """DualTVL1 handles by their non-default parameters, made on first use."""
    import tee_optical_flow_amd as T
    made = {}

    def get(**params):
        key = tuple(sorted(params.items()))
        if key not in made:
            made[key] = T.DenseFlow(**params)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def within(cid, dev):
    for key, v in dev.items():
        print(f"{cid} {key}: {v:.3g} (tolerance {K.tol(cid, key):.3g})")
    for key, v in dev.items():
        assert v <= K.tol(cid, key), f"{cid} {key}: {v:.3g} > {K.tol(cid, key):.3g}"


# ---- tf_dbg_iterate -----------------------------------------------------------------------------------------------------------------
_iter_refs = {}


def iter_refs(oracle, cid):
    """(reference, oracle) results of an iterate case, computed once and shared by the four forms"""
    if cid not in _iter_refs:
        st, k, (lam, theta, tau), _ = K.iter_inputs(cid)
        _iter_refs[cid] = (R.iterate(*st, k, lam, theta, tau),
                           oracle.iterate(st[0], st[1], st[0] * st[0] + st[1] * st[1], *st[2:], k, lam, theta, tau))
    return _iter_refs[cid]


@pytest.mark.parametrize("triple", K.GPU_ITER_TRIPLES)
@pytest.mark.parametrize("shape", K.GPU_ITER_SHAPES)
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_iterate_at_other_constants(handles, oracle, form, shape, triple):
    """6 and 7 steps of tvl1_iter with (lambda, theta, tau) = (0.05, 0.25, 0.2) and (1.0, 0.5, 0.125), from a random and from a zero dual
    state, in the four forms (tiles, row strips, two per launch on strips, two per launch on tiles; an odd total takes the two-per-launch
    forms' one-per-launch fall-back, as an odd `inner` does in a solve): state and error sums within tolerance of the reference and
    bit-equal to the oracle run with the same constants."""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    lam, theta, tau = K.TRIPLES[triple]
    eng = handles(lambda_=lam, theta=theta, tau=tau)
    with iter_form(eng, form):
        for k in K.GPU_ITER_STEPS:
            for pz in (0, 1):
                cid = K.iter_id(*shape, k, triple, pz)
                st, nsteps, _, _ = K.iter_inputs(cid)
                ref, orc = iter_refs(oracle, cid)
                h, w = shape
                dev = [a.copy() for a in st[3:]]
                err = np.zeros(nsteps, np.uint64)
                _lib.check(L.tf_dbg_iterate(eng._h, _ptr(st[0]), _ptr(st[1]), _ptr(st[2]), *[_ptr(a) for a in dev], w, h, nsteps, pz,
                                            _ptr(err)), eng._h)
                within(cid, K.dev_iter((*dev, K.err_sums(err)), ref))
                for n, a, r in zip(["u1", "u2", "p11", "p12", "p21", "p22"], dev, orc[:6]):
                    assert np.array_equal(a, r), f"{cid} {n}: {np.sum(a != r)} px differ from the oracle, max {np.abs(a - r).max()}"
                assert np.array_equal(err, orc[6]), cid


# ---- tf_dbg_pyramid, tf_dbg_resize --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", K.GPU_PYR)
def test_pyramid_at_other_scale_steps(handles, oracle, cid):
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    (h, w), step = K.PYR[cid]
    eng = handles(scale_step=step)
    img = K.pyr_input(cid)
    dev = {}
    for level in K.PYR_LEVELS:
        ref = R.pyramid_level(img, level, step)
        ow, oh = C.c_int(), C.c_int()
        _lib.check(L.tf_dbg_pyramid(eng._h, _ptr(img), h, w, level, None, C.byref(ow), C.byref(oh)), eng._h)
        assert (oh.value, ow.value) == ref.shape
        out = np.empty(ref.shape, np.float32)
        _lib.check(L.tf_dbg_pyramid(eng._h, _ptr(img), h, w, level, _ptr(out), C.byref(ow), C.byref(oh)), eng._h)
        dev[f"level{level}"] = K.dev_plane(out, ref)
        assert np.array_equal(out, oracle.pyramid_level(img, level, step)), f"level {level} differs from the oracle"
    within(cid, dev)


@pytest.mark.parametrize("cid", K.GPU_UP)
def test_flow_upsample_at_other_scale_steps(handles, oracle, cid):
    """level 1 -> level 0 of the pyramids above, times 1 / scale_step, as a solve upsamples its flow"""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    (sh, sw), (dh, dw), mul = K.UP[cid]
    eng = handles(scale_step=round(1 / mul, 6))
    src = K.up_input(cid)
    out = np.empty((dh, dw), np.float32)
    _lib.check(L.tf_dbg_resize(eng._h, _ptr(src), sw, sh, _ptr(out), dw, dh, dw / sw, dh / sh, mul), eng._h)
    within(cid, {"plane": K.dev_plane(out, R.resize_linear(src, dw, dh) * mul)})
    assert np.array_equal(out, oracle.resize_linear(src, dw, dh) * np.float32(mul))


# ---- tf_dbg_warp --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [0, 2, 8])
@pytest.mark.parametrize("cid", K.GPU_WARP)
def test_warp_against_reference(engine, oracle, cid, margin):
    """global gathers (margin 0) and the LDS-staged tile with a margin of 2 and 8, also on an image narrower than the 4-tap window"""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    I0, I1, u1, u2 = K.warp_inputs(cid)
    h, w = I0.shape
    wx, wy, rho = (np.empty((h, w), np.float32) for _ in range(3))
    engine.set_tuning("warp_margin", margin)
    try:
        _lib.check(L.tf_dbg_warp(engine._h, _ptr(I0), _ptr(I1), _ptr(u1), _ptr(u2), w, h, _ptr(wx), _ptr(wy), _ptr(rho)), engine._h)
    finally:
        engine.set_tuning("warp_margin", 0)
    within(cid, K.dev_warp((wx, wy, rho), R.warp(I0, I1, u1, u2)))
    o = oracle.warp(I0, I1, u1, u2)
    assert np.array_equal(wx, o[0]) and np.array_equal(wy, o[1]) and np.array_equal(rho, o[3])


@pytest.mark.parametrize("cid", list(K.CUDA_WARP))
def test_cuda_class_warp_against_reference(handles, cid):
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    eng = handles(variant="cuda")
    I0, I1, u1, u2 = K.cuda_warp_inputs(cid)
    h, w = I0.shape
    wx, wy, rho = (np.empty((h, w), np.float32) for _ in range(3))
    _lib.check(L.tf_dbg_warp(eng._h, _ptr(I0), _ptr(I1), _ptr(u1), _ptr(u2), w, h, _ptr(wx), _ptr(wy), _ptr(rho)), eng._h)
    within(cid, K.dev_warp((wx, wy, rho), R.warp_cuda(I0, I1, u1, u2)))


# ---- solves -------------------------------------------------------------------------------------------------------------------------
def solve_case(oracle, case, form):
    import tee_optical_flow_amd as T
    over, _, seeds, _, criterion = K.SOLVE[case]
    I0s, I1s = K.solve_pairs(case)
    eng = T.DenseFlow(**{k: ("cuda" if k == "variant" and v == 1 else v) for k, v in over.items()})
    try:
        with iter_form(eng, form):
            flows = eng.calc_pairs(I0s, I1s)
            iters = eng.last_iters()
            levels = eng.last_stats["nscales_used"]
    finally:
        eng.close()
    for b in range(len(seeds)):
        rf, rit, margin = K.ref_solve(case, b)
        assert margin >= K.MIN_MARGIN
        assert levels == rit.shape[0], "pyramid depth"
        assert np.array_equal(iters[b], rit), f"pair {b} iteration counts:\n{iters[b].tolist()}\n{rit.tolist()}"
        K.check_flow(K.solve_id(case, b), criterion, flows[b], rf)
        assert np.array_equal(flows[b], oracle.tvl1_calc(I0s[b], I1s[b], K.oracle_params(oracle, over))), f"pair {b} differs from the oracle"


@pytest.mark.parametrize("case", list(K.SOLVE))
def test_solve_against_reference(oracle, case):
    """The case's pairs as one batch on the strip forms: the reference's iteration counts and pyramid depth exactly, its flow within the
    case's criterion, and the oracle's flow bit for bit."""
    solve_case(oracle, case, "strips2")          # the strip forms, even for this small batch


def test_solve_against_reference_on_tiles(oracle):
    solve_case(oracle, K.GPU_SOLVE_TILES_TOO, "tiles")
