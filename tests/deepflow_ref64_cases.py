"""Named, seeded cases for the DeepFlow float64 reference (tests/deepflow_ref64.py): their inputs, the measurement of the oracle's
deviation from the reference that tests/golden/deepflow_ref64_measured.json records, and the tolerances that come from that record.  A
helper module shared by tests/test_deepflow_ref64_stages_cpu.py, tests/test_gpu_deepflow_ref64.py and
tests/golden/make_deepflow_ref64_measured.py: nothing here is collected.

The constants are DualTVL1's (tests/tvl1_ref64_cases.py): the tolerance of a case is TOL_FACTOR x its recorded oracle-vs-reference
deviation, per output; the multi-level solves take the project's own criterion (mean EPE <= EPE_MEAN, at most EPE_FRACTION of the pixels
beyond EPE_PX), because cv::remap quantises sample positions to 1/32 px, a 1e-6 difference in the flow flips that at a few pixels per
level, and the flipped pixels leave rounding noise behind.

Solve depths left out, on purpose: the default pyramids of 97x131 (27 levels) and 150x301 (36 levels), and every pyramid much deeper
than 20 levels.  Over that many levels the flips make the float32 and the float64 trajectories part: oracle against reference on the CPU
gave 6.9 % and 24.5 % of the pixels beyond 1e-3 px there (mean EPE 3.2e-4 and 8.2e-4 px), so such a case could only assert a loose
statistic.  The solve cases here have 1 to 19 levels, where the oracle stays well inside the criterion (the record shows by how much)."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np

from tests import deepflow_ref64 as R
from tests.test_deepflow_ref64_cpu import CASES as CPU_REFINE_CASES, oracle_refine, refine_inputs
from tests.tvl1_ref64_cases import DRIFT_FACTOR, EPE_FRACTION, EPE_MEAN, MUTATION_FACTOR, TOL_FACTOR, dev_flow  # noqa: F401

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deepflow_ref64_measured.json")

DEFAULTS = dict(sigma=0.6, min_size=25, downscale_factor=0.95, fixed_point_iterations=5, sor_iterations=25, alpha=1.0, delta=0.5, gamma=5.0,
                omega=1.6, zeta=0.1, epsilon=0.001)


def params(**over):
    """DeepFlow's parameters as a plain object with the oracle's field names."""
    return SimpleNamespace(**{**DEFAULTS, **over})


def _img(seed, h, w, lo=0.0, hi=255.0):
    return np.random.default_rng(seed).uniform(lo, hi, (h, w)).astype(np.float32)


def plane_rel(a, b, scale):
    """The largest deviation of a plane relative to its values' range `scale` (of the kind tvl1_ref64_cases.rho_rel is)."""
    return float((np.abs(a - b) / (np.abs(b) + scale)).max())


# ---- blur ---------------------------------------------------------------------------------------------------------------------------
BLUR_SHAPES = [(1, 40), (3, 2), (30, 27), (97, 131)]     # a side of length 1, narrower than the kernel's reach, odd, several blocks
BLUR_SIGMAS = (0.34, 0.6, 0.66)                           # the 3 x 3 kernel covers 1/3 <= sigma < 2/3
BLUR = {f"blur-{h}x{w}-s{s}": ((h, w), s) for (h, w) in BLUR_SHAPES for s in BLUR_SIGMAS}


def blur_input(cid):
    (h, w), _ = BLUR[cid]
    return _img(0, h, w)


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------
# factor 0.5 with min_size 10: with the default 25 these frames would have two levels only
PYR_PARAMS = {0.95: {}, 0.8: dict(downscale_factor=0.8), 0.5: dict(downscale_factor=0.5, min_size=10)}
PYR = {f"pyr-{h}x{w}-f{f}-{kind}": ((h, w), f, kind) for (h, w) in [(97, 131), (64, 80)] for f in PYR_PARAMS for kind in ("u8", "f32")}


def pyr_input(cid):
    """A uint8 frame, or a float32 frame in [0, 1] with detail below 1 / 255."""
    (h, w), _, kind = PYR[cid]
    rng = np.random.default_rng(1)
    if kind == "u8":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    return rng.random((h, w), dtype=np.float32)


def pyr_levels(cid):
    """The levels a pyramid case checks: 0, 1, 2 and the coarsest (by the reference's size rule)."""
    (h, w), f, _ = PYR[cid]
    n = len(R.pyramid_sizes(w, h, params(**PYR_PARAMS[f])))
    return sorted({l for l in (0, 1, 2, n - 1) if l < n})


# ---- the flow hand-down -------------------------------------------------------------------------------------------------------------
def _up(src, dst, factor):
    return f"up-{src[0]}x{src[1]}-{dst[0]}x{dst[1]}", (src, dst, factor)


# (H, W) -> (H, W): the coarsest default step, an odd one, a doubling, a wide level of several blocks, a single row
UP = dict([_up((26, 26), (27, 27), 0.95), _up((33, 47), (41, 59), 0.8), _up((49, 66), (97, 131), 0.5), _up((143, 286), (150, 301), 0.95),
           _up((1, 40), (1, 42), 0.95)])
UP_AMP = 5.0


def up_input(cid):
    (sh, sw), _, _ = UP[cid]
    return _img(2, sh, sw, -UP_AMP, UP_AMP), _img(3, sh, sw, -UP_AMP, UP_AMP)


# ---- refinement ---------------------------------------------------------------------------------------------------------------------
# where the device's SOR forms run: tiled 97x131; narrow 40x52, 100x33; co-resident 150x301, 65x129
REFINE_SHAPES = [(97, 131), (40, 52), (100, 33), (150, 301), (65, 129)]
# from test_deepflow_ref64_cpu.CASES, by its conditioning rules: a small epsilon over one fixed-point iteration only, a large omega with
# several sweeps per iteration
REFINE_PARAMS = {
    "defaults": {},
    "fp2-sor7": dict(fixed_point_iterations=2, sor_iterations=7),
    "omega1.9": dict(omega=1.9, fixed_point_iterations=2, sor_iterations=26),
    "alpha0.5": dict(alpha=0.5, fixed_point_iterations=2, sor_iterations=7),
    "gamma10": dict(gamma=10.0, fixed_point_iterations=2, sor_iterations=7),
    "zeta0.01": dict(zeta=0.01),
    "eps1e-5": dict(epsilon=1e-5, fixed_point_iterations=1, sor_iterations=26),
    "no-gradient-term": dict(delta=0.0, gamma=0.0, sor_iterations=7),
}
assert all(kw in CPU_REFINE_CASES for kw in REFINE_PARAMS.values())


def refine_id(shape, pid):
    return f"refine-{shape[0]}x{shape[1]}-{pid}"


REFINE = {refine_id(s, pid): (s, pid) for s in REFINE_SHAPES for pid in REFINE_PARAMS}


@functools.lru_cache(maxsize=None)
def refine_case_inputs(shape):
    h, w = shape
    return refine_inputs(h, w, seed=h * w)


@functools.lru_cache(maxsize=None)
def ref_refine(cid):
    """The reference's (u, v) of a refinement case; computed once per process and shared."""
    shape, pid = REFINE[cid]
    out = R.refine_params(*refine_case_inputs(shape), params(**REFINE_PARAMS[pid]))
    for a in out:
        a.setflags(write=False)
    return out


def dev_uv(got, ref):
    return {"uv": float(max(np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max()))}


# ---- solves -------------------------------------------------------------------------------------------------------------------------
# id -> (parameter overrides, (H, W), seeds, kind of input, criterion).  The seeds were chosen on the CPU, by the oracle's distance from the
# criterion and nothing else: at 19 levels that distance already depends on the pair (speckle seed 5 at 64x80 leaves 2.1 % of the pixels
# beyond 1e-3 px, float seeds 1 and 2 leave 1.5 %), which is why nothing deeper is compared.
SOLVE = {
    "one-level-64x80": (dict(min_size=64), (64, 80), (0, 1), "u8", "4x"),              # blur, zero start, one refinement: no hand-down
    "f0.8-96x120": (dict(downscale_factor=0.8), (96, 120), (0, 1), "u8", "epe"),        # 7 levels
    "f0.5-97x131": (dict(downscale_factor=0.5), (97, 131), (0, 1), "u8", "epe"),        # 2 levels
    "defaults-64x80": ({}, (64, 80), (0, 1), "u8", "epe"),                              # 19 levels
    "f0.8-150x301": (dict(downscale_factor=0.8), (150, 301), (0, 1), "u8", "epe"),      # 9 levels, co-resident regions on the fine ones
    "defaults-64x80-f32": ({}, (64, 80), (0, 4), "f32", "epe"),                         # float frames in [0, 1], taken as they are
}
GPU_SOLVE_COOP_TOO = "f0.8-150x301"          # run once more with sor_coop 2


@functools.lru_cache(maxsize=None)
def solve_pairs(cid):
    """The case's pairs as two stacks [B, H, W] (uint8, or float32 in [0, 1])."""
    from tee_optical_flow_amd.synth import speckle_pairs
    _, (H, W), seeds, kind, _ = SOLVE[cid]
    I0s, I1s = speckle_pairs(list(seeds), H, W)
    if kind == "f32":                         # not just u8 / 255: sub-level detail, so that the float path is really exercised
        rng = np.random.default_rng(seeds[0])
        I0s = (I0s.astype(np.float32) + rng.random(I0s.shape, dtype=np.float32)) / np.float32(256)
        I1s = (I1s.astype(np.float32) + rng.random(I1s.shape, dtype=np.float32)) / np.float32(256)
    return np.ascontiguousarray(I0s), np.ascontiguousarray(I1s)


def solve_id(cid, b):
    return f"{cid}/seed{SOLVE[cid][2][b]}"


@functools.lru_cache(maxsize=None)
def ref_solve(cid, b, mutate=None):
    """The reference's (flow, levels) of pair b of a case; computed once per process and shared."""
    I0s, I1s = solve_pairs(cid)
    out = R.solve(I0s[b], I1s[b], params(**SOLVE[cid][0]), mutate=mutate)
    out[0].setflags(write=False)
    return out


# ---- the measurement the record holds -----------------------------------------------------------------------------------------------
def measure(oracle, cid):
    """The oracle's deviation from the reference for one case id, per output.  Runs the oracle and the reference only."""
    if cid in BLUR:
        _, sigma = BLUR[cid]
        src = blur_input(cid)
        return {"plane": plane_rel(oracle.deepflow_gauss_blur3(src, sigma), R.blur3(src, sigma), 255.0)}
    if cid in PYR:
        _, f, kind = PYR[cid]
        img = pyr_input(cid)
        ref = R.pyramid(img, params(**PYR_PARAMS[f]))
        p = oracle.deepflow_default_params(**PYR_PARAMS[f])
        return {f"level{l}": plane_rel(oracle.deepflow_pyramid_level(img, l, p), ref[l], 255.0 if kind == "u8" else 1.0) for l in pyr_levels(cid)}
    if cid in UP:
        _, (dh, dw), f = UP[cid]
        u, v = up_input(cid)
        ou, ov = oracle.deepflow_upsample(u, v, dw, dh, oracle.deepflow_default_params(downscale_factor=f))
        ru, rv = R.upsample(u, v, dw, dh, f)
        return {"plane": max(plane_rel(ou, ru, UP_AMP), plane_rel(ov, rv, UP_AMP))}
    if cid in REFINE:
        shape, pid = REFINE[cid]
        return dev_uv(oracle_refine(oracle, *refine_case_inputs(shape), oracle.deepflow_default_params(**REFINE_PARAMS[pid])), ref_refine(cid))
    case, b = cid.split("/seed")
    b = SOLVE[case][2].index(int(b))
    I0s, I1s = solve_pairs(case)
    flow = oracle.deepflow_calc(I0s[b], I1s[b], params=oracle.deepflow_default_params(**SOLVE[case][0]))
    return dev_flow(flow, ref_solve(case, b)[0])


def all_ids():
    ids = list(BLUR) + list(PYR) + list(UP) + list(REFINE)
    return ids + [solve_id(c, b) for c in SOLVE for b in range(len(SOLVE[c][2]))]


@functools.lru_cache(maxsize=None)
def record():
    with open(RECORD) as f:
        return json.load(f)


def tol(cid, key):
    """The tolerance of one output of a case: TOL_FACTOR x the recorded oracle-vs-reference deviation."""
    return TOL_FACTOR * record()[cid][key]


def within(cid, dev):
    """Print every figure of a case, then hold each to its tolerance."""
    for key, v in dev.items():
        print(f"{cid} {key}: {v:.3g} (tolerance {tol(cid, key):.3g})")
    for key, v in dev.items():
        assert v <= tol(cid, key), f"{cid} {key}: {v:.3g} > {tol(cid, key):.3g}"


def check_flow(sid, criterion, flow, rf):
    """The flow criterion of a solve case: the north-star rule for the multi-level solves, 4 x the record for the one-level one."""
    d = dev_flow(flow, rf)
    print(sid, " ".join(f"{k}={v:.3g}" for k, v in d.items()))
    if criterion == "epe":
        assert d["flow_mean_epe"] <= EPE_MEAN and d["flow_frac_beyond"] <= EPE_FRACTION, f"{sid}: {d}"
    else:
        assert d["flow_max"] <= tol(sid, "flow_max") and d["flow_mean_epe"] <= tol(sid, "flow_mean_epe"), f"{sid}: {d}"
