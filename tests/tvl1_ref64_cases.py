"""Named, seeded cases for the DualTVL1 float64 reference (tests/tvl1_ref64.py): their inputs, the measurement of the oracle's deviation
from the reference that tests/golden/tvl1_ref64_measured.json records, and the tolerances that come from that record.  A helper module
shared by tests/test_tvl1_ref64_cpu.py, tests/test_gpu_tvl1_ref64.py and tests/golden/make_tvl1_ref64_measured.py: nothing here is
collected.

The tolerance of a case is TOL_FACTOR x its recorded oracle-vs-reference deviation, per output.  The deviation is float32 rounding
noise that grows about linearly with the iteration count, and another equally valid summation order can double it; every mutation of
the reference moves the results by orders of magnitude more (test_reference_tells_each_mutation_apart).  The short multi-stage solves of
the CPU form take the project's own criterion instead (BASELINE.json north_star): cv::remap quantises sample positions to 1/32 px, a
1e-6 difference in u flips that at a few pixels per warp, and the flipped pixels leave rounding noise behind.

No 5-level x 5-warp solve is compared point by point, on purpose: over 25 stages those flips make the trajectories part (iteration counts
differed in 3 of 4 seeds when it was tried, the mean EPE was 2e-4 to 1.4e-2 px), so such a test could only assert a loose statistic."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np

from tests import tvl1_ref64 as R

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tvl1_ref64_measured.json")
TOL_FACTOR = 4.0            # tolerance = TOL_FACTOR x the recorded deviation
DRIFT_FACTOR = 2.0          # test_tolerances_hold: what is measured now <= DRIFT_FACTOR x the record
MUTATION_FACTOR = 100.0     # a mutation must move a result by more than MUTATION_FACTOR x the tolerance
MIN_MARGIN = 1e-3           # every stop test of a solve case stays this far (relative) from its threshold
EPE_MEAN, EPE_PX, EPE_FRACTION = 1e-3, 1e-3, 0.02    # short CPU-form solves: mean EPE <= 1e-3 px, <= 2 % of the pixels beyond 1e-3 px

TRIPLES = {"dflt": (0.15, 0.3, 0.25), "lo": (0.05, 0.25, 0.2), "hi": (1.0, 0.5, 0.125)}     # (lambda, theta, tau)
DEFAULTS = dict(tau=0.25, lambda_=0.15, theta=0.3, nscales=5, warps=5, epsilon=0.01, inner_iterations=30, outer_iterations=10,
                scale_step=0.8, median_filtering=5, variant=0)


def params(**over):
    """The DualTVL1 parameters as a plain object with the oracle's field names."""
    return SimpleNamespace(**{**DEFAULTS, **over})


def oracle_params(oracle, over):
    return oracle.default_params(**over)


def _img(seed, h, w, lo=0.0, hi=255.0):
    return np.random.default_rng(seed).uniform(lo, hi, (h, w)).astype(np.float32)


# ---- warp ---------------------------------------------------------------------------------------------------------------------------
WARP = {"warp-64x64-a3": ((64, 64), 3.0), "warp-97x131-a8": ((97, 131), 8.0), "warp-40x300-a60": ((40, 300), 60.0),
        "warp-20x18-a30": ((20, 18), 30.0), "warp-5x7-a3": ((5, 7), 3.0), "warp-3x40-a3": ((3, 40), 3.0)}     # the last two: narrower than 4 taps
GPU_WARP = ("warp-97x131-a8", "warp-40x300-a60", "warp-5x7-a3")


def warp_inputs(cid):
    """I0, I1, u1, u2 (float32): random frames, flows of the case's amplitude, two samples far outside (the int16 saturation)."""
    (h, w), amp = WARP[cid]
    rng = np.random.default_rng(3)
    I0, I1 = _img(4, h, w), _img(5, h, w)
    u1 = rng.uniform(-amp, amp, (h, w)).astype(np.float32)
    u2 = rng.uniform(-amp, amp, (h, w)).astype(np.float32)
    u1[0, 0] = 1e6
    u2[-1, -1] = -1e6
    return I0, I1, u1, u2


CUDA_WARP = {"cwarp-64x80": (64, 80), "cwarp-40x40": (40, 40)}


def cuda_warp_inputs(cid):
    """Speckle frames, gaussian flows with rows of integer coordinates (five taps, the outer ones weigh 0) and far-outside rows."""
    from tee_optical_flow_amd.synth import speckle_pair
    h, w = CUDA_WARP[cid]
    rng = np.random.default_rng(4)
    I0, I1, _ = speckle_pair(11, h, w)
    u1 = rng.normal(0, 2.0, (h, w)).astype(np.float32)
    u2 = rng.normal(0, 2.0, (h, w)).astype(np.float32)
    u1[::7, ::5] = np.round(u1[::7, ::5])
    u2[::3, ::4] = 0.0
    u1[0, :] = -6.0
    u2[:, -1] = 9.0
    return I0.astype(np.float32), I1.astype(np.float32), u1, u2


def rho_rel(a, b):
    return float((np.abs(a - b) / (np.abs(b) + 255.0)).max())


def dev_warp(got, ref):
    """got = (wx, wy, rho_c) of the oracle or the device, ref = the reference's."""
    return {"wxy": float(max(np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max())), "rho_c": rho_rel(got[2], ref[2])}


# ---- iterate ------------------------------------------------------------------------------------------------------------------------
CPU_ITER = [(97, 131, k, t, pz) for k in (1, 6, 30) for t in TRIPLES for pz in (0, 1)]
GPU_ITER_SHAPES = [(15, 60), (16, 61), (31, 121), (97, 131), (3, 1021)]    # one tile, ragged tiles, odd widths, one strip wide
GPU_ITER_TRIPLES = ("lo", "hi")
GPU_ITER_STEPS = (6, 7)                                                     # 7: an odd total through the two-per-launch forms
GPU_ITER = [(h, w, k, t, pz) for (h, w) in GPU_ITER_SHAPES for k in GPU_ITER_STEPS for t in GPU_ITER_TRIPLES for pz in (0, 1)]


def iter_id(h, w, k, t, pz):
    return f"iter-{h}x{w}-k{k}-{t}-pz{pz}"


ITER = {iter_id(*c): c for c in CPU_ITER + GPU_ITER}


@functools.lru_cache(maxsize=None)
def _iter_planes(h, w):
    """Warp planes of smooth frames (so that all three threshold branches occur) with a patch of zero gradient, and a random state."""
    from scipy import ndimage
    rng = np.random.default_rng(7)
    I0 = ndimage.gaussian_filter(_img(8, h, w), 1.5).astype(np.float32)
    I1 = ndimage.gaussian_filter(_img(9, h, w), 1.5).astype(np.float32)
    u1 = rng.uniform(-1, 1, (h, w)).astype(np.float32)
    u2 = rng.uniform(-1, 1, (h, w)).astype(np.float32)
    wx, wy, rho = (a.astype(np.float32) for a in R.warp(I0, I1, u1, u2))
    wx[min(3, h - 1):6, 3:9] = 0.0
    wy[min(3, h - 1):6, 3:9] = 0.0
    p = [rng.uniform(-0.5, 0.5, (h, w)).astype(np.float32) for _ in range(4)]
    return wx, wy, rho, u1, u2, p


def iter_inputs(cid):
    """(wx, wy, rho_c, u1, u2, p11, p12, p21, p22) float32, nsteps, (lambda, theta, tau), pzero"""
    h, w, k, t, pz = ITER[cid]
    wx, wy, rho, u1, u2, p = _iter_planes(h, w)
    if pz:
        p = [np.zeros((h, w), np.float32) for _ in range(4)]
    return (wx, wy, rho, u1, u2, *p), k, TRIPLES[t], pz


def err_sums(err_q):
    """The exact error sums of the oracle / the device (2^-30 units) as float64."""
    return np.asarray(err_q, np.float64) / 2.0 ** 30


def dev_iter(got, ref):
    """got = (u1, u2, p11, p12, p21, p22, error sums as float64), ref = the reference's."""
    return {"u": float(max(np.abs(got[i] - ref[i]).max() for i in (0, 1))),
            "p": float(max(np.abs(got[i] - ref[i]).max() for i in (2, 3, 4, 5))),
            "err_rel": float((np.abs(got[6] - ref[6]) / ref[6]).max())}


# ---- pyramid and upsample -----------------------------------------------------------------------------------------------------------
PYR = {f"pyr-{h}x{w}-s{s}": ((h, w), s) for (h, w), s in [((97, 131), 0.8), ((97, 131), 0.55), ((97, 131), 0.9), ((17, 16), 0.55), ((17, 16), 0.9)]}
GPU_PYR = tuple(c for c in PYR if not c.endswith("s0.8"))
PYR_LEVELS = (1, 2, 3)


def pyr_input(cid):
    (h, w), _ = PYR[cid]
    return np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8)


def _up(src, dst, mul):
    return f"up-{src[0]}x{src[1]}-{dst[0]}x{dst[1]}", (src, dst, mul)


# the four shapes of test_flow_upsample_resize_bit_exact, then a level 1 -> level 0 step of the pyramids above at their own gain
UP = dict([_up((210, 210), (262, 262), 1.25), _up((33, 47), (41, 59), 1.25), _up((16, 16), (20, 20), 1.25), _up((328, 328), (410, 410), 1.25),
           _up((53, 72), (97, 131), 1 / 0.55), _up((87, 118), (97, 131), 1 / 0.9), _up((9, 9), (17, 16), 1 / 0.55), _up((15, 14), (17, 16), 1 / 0.9)])
GPU_UP = tuple(UP)[4:]
CUDA_RESIZE = dict([_up((97, 131), (78, 105), 1.0), _up((33, 47), (41, 59), 1.25)])
CUDA_RESIZE = {"c" + k: v for k, v in CUDA_RESIZE.items()}


def up_input(cid):
    (sh, sw), _, _ = (UP.get(cid) or CUDA_RESIZE[cid])
    return _img(2, sh, sw, -5, 5)


def dev_plane(got, ref):
    return float(np.abs(got - ref).max())


# ---- solves -------------------------------------------------------------------------------------------------------------------------
ONE = dict(nscales=1, warps=1)
# id -> (parameter overrides, (H, W), seeds, kind of input, criterion)
SOLVE = {
    "one-defaults": (dict(ONE), (72, 88), (0, 1), "u8", "4x"),
    "one-median3": (dict(ONE, median_filtering=3), (72, 88), (0, 1), "u8", "4x"),
    "one-median1": (dict(ONE, median_filtering=1), (72, 88), (0, 1), "u8", "4x"),
    "one-odd-inner": (dict(ONE, inner_iterations=7, outer_iterations=4), (72, 88), (0, 1), "u8", "4x"),
    "one-cap-reached": (dict(ONE, inner_iterations=9, outer_iterations=5, epsilon=1e-4), (72, 88), (0, 1), "u8", "4x"),
    "one-first-outer": (dict(ONE, epsilon=0.05), (72, 88), (0, 1), "u8", "4x"),
    "one-lambda0.05": (dict(ONE, lambda_=0.05), (72, 88), (0, 1), "u8", "4x"),
    "one-lambda1": (dict(ONE, lambda_=1.0), (72, 88), (0, 1), "u8", "4x"),
    "one-tau-theta": (dict(ONE, tau=0.2, theta=0.25), (72, 88), (0, 1), "u8", "4x"),
    "one-f32": (dict(ONE), (72, 88), (0, 1), "f32", "4x"),
    "one-sector": (dict(ONE), (72, 88), (0, 1), "sector", "4x"),
    "truncated-24x40": (dict(warps=1), (24, 40), (7, 8), "u8", "4x"),                  # 24 -> 19 -> 15: two levels of five
    "one-two-warps": (dict(nscales=1, warps=2), (72, 88), (0, 1), "u8", "4x"),          # the duals carried from warp to warp
    "short-3x2": (dict(nscales=3, warps=2), (97, 131), (0, 1), "u8", "epe"),
    "short-2x3-s0.55": (dict(nscales=2, warps=3, scale_step=0.55), (97, 131), (0, 1), "u8", "epe"),
    "short-3x2-median3": (dict(nscales=3, warps=2, median_filtering=3), (97, 131), (0, 2), "u8", "epe"),
    "cuda-one": (dict(ONE, variant=1), (72, 88), (0, 1), "u8", "4x"),
    "cuda-3-levels": (dict(nscales=3, warps=1, variant=1), (97, 131), (0, 1), "u8", "4x"),
}
GPU_SOLVE_TILES_TOO = "one-defaults"         # run once more with iter_variant 0


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
    if kind == "sector":                      # a bright sector on an exactly black background, as real echo frames are
        yy, xx = np.mgrid[0:H, 0:W]
        sector = (np.abs(np.arctan2(xx - W / 2, yy + 8.0)) < 0.6) & (np.hypot(xx - W / 2, yy + 8.0) < H * 0.95)
        I0s, I1s = np.where(sector, I0s, 0).astype(np.uint8), np.where(sector, I1s, 0).astype(np.uint8)
    return np.ascontiguousarray(I0s), np.ascontiguousarray(I1s)


def solve_id(cid, b):
    return f"{cid}/seed{SOLVE[cid][2][b]}"


@functools.lru_cache(maxsize=None)
def ref_solve(cid, b, mutate=None):
    """The reference's (flow, iters, min_margin) of pair b of a case; computed once per process and shared."""
    I0s, I1s = solve_pairs(cid)
    out = R.solve(I0s[b], I1s[b], params(**SOLVE[cid][0]), mutate=mutate)
    out[0].setflags(write=False)
    return out


def dev_flow(got, ref):
    d = got.astype(np.float64) - ref
    epe = np.sqrt((d ** 2).sum(-1))
    return {"flow_max": float(np.abs(d).max()), "flow_mean_epe": float(epe.mean()), "flow_frac_beyond": float((epe > EPE_PX).mean())}


# ---- the measurement the record holds -----------------------------------------------------------------------------------------------
def measure(oracle, cid):
    """The oracle's deviation from the reference for one case id, per output.  Runs the oracle and the reference only."""
    if cid in WARP:
        I0, I1, u1, u2 = warp_inputs(cid)
        wx, wy, _, rho = oracle.warp(I0, I1, u1, u2)
        return dev_warp((wx, wy, rho), R.warp(I0, I1, u1, u2))
    if cid in CUDA_WARP:
        I0, I1, u1, u2 = cuda_warp_inputs(cid)
        h, w = I0.shape
        I1x, I1y = oracle.centered_gradient(I1)
        o = [np.empty((h, w), np.float32) for _ in range(4)]
        oracle.lib().orc_warp_cuda(I0, I1, I1x, I1y, u1, u2, w, h, *o)
        return dev_warp((o[0], o[1], o[3]), R.warp_cuda(I0, I1, u1, u2))
    if cid in ITER:
        st, k, (lam, theta, tau), _ = iter_inputs(cid)
        o = oracle.iterate(st[0], st[1], st[0] * st[0] + st[1] * st[1], *st[2:], k, lam, theta, tau)
        return dev_iter((*o[:6], err_sums(o[6])), R.iterate(*st, k, lam, theta, tau))
    if cid in PYR:
        _, step = PYR[cid]
        img = pyr_input(cid)
        return {f"level{l}": dev_plane(oracle.pyramid_level(img, l, step), R.pyramid_level(img, l, step)) for l in PYR_LEVELS}
    if cid in UP:
        _, (dh, dw), mul = UP[cid]
        src = up_input(cid)
        return {"plane": dev_plane(oracle.resize_linear(src, dw, dh) * np.float32(mul), R.resize_linear(src, dw, dh) * mul)}
    if cid in CUDA_RESIZE:
        _, (dh, dw), mul = CUDA_RESIZE[cid]
        src = up_input(cid)
        return {"plane": dev_plane(oracle.resize_cuda(src, dw, dh) * np.float32(mul), R.resize_cuda(src, dw, dh) * mul)}
    case, b = cid.split("/seed")
    b = SOLVE[case][2].index(int(b))
    I0s, I1s = solve_pairs(case)
    flow, _, _ = oracle.tvl1_calc(I0s[b], I1s[b], oracle_params(oracle, SOLVE[case][0]), return_iters=True)
    rf, _, margin = ref_solve(case, b)
    return {**dev_flow(flow, rf), "min_margin": float(margin)}


def all_ids():
    ids = list(WARP) + list(CUDA_WARP) + list(ITER) + list(PYR) + list(UP) + list(CUDA_RESIZE)
    return ids + [solve_id(c, b) for c in SOLVE for b in range(len(SOLVE[c][2]))]


@functools.lru_cache(maxsize=None)
def record():
    with open(RECORD) as f:
        return json.load(f)


def tol(cid, key):
    """The tolerance of one output of a case: TOL_FACTOR x the recorded oracle-vs-reference deviation."""
    return TOL_FACTOR * record()[cid][key]


def check_flow(sid, criterion, flow, rf):
    """The flow criterion of a solve case: the north-star rule for the short CPU-form solves, 4 x the record for the others."""
    d = dev_flow(flow, rf)
    print(sid, " ".join(f"{k}={v:.3g}" for k, v in d.items()))
    if criterion == "epe":
        assert d["flow_mean_epe"] <= EPE_MEAN and d["flow_frac_beyond"] <= EPE_FRACTION, f"{sid}: {d}"
    else:
        assert d["flow_max"] <= tol(sid, "flow_max") and d["flow_mean_epe"] <= tol(sid, "flow_mean_epe"), f"{sid}: {d}"
