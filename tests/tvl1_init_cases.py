"""DualTVL1 with useInitialFlow: the cases, the two CPU restatements the device is compared with, and the criterion.  A helper module
shared by tests/test_tvl1_init_cpu.py and tests/test_gpu_tvl1_init.py: nothing here is collected.

oracle/tvl1_oracle.c refuses the flag, so the bit-exact checker is `composed`: the oracle's solve restated in Python over the stages
the oracle exports (pyramid_level, warp, median_blur, iterate one step at a time, resize_linear), seeded by the rule of
include/teeflow.h: u?s[0] = split(flow); u?s[s] = resize(u?s[s-1], Size(), scaleStep, scaleStep, INTER_LINEAR) * (float)scaleStep, every
level rounded to float32; the coarsest level starts from its level of that chain.  composed(init=None) is the oracle's own solve bit
for bit (test_tvl1_init_cpu.py), which is what ties the restatement to the oracle.  `ref_init` is the same solve over the float64
stages of tests/tvl1_ref64.py; the criterion against it is the project's own for short multi-stage solves (tvl1_ref64_cases).

`seed_error` names one deliberate error in composed's seeding (SEED_ERRORS) for the sensitivity test; nothing else may pass it."""
import functools

import numpy as np

from tests import tvl1_ref64 as R
from tests import tvl1_ref64_cases as K

FLT_MAX = float(np.finfo(np.float32).max)
SEED_ERRORS = ("no_gain", "gain_inverse", "direct", "size_ratio")

# id -> (parameter overrides, (H, W), seeds, largest magnitude of the initial flow in px)
CASES = {
    "one": (dict(nscales=1, warps=1), (72, 88), (0, 1), 1.5),
    "one-two-warps": (dict(nscales=1, warps=2), (72, 88), (0, 1), 1.5),
    "one-big": (dict(nscales=1, warps=1), (72, 88), (0, 1), 6.0),
    "trunc-24x40": (dict(warps=1), (24, 40), (7, 8), 1.5),                       # 24 -> 19 -> 15: two levels of five
    "short-3x2": (dict(nscales=3, warps=2), (97, 131), (0, 1), 1.5),
    "short-2x3-s0.55": (dict(nscales=2, warps=3, scale_step=0.55), (97, 131), (0, 1), 1.5),
    "odd-37x53": (dict(warps=1), (37, 53), (3, 4), 1.5),                         # five levels, odd sizes on every one
}
TILES_TOO = ("one", "odd-37x53")              # run once more with iter_variant 0
SENSITIVE = ("short-3x2", "odd-37x53", "short-2x3-s0.55")     # the cases with a chain to get wrong


def initial_flow(seed, H, W, amp):
    """A smooth random field float32 [H, W, 2] whose largest component is `amp` px in magnitude."""
    from scipy.ndimage import gaussian_filter
    f = gaussian_filter(np.random.default_rng(100 + seed).standard_normal((H, W, 2)), (6, 6, 0))
    return (f * (amp / np.abs(f).max())).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_inputs(cid):
    """(I0s, I1s uint8 [B, H, W], inits float32 [B, H, W, 2]) of a case, read-only."""
    from tee_optical_flow_amd.synth import speckle_pairs
    _, (H, W), seeds, amp = CASES[cid]
    I0s, I1s = speckle_pairs(list(seeds), H, W)
    out = (np.ascontiguousarray(I0s), np.ascontiguousarray(I1s), np.stack([initial_flow(s, H, W, amp) for s in seeds]))
    for a in out:
        a.setflags(write=False)
    return out


def f32_frames(I0s, I1s, seed):
    """uint8 frames as float32 in [0, 1] with sub-level detail (tvl1_ref64_cases.solve_pairs' "f32" kind)."""
    rng = np.random.default_rng(seed)
    return tuple(((a.astype(np.float32) + rng.random(a.shape, dtype=np.float32)) / np.float32(256)) for a in (I0s, I1s))


# ---- the oracle's solve, composed of its exported stages ------------------------------------------------------------------------------
def _sizes(O, P, H, W):
    """(w, h) of the levels a solve uses, finest first: compute_levels' rule"""
    sizes = [(W, H)]
    for _ in range(1, P.nscales):
        w, h = O.scaled_size(sizes[-1][0], P.scale_step), O.scaled_size(sizes[-1][1], P.scale_step)
        if w < 16 or h < 16:
            break
        sizes.append((w, h))
    return sizes


def _levels(O, img, P, n):
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return [img.astype(np.float32)] + [O.pyramid_level(img, s, P.scale_step) for s in range(1, n)]
    lv = [img * np.float32(255.0)]                       # CV_32F frames: convertTo(CV_32F, 255)
    for s in range(1, n):
        h, w = lv[-1].shape
        lv.append(O.resize_linear(lv[-1], O.scaled_size(w, P.scale_step), O.scaled_size(h, P.scale_step), P.scale_step, P.scale_step))
    return lv


def _seed(O, init, sizes, step, seed_error):
    """the initial flow at the coarsest level of `sizes`"""
    u = [np.ascontiguousarray(init[..., k], dtype=np.float32) for k in (0, 1)]
    n = len(sizes)
    if seed_error == "direct" and n > 1:                 # one resize(flow, size of the coarsest level) instead of the chain: its scale
        w, h = sizes[-1]                                 # is the size ratio (with two levels this is "size_ratio")
        return [O.resize_linear(a, w, h) * np.float32(step ** (n - 1)) for a in u]
    gain = np.float32({"no_gain": 1.0, "gain_inverse": 1 / step}.get(seed_error, step))
    for (w, h) in sizes[1:]:
        if seed_error == "size_ratio":                   # resize(src, dsize): the upsample's rule, not the pyramid's
            u = [O.resize_linear(a, w, h) * gain for a in u]
        else:
            u = [O.resize_linear(a, w, h, step, step) * gain for a in u]
    return u


def composed(O, I0, I1, P, init=None, seed_error=None):
    """calc(I0, I1[, init]) -> (flow float32 [H, W, 2], iters int32 [levels used, warps, 2] finest level first, levels used).
    P: any object with the oracle's field names."""
    assert seed_error is None or seed_error in SEED_ERRORS
    H, W = np.shape(I0)
    sizes = _sizes(O, P, H, W)
    n = len(sizes)
    L0, L1 = _levels(O, I0, P, n), _levels(O, I1, P, n)
    iters = np.zeros((n, P.warps, 2), np.int32)
    if init is None:
        u1, u2 = (np.zeros(L0[-1].shape, np.float32) for _ in range(2))
    else:
        u1, u2 = _seed(O, np.asarray(init), sizes, P.scale_step, seed_error)
    for s in range(n - 1, -1, -1):
        w, h = sizes[s]
        assert L0[s].shape == (h, w)
        thr = float(np.float32(P.epsilon * P.epsilon * float(w * h)))
        p = [np.zeros((h, w), np.float32) for _ in range(4)]
        for wi in range(P.warps):
            wx, wy, grad, rho = O.warp(L0[s], L1[s], u1, u2)
            error, n_in, n_out = FLT_MAX, 0, 0
            while error > thr and n_out < P.outer_iterations:
                if P.median_filtering > 1:
                    u1, u2 = O.median_blur(u1, P.median_filtering), O.median_blur(u2, P.median_filtering)
                n_out += 1
                ni = 0
                while error > thr and ni < P.inner_iterations:
                    u1, u2, *p, q = O.iterate(wx, wy, grad, rho, u1, u2, *p, 1, P.lambda_, P.theta, P.tau)
                    error = float(int(q[0])) / 2.0 ** 30
                    ni += 1
                n_in += ni
            iters[s, wi] = n_in, n_out
        if s:
            w, h = sizes[s - 1]
            mul = np.float32(1 / P.scale_step)
            u1, u2 = O.resize_linear(u1, w, h) * mul, O.resize_linear(u2, w, h) * mul
    return np.stack([u1, u2], -1), iters, n


# ---- the same solve in float64 --------------------------------------------------------------------------------------------------------
def ref_init(I0, I1, P, init=None):
    """-> (flow float64 [H, W, 2], iters [levels used, warps, 2], min_margin) over tvl1_ref64's pyramid, _stage and resize_linear"""
    L0, L1 = R.pyramid(I0, P.nscales, P.scale_step), R.pyramid(I1, P.nscales, P.scale_step)
    margin = R._Margin()
    iters = np.zeros((len(L0), P.warps, 2), np.int64)
    if init is None:
        u = (np.zeros(L0[-1].shape), np.zeros(L0[-1].shape))
    else:
        u = tuple(np.asarray(init[..., k], np.float32).astype(np.float64) for k in (0, 1))
        for lv in L0[1:]:
            h, w = lv.shape
            u = tuple(R.resize_linear(a, w, h, P.scale_step, P.scale_step) * P.scale_step for a in u)
    for s in range(len(L0) - 1, -1, -1):
        p = tuple(np.zeros(L0[s].shape) for _ in range(4))
        for wi in range(P.warps):
            u, p, iters[s, wi] = R._stage(L0[s], L1[s], u, p, P, wi, margin, None)
        if s:
            h, w = L0[s - 1].shape
            u = tuple(R.resize_linear(a, w, h) * (1.0 / P.scale_step) for a in u)
    return np.stack(u, -1), iters, margin.least


@functools.lru_cache(maxsize=None)
def ref_case(cid, b):
    """The float64 result of pair b of a case; computed once per process and shared."""
    I0s, I1s, inits = case_inputs(cid)
    out = ref_init(I0s[b], I1s[b], K.params(**CASES[cid][0]), inits[b])
    out[0].setflags(write=False)
    return out


_composed = {}


def composed_case(O, cid, b):
    """composed's result of pair b of a case; computed once per process and shared."""
    if (cid, b) not in _composed:
        I0s, I1s, inits = case_inputs(cid)
        out = composed(O, I0s[b], I1s[b], K.params(**CASES[cid][0]), inits[b])
        out[0].setflags(write=False)
        _composed[cid, b] = out
    return _composed[cid, b]


def criterion(sid, flow, iters, levels, ref):
    """What a seeded solve must meet against the float64 one: -> a list of what it misses (empty: it passes).  Prints the figures."""
    rf, rit, margin = ref
    d = K.dev_flow(flow, rf)
    print(sid, f"margin={margin:.3g}", " ".join(f"{k}={v:.3g}" for k, v in d.items()))
    missed = []
    if margin < K.MIN_MARGIN:
        missed.append(f"a stop test of the reference is {margin:.3g} from its threshold: change the seed")
    if levels != rit.shape[0]:
        missed.append(f"pyramid depth {levels}, reference {rit.shape[0]}")
    elif not np.array_equal(iters, rit):
        missed.append(f"iteration counts {np.asarray(iters).tolist()}, reference {rit.tolist()}")
    if d["flow_mean_epe"] > K.EPE_MEAN:
        missed.append(f"mean EPE {d['flow_mean_epe']:.3g} > {K.EPE_MEAN}")
    if d["flow_frac_beyond"] > K.EPE_FRACTION:
        missed.append(f"{d['flow_frac_beyond']:.3g} of the pixels beyond {K.EPE_PX} px > {K.EPE_FRACTION}")
    return missed
