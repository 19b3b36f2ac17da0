"""A float64 reference of DualTVL1 (Zach-Pock-Bischof as OpenCV's tvl1flow.cpp arranges it), independent of oracle/tvl1_oracle.c.

Written from the algorithm (SURVEY.md Appendix A and the prose of the oracle's header), in whole-array numpy / scipy form, not from the
oracle's loops, and sharing no code with oracle/oracle.py:
  pyramid: level s is level s-1 resized by scale_step with INTER_LINEAR (half-pixel centres: src = (dst + 1/2) / f - 1/2, clamped to
    the image, so below 0 the first sample has all the weight and the far edge is replicated); sizes are rint(size * step), half to
    even; the pyramid ends before a level narrower or lower than 16 and before an empty one.  uint8 frames are taken as they are,
    float32 frames times 255.
  per level, coarsest first, from u = 0: the centred gradient of I1 (1/2 (next - prev), the missing neighbour replaced by the pixel, so
    the border gives 1/2 (a1 - a0)); the duals p = 0 once per level; then `warps` times:
      warp: I1, I1x, I1y sampled at (x + u1, y + u2) -- the positions are float32 sums (a CV_32F map) quantised to 1/32 px, half to
        even; 4 x 4 Keys cubic with a = -0.75, the fourth weight 1 - the others; taps outside the image are 0; the integer part
        saturates to int16 -- giving I1wx, I1wy, |grad|^2 = I1wx^2 + I1wy^2 and rho_c = I1w - I1wx u1 - I1wy u2 - I0;
      at most `outer` times, while error > epsilon^2 w h: median-filter u1 and u2 (replicated border), then at most `inner` times
      under the same guard one iteration:
        rho = rho_c + I1wx u1 + I1wy u2, l_t = lambda theta;
        v = u + l_t grad I1w            where rho < -l_t |grad|^2
            u - l_t grad I1w            where rho >  l_t |grad|^2
            u - rho grad I1w / |grad|^2 elsewhere, if |grad|^2 > FLT_EPSILON (else v = u);
        u' = v + theta div p, div p = (p1[x] - p1[x-1]) + (p2[y] - p2[y-1]), where the first column takes p1[x] and the first row
          p2[y] themselves;
        error = sum (u1' - u1)^2 + (u2' - u2)^2;
        grad u' by forward differences, 0 in the last column / row;  p = (p + taut grad u') / (1 + taut |grad u'|), taut = tau / theta,
          per flow component;
    the flow goes to the next finer level by INTER_LINEAR to that level's size (scale = the size ratio), times 1 / scale_step.
  variant 1 (what cv2.cuda.OpticalFlowDual_TVL1 runs): the resizes have no half-pixel shift (src = dst / f, far edge replicated); the
    warp is a Catmull-Rom (a = -0.5) cubic over the taps ceil(w - 2) .. floor(w + 2), clamp addressing, divided by the weight sum, no
    quantisation; no median; per warp one loop of inner * outer iterations in which the error is taken only on odd iterations, and
    only once `prevError` (the last error taken, less the threshold for every iteration that took none) is below the threshold.
Everything is float64 except where the algorithm itself says float32 (the sample positions).  `mutate=` names one deliberate error
(MUTATIONS) for the sensitivity test; nothing else may pass it.  Only tests use this module.
"""
import numpy as np
from scipy import ndimage

FLT_EPSILON = float(np.finfo(np.float32).eps)

MUTATIONS = ("div_first_row", "div_first_col", "taut_product", "lt_lambda_only", "threshold_sign", "median_after",
             "duals_reset_per_warp", "no_upsample_gain", "grad_border_full", "cubic_a_-0.5", "fwd_grad_wraps")


def _check(mutate):
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutate!r}")


# ---- resizing and the pyramid -------------------------------------------------------------------------------------------------------
def _linear_taps(n_dst, n_src, f, shift):
    """Per destination index: the two source indices and the weight of the second, for src = (dst + shift) / f - shift clamped to
    the image."""
    pos = np.clip((np.arange(n_dst) + shift) / f - shift, 0.0, n_src - 1.0)
    i0 = np.floor(pos).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_src - 1), pos - i0


def _resize(src, dw, dh, scale_x, scale_y, shift):
    src = np.asarray(src, np.float64)
    sh, sw = src.shape
    x0, x1, ax = _linear_taps(dw, sw, scale_x, shift)
    y0, y1, ay = _linear_taps(dh, sh, scale_y, shift)
    rows = src[:, x0] * (1 - ax) + src[:, x1] * ax
    return rows[y0] * (1 - ay)[:, None] + rows[y1] * ay[:, None]


def resize_linear(src, dw, dh, scale_x=None, scale_y=None):
    """cv::resize INTER_LINEAR to dw x dh; scale_* is the factor dst / src (default: the size ratio)."""
    sh, sw = np.shape(src)
    return _resize(src, dw, dh, scale_x or dw / sw, scale_y or dh / sh, 0.5)


def resize_cuda(src, dw, dh, scale_x=None, scale_y=None):
    """cv::cuda::resize INTER_LINEAR (variant 1): no half-pixel shift."""
    sh, sw = np.shape(src)
    return _resize(src, dw, dh, scale_x or dw / sw, scale_y or dh / sh, 0.0)


def scaled_size(n, step):
    return int(np.rint(n * step))


def pyramid(img, nscales, scale_step, variant=0):
    """The levels a solve uses, finest first."""
    img = np.asarray(img)
    lv = [img.astype(np.float64) * (255.0 if img.dtype == np.float32 else 1.0)]
    rs = resize_cuda if variant == 1 else resize_linear
    for _ in range(1, nscales):
        h, w = lv[-1].shape
        nw, nh = scaled_size(w, scale_step), scaled_size(h, scale_step)
        if nw < 16 or nh < 16:
            break
        lv.append(rs(lv[-1], nw, nh, scale_step, scale_step))
    return lv


def pyramid_level(img, level, scale_step, variant=0):
    """Level `level` of the pyramid without the size-16 rule (what the kernel-level hooks build)."""
    a = np.asarray(img, np.float64)
    rs = resize_cuda if variant == 1 else resize_linear
    for _ in range(level):
        h, w = a.shape
        a = rs(a, scaled_size(w, scale_step), scaled_size(h, scale_step), scale_step, scale_step)
    return a


# ---- the warp -----------------------------------------------------------------------------------------------------------------------
def centered_gradient(a, mutate=None):
    _check(mutate)
    a = np.asarray(a, np.float64)
    px = np.pad(a, ((0, 0), (1, 1)), mode="edge")
    py = np.pad(a, ((1, 1), (0, 0)), mode="edge")
    gx, gy = 0.5 * (px[:, 2:] - px[:, :-2]), 0.5 * (py[2:] - py[:-2])
    if mutate == "grad_border_full":
        gx[:, [0, -1]] *= 2
        gy[[0, -1]] *= 2
    return gx, gy


def keys(t, a):
    """The Keys cubic convolution kernel."""
    t = np.abs(t)
    return np.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1, np.where(t < 2, ((a * t - 5 * a) * t + 8 * a) * t - 4 * a, 0.0))


def _positions(shape, u, v):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return xx.astype(np.float32) + np.asarray(u, np.float32), yy.astype(np.float32) + np.asarray(v, np.float32)


def _gather(pad, ix, iy):
    """pad = the image inside one ring of whatever lies outside; indices beyond the ring read the ring."""
    h, w = pad.shape[0] - 2, pad.shape[1] - 2
    return pad[np.clip(iy, -1, h) + 1, np.clip(ix, -1, w) + 1]


def remap_bicubic(src, u, v, a=-0.75):
    """cv::remap INTER_CUBIC, BORDER_CONSTANT 0, with the float32 maps (x + u, y + v)."""
    src = np.asarray(src, np.float64)
    mx, my = _positions(src.shape, u, v)
    sx = np.rint(mx.astype(np.float64) * 32)
    sy = np.rint(my.astype(np.float64) * 32)
    fx, fy = np.mod(sx, 32) / 32.0, np.mod(sy, 32) / 32.0
    ix = np.clip(np.floor(sx / 32), -32768, 32767).astype(np.int64) - 1
    iy = np.clip(np.floor(sy / 32), -32768, 32767).astype(np.int64) - 1

    def weights(f):
        w = [keys(1 + f, a), keys(f, a), keys(1 - f, a)]
        return w + [1 - w[0] - w[1] - w[2]]
    pad = np.pad(src, 1)
    out = np.zeros(src.shape)
    for j, wy in enumerate(weights(fy)):
        for i, wx in enumerate(weights(fx)):
            out += wy * wx * _gather(pad, ix + i, iy + j)
    return out


def warp(I0, I1, u1, u2, mutate=None):
    """One warp of the CPU form -> I1wx, I1wy, rho_c."""
    _check(mutate)
    I1 = np.asarray(I1, np.float64)
    a = -0.5 if mutate == "cubic_a_-0.5" else -0.75
    gx, gy = centered_gradient(I1, mutate)
    Iw, wx, wy = (remap_bicubic(s, u1, u2, a) for s in (I1, gx, gy))
    u1, u2 = np.asarray(u1, np.float32).astype(np.float64), np.asarray(u2, np.float32).astype(np.float64)
    return wx, wy, Iw - wx * u1 - wy * u2 - np.asarray(I0, np.float64)


def warp_cuda(I0, I1, u1, u2, mutate=None):
    """One warp of variant 1 -> I1wx, I1wy, rho_c."""
    _check(mutate)
    I1 = np.asarray(I1, np.float64)
    h, w = I1.shape
    mx, my = (m.astype(np.float64) for m in _positions(I1.shape, u1, u2))
    bx, by = np.ceil(mx - 2), np.ceil(my - 2)
    srcs = (I1,) + centered_gradient(I1, mutate)
    acc = [np.zeros(I1.shape) for _ in srcs]
    wsum = np.zeros(I1.shape)
    for j in range(5):                      # a fifth tap exists only at integer positions; the kernel is 0 at distance 2
        for i in range(5):
            cx, cy = bx + i, by + j
            wt = keys(mx - cx, -0.5) * keys(my - cy, -0.5)
            ys, xs = np.clip(cy, 0, h - 1).astype(np.int64), np.clip(cx, 0, w - 1).astype(np.int64)
            for k, s in enumerate(srcs):
                acc[k] += wt * s[ys, xs]
            wsum += wt
    Iw, wx, wy = (s / wsum for s in acc)
    u1, u2 = np.asarray(u1, np.float32).astype(np.float64), np.asarray(u2, np.float32).astype(np.float64)
    return wx, wy, Iw - wx * u1 - wy * u2 - np.asarray(I0, np.float64)


# ---- the iteration ------------------------------------------------------------------------------------------------------------------
def _div(p1, p2, mutate):
    d1, d2 = p1.copy(), p2.copy()
    d1[:, 1:] -= p1[:, :-1]
    d2[1:] -= p2[:-1]
    # The two border mutations: the interior form a[i] - a[i-1] at the border.  Reading the outside as 0 there IS the right form
    # (a[0] - 0), so the neighbour that does not exist is read as the border value, as an unguarded index would: the term drops out.
    if mutate == "div_first_col":
        d1[:, 0] = 0
    if mutate == "div_first_row":
        d2[0] = 0
    return d1 + d2


def _fwd(u, mutate):
    ux, uy = np.zeros_like(u), np.zeros_like(u)
    ux[:, :-1] = u[:, 1:] - u[:, :-1]
    uy[:-1] = u[1:] - u[:-1]
    if mutate == "fwd_grad_wraps":
        if u.shape[1] > 1:
            ux[:, -1] = u[:, -1] - u[:, -2]
        if u.shape[0] > 1:
            uy[-1] = u[-1] - u[-2]
    return ux, uy


def _step(wx, wy, grad, rho_c, u, p, lam, theta, tau, mutate):
    """One iteration: u = (u1, u2), p = (p11, p12, p21, p22) -> the new u, the new p, the error sum."""
    lt = lam if mutate == "lt_lambda_only" else lam * theta
    taut = tau * theta if mutate == "taut_product" else tau / theta
    rho = rho_c + wx * u[0] + wy * u[1]
    below, above = rho < -lt * grad, rho > lt * grad
    if mutate == "threshold_sign":
        below, above = above, below
    with np.errstate(divide="ignore", invalid="ignore"):
        mid = np.where(grad > FLT_EPSILON, -rho / grad, 0.0)
    step = np.where(below, lt, np.where(above, -lt, mid))
    v = (u[0] + step * wx, u[1] + step * wy)
    un = (v[0] + theta * _div(p[0], p[1], mutate), v[1] + theta * _div(p[2], p[3], mutate))
    err = float(((un[0] - u[0]) ** 2 + (un[1] - u[1]) ** 2).sum())
    pn = []
    for k in (0, 1):
        ux, uy = _fwd(un[k], mutate)
        ng = 1 + taut * np.hypot(ux, uy)
        pn += [(p[2 * k] + taut * ux) / ng, (p[2 * k + 1] + taut * uy) / ng]
    return un, tuple(pn), err


def iterate(wx, wy, rho_c, u1, u2, p11, p12, p21, p22, n, lam=0.15, theta=0.3, tau=0.25, mutate=None):
    """n iterations without a stop test -> (u1, u2, p11, p12, p21, p22, the n error sums)."""
    _check(mutate)
    wx, wy, rho_c = (np.asarray(a, np.float64) for a in (wx, wy, rho_c))
    u = tuple(np.asarray(a, np.float64) for a in (u1, u2))
    p = tuple(np.asarray(a, np.float64) for a in (p11, p12, p21, p22))
    grad = wx * wx + wy * wy
    errs = np.zeros(n)
    for k in range(n):
        u, p, errs[k] = _step(wx, wy, grad, rho_c, u, p, lam, theta, tau, mutate)
    return (*u, *p, errs)


def median(a, k):
    return a if k <= 1 else ndimage.median_filter(a, size=k, mode="nearest")


# ---- the solve ----------------------------------------------------------------------------------------------------------------------
class _Margin:
    """The smallest |error / threshold - 1| over the stop tests a solve evaluates."""

    def __init__(self):
        self.least = np.inf

    def above(self, error, thr):
        if np.isfinite(error) and thr > 0:
            self.least = min(self.least, abs(error / thr - 1))
        return error > thr


def _stage(I0, I1, u, p, P, wi, margin, mutate):
    """One warp of the CPU form and its outer / inner loops -> u, p, (inner, outer) iterations executed."""
    lam, theta, tau = P.lambda_, P.theta, P.tau
    thr = P.epsilon * P.epsilon * I0.size
    wx, wy, rho_c = warp(I0, I1, u[0], u[1], mutate)
    grad = wx * wx + wy * wy
    error, n_in, n_out = np.inf, 0, 0
    for _ in range(P.outer_iterations):
        if not margin.above(error, thr):
            break
        if mutate != "median_after":
            u = tuple(median(a, P.median_filtering) for a in u)
        n_out += 1
        for _ in range(P.inner_iterations):
            if not margin.above(error, thr):
                break
            u, p, error = _step(wx, wy, grad, rho_c, u, p, lam, theta, tau, mutate)
            n_in += 1
        if mutate == "median_after":
            u = tuple(median(a, P.median_filtering) for a in u)
    return u, p, (n_in, n_out)


def _stage_cuda(I0, I1, u, p, P, wi, margin, mutate):
    """One warp of variant 1 and its single loop."""
    thr = P.epsilon * P.epsilon * I0.size
    wx, wy, rho_c = warp_cuda(I0, I1, u[0], u[1], mutate)
    grad = wx * wx + wy * wy
    error, prev, n = np.inf, 0.0, 0
    while margin.above(error, thr) and n < P.inner_iterations * P.outer_iterations:
        take = P.epsilon > 0 and n % 2 == 1 and not margin.above(prev, thr) and prev != thr
        u, p, e = _step(wx, wy, grad, rho_c, u, p, P.lambda_, P.theta, P.tau, mutate)
        if take:
            error = prev = e
        else:
            error, prev = np.inf, prev - thr
        n += 1
    return u, p, (n, 0)


def solve(I0, I1, params, mutate=None):
    """calc(I0, I1) -> (flow float64 [H, W, 2], iters int [levels used, warps, 2] finest level first, min_margin).
    `params`: any object with the oracle's field names (lambda_, theta, tau, epsilon, scale_step, nscales, warps, inner_iterations,
    outer_iterations, median_filtering, variant)."""
    _check(mutate)
    P = params
    variant = getattr(P, "variant", 0)
    L0, L1 = pyramid(I0, P.nscales, P.scale_step, variant), pyramid(I1, P.nscales, P.scale_step, variant)
    stage = _stage_cuda if variant == 1 else _stage
    margin = _Margin()
    iters = np.zeros((len(L0), P.warps, 2), np.int64)
    u = (np.zeros(L0[-1].shape), np.zeros(L0[-1].shape))
    for s in range(len(L0) - 1, -1, -1):
        p = tuple(np.zeros(L0[s].shape) for _ in range(4))
        for wi in range(P.warps):
            if mutate == "duals_reset_per_warp":
                p = tuple(np.zeros(L0[s].shape) for _ in range(4))
            u, p, iters[s, wi] = stage(L0[s], L1[s], u, p, P, wi, margin, mutate)
        if s:
            h, w = L0[s - 1].shape
            gain = 1.0 if mutate == "no_upsample_gain" else 1.0 / P.scale_step
            u = tuple((resize_cuda if variant == 1 else resize_linear)(a, w, h) * gain for a in u)
    return np.stack(u, -1), iters, margin.least
