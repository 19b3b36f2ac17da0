"""A float64 reference of DeepFlow -- one VariationalRefinement::calcUV, and the solve around it -- independent of oracle/deepflow_oracle.c.

Written from the algorithm the oracle's header states, in whole-array numpy / scipy form, not from its loops:
  warp I1 by W (bilinear on float32 maps quantised to 1/32 px, zero outside the image); Iavg = (I0 + Iw) / 2, Iz = Iw - I0;
  [-1 0 1] derivatives with a replicated border: Ix, Iy of Iavg, Ixx, Ixy of Ix, Iyy of Iy, Ixz, Iyz of Iz;
  per fixed-point iteration, from the current increment dW:
    robust data term: colour constancy (weight delta/2) and gradient constancy (weight gamma/2), each normalised by its
      derivative norm + zeta^2, with eps in the robust function -> a diagonal 2x2 block and a right-hand side per pixel;
    smoothness weight (alpha/2) / sqrt(|grad(W + dW)|^2 + eps^2) per pixel from forward differences (0 across the border);
    every in-image edge (p, q), q to the right of or below p, couples dW(p) and dW(q) with the weight of p and adds
      +/- w (W(q) - W(p)) to their right-hand sides;
    then either `sor` red-black SOR sweeps (red = (x + y) even first; u then v per pixel, v sees the new u) started from the
    current dW, or the exact solution of the same sparse system.
The result is W + dW in float64.

And of the solve around it (OpticalFlowDeepFlow::calc), from the same header:
  frames to floating point without a factor: uint8 frames keep 0..255, float32 frames are taken as they are;
  a 3 x 3 Gaussian blur: taps exp(-x^2 / (2 sigma^2)), x = -1, 0, 1, of the float32 sigma, normalised in double and THEN rounded to
    float32 (that rounding is part of the specification); row pass, column pass; BORDER_REFLECT_101 (the neighbour beyond the edge is the
    pixel one inside it; a side of length 1 reflects onto itself);
  level sizes: size' = (int)(size * factor + 0.5f) in float32 arithmetic, per side, while both new sides are > min_size, at most 201
    levels; level l is level l - 1 resized to that size with INTER_LINEAR (half-pixel centres, the scale is the size ratio);
  the flow starts at zero on the coarsest level; every level is refined (calcUV with alpha 4 alpha, delta / 3, gamma / 3); the refined
    flow goes to the next finer level by INTER_LINEAR to that level's size, times float32(1) / float32(factor).
Everything is float64 except where the algorithm itself says float32 (the taps, the size rule, the gain, the warp's sample positions).
`mutate=` names one deliberate error (MUTATIONS) for the sensitivity test; nothing else may pass it.  Only tests use this module.
"""
import numpy as np
from scipy import sparse
from scipy.sparse import linalg as splinalg

from tests.tvl1_ref64 import resize_cuda, resize_linear      # written from cv::resize's definition, independent of both oracles

MAX_LEVELS = 201

MUTATIONS = ("no_blur", "sigma_plus_0.05", "border_reflect", "sizes_truncated", "sizes_float64", "resize_no_half_pixel", "no_gain",
             "gain_is_factor", "nonzero_start", "level0_not_refined")


def _check(mutate):
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutate!r}")


def warp_bilinear(I1, u, v):
    """cv::remap INTER_LINEAR with float32 maps (x + u, y + v), 1/32-px fixed point, BORDER_CONSTANT 0."""
    h, w = I1.shape
    yy, xx = np.mgrid[0:h, 0:w]
    mx = xx.astype(np.float32) + np.asarray(u, np.float32)       # the maps are CV_32F: the sum is rounded to float32
    my = yy.astype(np.float32) + np.asarray(v, np.float32)
    sx = np.rint(mx.astype(np.float64) * 32).astype(np.int64)   # x 32 is exact; round half to even
    sy = np.rint(my.astype(np.float64) * 32).astype(np.int64)
    fx, fy = (sx & 31) / 32.0, (sy & 31) / 32.0
    ix, iy = sx >> 5, sy >> 5
    pad = np.zeros((h + 2, w + 2))                               # one ring of zeros is all a tap just outside can see
    pad[1:-1, 1:-1] = I1
    out = np.zeros((h, w))
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            px, py = ix + dx, iy + dy
            inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            val = np.where(inside, pad[np.clip(py, -1, h) + 1, np.clip(px, -1, w) + 1], 0.0)
            out += wy * wx * val
    return out


def dx(a):
    p = np.pad(a, ((0, 0), (1, 1)), mode="edge")
    return p[:, 2:] - p[:, :-2]


def dy(a):
    p = np.pad(a, ((1, 1), (0, 0)), mode="edge")
    return p[2:] - p[:-2]


def derivatives(I0, I1, u, v):
    Iw = warp_bilinear(np.asarray(I1, np.float64), u, v)
    I0 = np.asarray(I0, np.float64)
    avg, Iz = (I0 + Iw) / 2, Iw - I0
    Ix, Iy = dx(avg), dy(avg)
    return dict(Ix=Ix, Iy=Iy, Iz=Iz, Ixx=dx(Ix), Ixy=dy(Ix), Iyy=dy(Iy), Ixz=dx(Iz), Iyz=dy(Iz))


def data_term(D, du, dv, delta, gamma, zeta, eps):
    """Per-pixel 2x2 block (a11, a12, a22) and right-hand side (b1, b2) of the robust data term, linearised at dW."""
    Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz = (D[k] for k in ("Ix", "Iy", "Iz", "Ixx", "Ixy", "Iyy", "Ixz", "Iyz"))
    z2, e2 = zeta * zeta, eps * eps
    n0 = Ix * Ix + Iy * Iy + z2
    r0 = Iz + Ix * du + Iy * dv
    c = (delta / 2) / np.sqrt(r0 * r0 / n0 + e2) / n0
    a11, a12, a22 = c * Ix * Ix + z2, c * Ix * Iy, c * Iy * Iy + z2
    b1, b2 = -c * Iz * Ix, -c * Iz * Iy
    n1, n2 = Ixx * Ixx + Ixy * Ixy + z2, Iyy * Iyy + Ixy * Ixy + z2
    rx, ry = Ixz + Ixx * du + Ixy * dv, Iyz + Ixy * du + Iyy * dv
    g = (gamma / 2) / np.sqrt(rx * rx / n1 + ry * ry / n2 + e2)
    a11 = a11 + g * (Ixx * Ixx / n1 + Ixy * Ixy / n2)
    a12 = a12 + g * (Ixx * Ixy / n1 + Ixy * Iyy / n2)
    a22 = a22 + g * (Ixy * Ixy / n1 + Iyy * Iyy / n2)
    b1 = b1 - g * (Ixx * Ixz / n1 + Ixy * Iyz / n2)
    b2 = b2 - g * (Ixy * Ixz / n1 + Iyy * Iyz / n2)
    return a11, a12, a22, b1, b2


def smoothness_weight(U, V, alpha, eps):
    """(alpha/2) / sqrt(ux^2 + vx^2 + uy^2 + vy^2 + eps^2) with forward differences, 0 at the last column / row."""
    ux, vx, uy, vy = (np.zeros_like(U) for _ in range(4))
    ux[:, :-1], vx[:, :-1] = U[:, 1:] - U[:, :-1], V[:, 1:] - V[:, :-1]
    uy[:-1], vy[:-1] = U[1:] - U[:-1], V[1:] - V[:-1]
    return (alpha / 2) / np.sqrt(ux * ux + vx * vx + uy * uy + vy * vy + eps * eps)


def edges(h, w, wg):
    """Every in-image edge as (index p, index q, weight of p), q to the right of or below p."""
    idx = np.arange(h * w).reshape(h, w)
    p = np.concatenate([idx[:, :-1].ravel(), idx[:-1].ravel()])
    q = np.concatenate([idx[:, 1:].ravel(), idx[1:].ravel()])
    return p, q, wg.ravel()[p]


def assemble(a11, a12, a22, b1, b2, wg, Wu, Wv):
    """The full system: the data blocks, the edge terms on the diagonals, -w off the diagonal, w (W(q) - W(p)) on the right."""
    h, w = wg.shape
    n = h * w
    p, q, we = edges(h, w, wg)
    deg = np.bincount(p, we, n) + np.bincount(q, we, n)
    Wuf, Wvf = Wu.ravel(), Wv.ravel()
    r1 = b1.ravel() + np.bincount(p, we * (Wuf[q] - Wuf[p]), n) - np.bincount(q, we * (Wuf[q] - Wuf[p]), n)
    r2 = b2.ravel() + np.bincount(p, we * (Wvf[q] - Wvf[p]), n) - np.bincount(q, we * (Wvf[q] - Wvf[p]), n)
    return a11.ravel() + deg, a12.ravel(), a22.ravel() + deg, r1, r2, (p, q, we)


def sor_sweeps(A11, A12, A22, r1, r2, E, du, dv, shape, sweeps, omega):
    """Red-black SOR on the assembled system, red ((x + y) even) first; in a colour u then v, v with the new u."""
    h, w = shape
    n = h * w
    p, q, we = E
    yy, xx = np.mgrid[0:h, 0:w]
    colours = [np.flatnonzero(((xx + yy) & 1).ravel() == c) for c in (0, 1)]
    du, dv = du.ravel().copy(), dv.ravel().copy()

    def nsum(a, m):      # sum over the neighbours of the pixels in m of w * a(neighbour)
        s = np.bincount(p, we * a[q], n) + np.bincount(q, we * a[p], n)
        return s[m]

    for _ in range(sweeps):
        for m in colours:
            su, sv = nsum(du, m), nsum(dv, m)
            du[m] += omega * ((su + r1[m] - dv[m] * A12[m]) / A11[m] - du[m])
            dv[m] += omega * ((sv + r2[m] - du[m] * A12[m]) / A22[m] - dv[m])
    return du.reshape(h, w), dv.reshape(h, w)


def exact_solve(A11, A12, A22, r1, r2, E, shape):
    h, w = shape
    n = h * w
    p, q, we = E
    L = sparse.coo_matrix((np.concatenate([-we, -we]), (np.concatenate([p, q]), np.concatenate([q, p]))), shape=(n, n))
    M = sparse.bmat([[sparse.diags(A11) + L, sparse.diags(A12)], [sparse.diags(A12), sparse.diags(A22) + L]], format="csc")
    x = splinalg.spsolve(M, np.concatenate([r1, r2]))
    return x[:n].reshape(h, w), x[n:].reshape(h, w)


def refine(I0, I1, u, v, alpha, delta, gamma, zeta, epsilon, fixed_point_iterations, sor_iterations, omega, exact=False):
    """VariationalRefinement::calcUV in float64: returns (u + du, v + dv).  alpha, delta, gamma are the refinement's own
    (OpticalFlowDeepFlow passes 4 alpha, delta / 3, gamma / 3); `exact` replaces the SOR sweeps by a sparse direct solve."""
    Wu, Wv = np.asarray(u, np.float64), np.asarray(v, np.float64)
    D = derivatives(I0, I1, u, v)
    du, dv = np.zeros_like(Wu), np.zeros_like(Wv)
    for _ in range(fixed_point_iterations):
        a11, a12, a22, b1, b2 = data_term(D, du, dv, delta, gamma, zeta, epsilon)
        wg = smoothness_weight(Wu + du, Wv + dv, alpha, epsilon)
        A11, A12, A22, r1, r2, E = assemble(a11, a12, a22, b1, b2, wg, Wu, Wv)
        if exact:
            du, dv = exact_solve(A11, A12, A22, r1, r2, E, Wu.shape)
        else:
            du, dv = sor_sweeps(A11, A12, A22, r1, r2, E, du, dv, Wu.shape, sor_iterations, omega)
    return Wu + du, Wv + dv


def refine_params(I0, I1, u, v, params, exact=False):
    """refine() with the constants OpticalFlowDeepFlow derives from its parameters (a DfoParams / TfDeepflowParams-like object)."""
    f = np.float32
    return refine(I0, I1, u, v, alpha=float(f(4) * f(params.alpha)), delta=float(f(params.delta) / f(3)),
                  gamma=float(f(params.gamma) / f(3)), zeta=float(f(params.zeta)), epsilon=float(f(params.epsilon)),
                  fixed_point_iterations=params.fixed_point_iterations, sor_iterations=params.sor_iterations,
                  omega=float(f(params.omega)), exact=exact)


# ---- the solve around the refinement ------------------------------------------------------------------------------------------------
def gauss3(sigma, mutate=None):
    """getGaussianKernel(3, sigma, CV_32F) -> (centre, side) as the float32 values they are rounded to."""
    _check(mutate)
    s = float(np.float32(sigma)) + (0.05 if mutate == "sigma_plus_0.05" else 0.0)
    side = np.exp(-1.0 / (2.0 * s * s))
    total = 1.0 + 2.0 * side
    return float(np.float32(1.0 / total)), float(np.float32(side / total))


def _pad1(a, axis, mutate):
    """One more sample at each end of an axis: REFLECT_101 (cv2) is numpy's 'reflect'; cv2's REFLECT is numpy's 'symmetric'."""
    width = [(0, 0), (0, 0)]
    width[axis] = (1, 1)
    if a.shape[axis] == 1:
        return np.pad(a, width, mode="edge")
    return np.pad(a, width, mode="symmetric" if mutate == "border_reflect" else "reflect")


def blur3(img, sigma, mutate=None):
    """GaussianBlur(img, (3, 3), sigma), BORDER_REFLECT_101."""
    _check(mutate)
    a = np.asarray(img, np.float64)
    if mutate == "no_blur":
        return a.copy()
    k0, k1 = gauss3(sigma, mutate)
    p = _pad1(a, 1, mutate)
    a = k0 * p[:, 1:-1] + k1 * (p[:, :-2] + p[:, 2:])
    p = _pad1(a, 0, mutate)
    return k0 * p[1:-1] + k1 * (p[:-2] + p[2:])


def _next_size(n, factor, mutate):
    if mutate == "sizes_float64":
        return int(n * float(np.float32(factor)) + 0.5)
    f = np.float32
    if mutate == "sizes_truncated":
        return int(f(n) * f(factor))
    return int(f(f(n) * f(factor)) + f(0.5))                      # float32 product, float32 sum, truncation


def pyramid_sizes(W, H, params, mutate=None):
    """[(w, h)] of every level, finest first."""
    _check(mutate)
    sizes = [(int(W), int(H))]
    while len(sizes) < MAX_LEVELS:
        w, h = sizes[-1]
        nw, nh = _next_size(w, params.downscale_factor, mutate), _next_size(h, params.downscale_factor, mutate)
        if nw <= params.min_size or nh <= params.min_size:
            break
        sizes.append((nw, nh))
    return sizes


def _resize(a, w, h, mutate):
    return (resize_cuda if mutate == "resize_no_half_pixel" else resize_linear)(a, w, h)


def pyramid(img, params, mutate=None):
    """The levels of one frame, finest first: the blurred frame, then each level resized from the one before."""
    _check(mutate)
    lv = [blur3(img, params.sigma, mutate)]
    for w, h in pyramid_sizes(lv[0].shape[1], lv[0].shape[0], params, mutate)[1:]:
        lv.append(_resize(lv[-1], w, h, mutate))
    return lv


def upsample(u, v, dw, dh, factor, mutate=None):
    """The flow handed down to the next finer level, of dw x dh."""
    _check(mutate)
    gain = float(np.float32(1) / np.float32(factor))
    if mutate == "no_gain":
        gain = 1.0
    if mutate == "gain_is_factor":
        gain = float(np.float32(factor))
    return _resize(u, dw, dh, mutate) * gain, _resize(v, dw, dh, mutate) * gain


def solve(I0, I1, params, mutate=None):
    """OpticalFlowDeepFlow::calc -> (flow float64 [H, W, 2], levels).  `params`: any object with the oracle's field names."""
    _check(mutate)
    P0, P1 = pyramid(I0, params, mutate), pyramid(I1, params, mutate)
    start = 0.5 if mutate == "nonzero_start" else 0.0
    u, v = np.full(P0[-1].shape, start), np.full(P0[-1].shape, start)
    for l in range(len(P0) - 1, -1, -1):
        if not (l == 0 and mutate == "level0_not_refined"):
            u, v = refine_params(P0[l], P1[l], u, v, params)
        if l:
            h, w = P0[l - 1].shape
            u, v = upsample(u, v, w, h, params.downscale_factor, mutate)
    return np.stack([u, v], -1), len(P0)
