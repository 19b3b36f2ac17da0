"""One (level, warp) stage of DualTVL1 without its warp: the reference, the batches and the strip layouts that tests/test_tvl1_stage_cpu.py
(the reference against the oracle's whole solve, the batches' coverage) and tests/test_gpu_tvl1_stage.py (tf_dbg_stage against the
reference) share.  A helper module: nothing here is collected.

`stage_ref` is the loop of tests/tvl1_init_cases.py::composed over the oracle's median_blur and iterate, one iteration at a time, with
the exact uint64 error sums kept; for TF_VARIANT_CUDA the stop rule is restated from oracle/tvl1_oracle.c (proc_one_scale, variant 1).
The kernels read `variant` only in their stop rule, so the oracle's `iterate` is the arithmetic of both.

A batch's threshold is chosen from the reference's own sums (`pick_thr`): a float32 value that no sum of the batch comes close to, so
that no comparison of a test sits near a rounding boundary, and at which the pairs stop where the case needs them to."""
import ctypes as C
import functools

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)
PLANES = ("u1", "u2", "p11", "p12", "p21", "p22")
THR_MARGIN = 1e-4            # no error sum of a batch within this (relative) of its threshold


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def stage_ref(O, wx, wy, rho, state, inner, outer, ksize, thr, variant, pzero):
    """One stage for one pair -> (state: six float32 planes, err: uint64 [inner * outer], n_it, n_out).  thr: the stage's threshold
    (a float32 value for the CPU class; thr < 0: the pair never stops).  err[n] is the exact sum of iteration n for n < n_it, 0 after."""
    total = inner * outer
    grad = wx * wx + wy * wy
    u = [np.array(a, np.float32) for a in state[:2]]
    p = [np.zeros_like(u[0]) if pzero else np.array(a, np.float32) for a in state[2:]]
    err = np.zeros(total, np.uint64)

    def step(n):
        nonlocal u, p
        *s, q = O.iterate(wx, wy, grad, rho, *u, *p, 1)
        u, p = s[:2], s[2:]
        err[n] = q[0]
        return float(int(q[0])) / 2.0 ** 30

    n_it = n_out = 0
    if variant == 1:                                    # one loop; the sum is looked at on odd n, once prev has dropped below thr
        error, prev = DBL_MAX, 0.0
        while error > thr and n_it < total:
            calc = thr > 0 and (n_it & 1) and prev < thr
            e = step(n_it)
            if calc:
                error = prev = e
            else:
                error, prev = DBL_MAX, prev - thr
            n_it += 1
    else:
        error = FLT_MAX
        while error > thr and n_out < outer:
            if ksize > 1:
                u = [O.median_blur(a, ksize) for a in u]
            n_out += 1
            ni = 0
            while error > thr and ni < inner:
                error = step(n_it + ni)
                ni += 1
            n_it += ni
    return [*u, *p], err, n_it, n_out


def stops(E, thr, variant, inner):
    """(n_it, n_out) of a pair whose never-stopping run has the error sums E (uint64 [total]), by stage_ref's rules.  Until a pair
    stops, its run is the never-stopping one, so this is what stage_ref(thr) gives."""
    total = len(E)
    e = [float(int(q)) / 2.0 ** 30 for q in E]
    if variant == 1:
        error, prev, n = DBL_MAX, 0.0, 0
        while error > thr and n < total:
            if thr > 0 and (n & 1) and prev < thr:
                error = prev = e[n]
            else:
                error, prev = DBL_MAX, prev - thr
            n += 1
        return n, 0
    n = next((j + 1 for j in range(total) if not e[j] > thr), total)
    return n, (n - 1) // inner + 1


def mode_history(n_it, total, step, variant):
    """The pair's mode at every tvl1_iter launch of the stage, from the reference's n_it: N(ORMAL), R(EPLAY), E(XIT)."""
    out = []
    for it in range(0, total + step - 1, step):
        if it < n_it:
            out.append("N")
        elif step == 2 and variant == 0 and n_it % 2 == 1 and it == n_it + 1:
            out.append("R")
        else:
            out.append("E")
    return "".join(out)


def pick_thr(E, variant, inner, ok):
    """A float32 threshold between two neighbouring sums of E (uint64 [B, total]) at which ok(n_it of every pair) holds; of those, the
    one with the most different n_it.  No sum of E is within THR_MARGIN of it."""
    vals = np.unique(E.astype(np.float64)) / 2.0 ** 30
    best = None
    for lo, hi in zip(vals[:-1], vals[1:]):
        if lo <= 0 or hi / lo < 1 + 4 * THR_MARGIN:
            continue
        thr = float(np.float32(np.sqrt(lo * hi)))
        if not (lo * (1 + THR_MARGIN) < thr < hi * (1 - THR_MARGIN)):
            continue
        n = np.array([stops(e, thr, variant, inner)[0] for e in E])
        if ok(n) and (best is None or len(set(n)) > best[0]):
            best = (len(set(n)), thr)
    assert best is not None, "no threshold gives the batch the stops it needs"
    return best[1]


# ---- planes ----------------------------------------------------------------------------------------------------------------------------
def pair_planes(O, seed, h, w, amp, tiny=False):
    """(wx, wy, rho, [u1, u2, p11, p12, p21, p22]) of one pair, made as test_gpu_kernels._iterate_case makes them: smoothed frames
    through the oracle's warp, a patch with grad <= FLT_EPSILON.  The second frame differs from the first by `amp` of an unrelated
    frame, and the flow and the dual variable are `amp` of a unit field: the error sums of a stage scale with about amp^2.
    tiny: rows of +0 and of -0 in every plane and a band of columns in the denormal range."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    I0 = ndimage.gaussian_filter(rng.uniform(0, 255, (h, w)), 1.5).astype(np.float32)
    J = ndimage.gaussian_filter(rng.uniform(0, 255, (h, w)), 1.5).astype(np.float32)
    a = np.float32(amp)
    I1 = I0 + a * (J - I0)
    u = [rng.uniform(-1, 1, (h, w)).astype(np.float32) * a for _ in range(2)]
    p = [rng.uniform(-0.5, 0.5, (h, w)).astype(np.float32) * a for _ in range(4)]
    wx, wy, _, rho = O.warp(I0, I1, *u)
    wx[3:6, 3:9] = 0.0
    wy[3:6, 3:9] = 0.0
    if tiny:
        c0, c1 = w // 2, w // 2 + 8
        for arr, sc in [(wx, 1e-20), (wy, 1e-20), (rho, 1e-40)] + [(x, 1e-40) for x in (*u, *p)]:
            arr[:, c0:c1] = (arr[:, c0:c1].astype(np.float64) * sc / max(amp, 1e-3)).astype(np.float32)
            arr[h // 4:h // 4 + 3, :] = 0.0
            arr[h // 2:h // 2 + 2, :] = -0.0
    return wx, wy, rho, [*u, *p]


class Batch:
    """A batch of a case: planes [B, h, w] (read-only), the stage's parameters, and the reference of every pair."""
    def __init__(self, name, planes, inner, outer, ksize, thr, variant, pzero, ref):
        self.name, self.inner, self.outer, self.ksize, self.thr, self.variant, self.pzero = name, inner, outer, ksize, thr, variant, pzero
        self.wx, self.wy, self.rho, self.state = planes
        self.ref_state, self.ref_err, self.n_it, self.n_out = ref
        self.B, self.h, self.w = self.wx.shape
        self.total = inner * outer
        for a in (self.wx, self.wy, self.rho, *self.state, *self.ref_state, self.ref_err, self.n_it, self.n_out):
            a.setflags(write=False)

    def subset(self, idx):
        """the pairs `idx` of the batch as a batch of their own (a pair's stage does not depend on the batch it is in)"""
        ref = ([s[idx] for s in self.ref_state], self.ref_err[idx], self.n_it[idx], self.n_out[idx])
        return Batch(f"{self.name}-{len(idx)}", _take((self.wx, self.wy, self.rho, self.state), idx), self.inner, self.outer, self.ksize,
                     self.thr, self.variant, self.pzero, ref)

    def histogram(self):
        v, c = np.unique(self.n_it, return_counts=True)
        return {int(a): int(b) for a, b in zip(v, c)}


def _stack(pairs):
    wx, wy, rho = (np.stack([q[k] for q in pairs]) for k in range(3))
    state = [np.stack([q[3][k] for q in pairs]) for k in range(6)]
    return wx, wy, rho, state


def _take(planes, idx):
    wx, wy, rho, state = planes
    return wx[idx].copy(), wy[idx].copy(), rho[idx].copy(), [s[idx].copy() for s in state]


def _run_all(O, planes, inner, outer, ksize, thr, variant, pzero):
    wx, wy, rho, state = planes
    B = wx.shape[0]
    out = [stage_ref(O, wx[b], wy[b], rho[b], [s[b] for s in state], inner, outer, ksize, thr, variant, pzero) for b in range(B)]
    ref_state = [np.stack([o[0][k] for o in out]) for k in range(6)]
    return ref_state, np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.int32)


TINY70 = (7, 33, 58)         # pairs of the 70 (before the permutation) with +0 / -0 rows and a denormal band


@functools.lru_cache(maxsize=None)
def _planes70(O):
    h, w = 97, 131
    amps = np.logspace(-2.6, 0.4, 70)                    # three decades of amplitude: six of error
    return _stack([pair_planes(O, 500 + b, h, w, float(amps[b]), tiny=b in TINY70) for b in range(70)])


@functools.lru_cache(maxsize=None)
def _never70(O, ksize):
    """error sums [70, 12] of the 70 pairs when none ever stops (inner 4, outer 3)"""
    return _run_all(O, _planes70(O), 4, 3, ksize, -1.0, 0, 0)[1]


def _place(n_it, total, early_at, never_at):
    """A permutation of the batch: pairs that have stopped by iteration 2 at `early_at`, pairs that never stop at `never_at`, the
    others shuffled (the planes are made in order of amplitude)."""
    B = len(n_it)
    early = [b for b in range(B) if n_it[b] <= 2][:len(early_at)]
    never = [b for b in range(B) if n_it[b] == total][:len(never_at)]
    assert len(early) == len(early_at) and len(never) == len(never_at), "too few pairs that stop at once / never"
    fixed = dict(zip(early_at, early)) | dict(zip(never_at, never))
    rest = iter(np.random.default_rng(5).permutation([b for b in range(B) if b not in fixed.values()]))
    return np.array([fixed[i] if i in fixed else next(rest) for i in range(B)])


def mixed70_ok(n, inner=4, total=12):
    """what `mixed70` needs of its pairs' n_it (before they are placed)"""
    n = np.asarray(n)
    return bool((n == 1).any() and ((n % 2 == 1) & (n > 1)).any() and ((n % 2 == 0) & (n < total)).any() and (n == inner).any() and
                (n == inner + 1).any() and (n <= 2).sum() >= 4 and (n == total).sum() >= 2)


def cuda70_ok(n, total=12):
    n = np.asarray(n)
    return bool((n == 2).sum() >= 4 and ((n == 4) | (n == 6)).any() and (n == total).sum() >= 2)


@functools.lru_cache(maxsize=None)
def mixed70(O, ksize):
    """B = 70 pairs of 97 x 131, inner 4, outer 3, the CPU class's stop rule, medianFiltering `ksize` (0, 3, 5), p read from memory."""
    E = _never70(O, ksize)
    thr = pick_thr(E, 0, 4, mixed70_ok)
    n = np.array([stops(e, thr, 0, 4)[0] for e in E])
    planes = _take(_planes70(O), _place(n, 12, (0, 63, 64, 69), (1, 65)))
    return Batch(f"mixed70-k{ksize}", planes, 4, 3, ksize, thr, 0, 0, _run_all(O, planes, 4, 3, ksize, thr, 0, 0))


@functools.lru_cache(maxsize=None)
def cuda70(O):
    """The same planes under TF_VARIANT_CUDA's stop rule: one loop of 12 iterations, no median."""
    E = _never70(O, 0)
    thr = pick_thr(E, 1, 4, cuda70_ok)
    n = np.array([stops(e, thr, 1, 4)[0] for e in E])
    planes = _take(_planes70(O), _place(n, 12, (0, 63, 64, 69), (1, 65)))
    return Batch("cuda70", planes, 4, 3, 0, thr, 1, 0, _run_all(O, planes, 4, 3, 0, thr, 1, 0))


def over1024_ok(n, total=6):
    n = np.asarray(n)
    stopped = n < total
    return bool(6 <= stopped.sum() <= 10 and (n[stopped] % 2 == 1).any() and (n[stopped] % 2 == 0).any())


@functools.lru_cache(maxsize=None)
def over1024(O):
    """B = 1025 pairs of 40 x 64: 16 different pairs, tiled and shuffled; inner 6, outer 1, no median; about half of them stop."""
    h, w = 40, 64
    amps = np.logspace(-1.5, 0.3, 16)
    base = _stack([pair_planes(O, 900 + b, h, w, float(amps[b])) for b in range(16)])
    E = _run_all(O, base, 6, 1, 0, -1.0, 0, 0)[1]
    thr = pick_thr(E, 0, 6, over1024_ok)
    ref16 = _run_all(O, base, 6, 1, 0, thr, 0, 0)
    idx = np.random.default_rng(77).permutation(np.arange(1025) % 16)
    ref = ([s[idx] for s in ref16[0]], ref16[1][idx], ref16[2][idx], ref16[3][idx])
    return Batch("over1024", _take(base, idx), 6, 1, 0, thr, 0, 0, ref)


def has_denormals(batch):
    """does the reference's final state of the batch hold denormal values?"""
    return any(np.any((np.abs(s) < np.finfo(np.float32).tiny) & (s != 0)) for s in batch.ref_state)


# ---- strip layouts ---------------------------------------------------------------------------------------------------------------------
def block_shape(w):
    """(QX, RY, threads) of the row-strip kernels at width w: strip_shape's rule (teeflow_tvl1_host.hip.h)"""
    qx = (w + 3) // 4
    ry = max(1, 256 // qx)
    return qx, ry, 256 if qx * ry <= 256 else (qx * ry + 63) // 64 * 64


def fixed_strip_rows(h, w, B, strip_blocks):
    """(n, R) of strip_shape: R = RY * n rows per strip of k_iter_rows, and of k_iter2_rows for a sub-batch above 1024 pairs"""
    ry = block_shape(w)[1]
    n = min(16, max(2, h * B // (strip_blocks * ry)))
    return n, ry * n


STRIP_BLOCKS_210 = (26, 17, 1)      # strip_blocks at which one pair of 210 x 210 gets n = 2, 3 and 16 (k_iter_rows)
STRIP_BLOCKS_ONE = 100              # ... at which 1025 pairs of 40 x 64 get n = 16: one strip per pair
LAYOUT_SHAPES = ((97, 131), (210, 210), (40, 300), (61, 16), (9, 1100), (6, 2048))


def slot_values(h, w):
    """strip_test_slots 1 .. smax + 1 for one pair: every strip count the rule allows at this shape, and one value beyond"""
    ry = block_shape(w)[1]
    return list(range(1, max(1, h // (4 * ry)) + 2))


def strip_rule(L, n_active, h, ry, slots):
    R, S = C.c_int(), C.c_int()
    L.tf_dbg_strip_rule(n_active, h, ry, slots, C.byref(R), C.byref(S))
    return R.value, S.value
