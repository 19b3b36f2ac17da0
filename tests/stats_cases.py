"""Named, seeded cases for the device statistics tail (k_radlong_hist, the radix select, radlong_reduce, the angle bins and
k_polar_mode, and their Python glue in analysis.py), numpy models of the two device algorithms, and the comparison of a device
call with plain numpy that the GPU tests and tools/fuzz_stats.py share.  A helper module: nothing here is collected.

How exact values are planted:
  rad/long planes (float64): a one-column study (W = 1) with the centroid (-1.0, 0.0) in every frame has u0 = -1, u1 = 0
    exactly, so rad = -fx and long = fy for finite float32 flow: the planes are the flow that was written.
  polar planes (float32): fy = 0 gives mag = |fx| for 1e-15 < |fx| < 1e15; angle populations come from a pool of flow vectors whose
    bin k = rint(ang * 100) is read off analysis.cart_to_polar on the host."""
import numpy as np

from tee_optical_flow_amd import analysis as A

CENT = (-1.0, 0.0)
NBINS = (1, 2, 3, 7, 50, 1000, 1024, 4096, 10000)
PERCENTILES = (0, 100, 50, 99.9, 0.001, 25, 75, 99, 1)
PERC_PAIRS = ((0, 100), (100, 0), (50, 50), (0.001, 99.9), (99.9, 0.001), (25, 75))      # (perc_lo, perc_hi)
COUNTS = (1, 2, 3, 100, 101)
COMPS = ("radial", "longitudinal")
POLAR_OUTS = ("mag_freq", "ang_freq", "mag_edges", "ang_edges", "hi")
TOO_MANY_BINS = "Too many bins for data range"


# ---- numpy models of the device algorithms ----------------------------------------------------------------------------------
def device_hist_rule(x, edges):
    """k_radlong_hist's rule in numpy: the float64 estimate, then one step of numpy's fix-up against the edges (float32 edges are
    passed to the kernel as float64, exactly)"""
    e = np.asarray(edges).astype(np.float64)
    nb = len(e) - 1
    x = np.asarray(x).astype(np.float64)
    x = x[(x != 0) & (x >= e[0]) & (x <= e[nb])]
    idx = np.clip((((x - e[0]) / (e[nb] - e[0])) * nb).astype(np.int64), 0, nb - 1)
    idx -= x < e[idx]
    up = (idx != nb - 1) & (x >= e[np.minimum(idx + 1, nb)])
    idx += up
    return np.bincount(idx, minlength=nb)


def f64_key(v):
    """the order-preserving map double -> uint64 of teeflow_analysis.hip.h"""
    b = np.ascontiguousarray(v, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def f64_unkey(k):
    k = np.uint64(k)
    b = (k & np.uint64(0x7FFFFFFFFFFFFFFF)) if (k >> np.uint64(63)) else ~k
    return np.array([b], np.uint64).view(np.float64)[0]


def select_model(v, rank):
    """tf_radlong_select for one slot in numpy: four 16-bit digit passes over the keys of the non-zero values (k_radlong_sel_hist),
    each followed by the 256 x 256 two-level scan with its `<= r` walk (k_radlong_sel_scan)"""
    v = np.asarray(v, np.float64).ravel()
    k = f64_key(v[v != 0])
    prefix = np.uint64(0)
    r = int(rank)
    for shift in (48, 32, 16, 0):
        himask = np.uint64(0) if shift == 48 else np.uint64((~0 << (shift + 16)) & 0xFFFFFFFFFFFFFFFF)
        sel = (k & himask) == (prefix & himask)
        hist = np.bincount(((k[sel] >> np.uint64(shift)) & np.uint64(0xFFFF)).astype(np.int64), minlength=65536)
        part = hist.reshape(256, 256).sum(1)
        t = 0
        while t < 255 and part[t] <= r:
            r -= int(part[t]); t += 1
        b = 0
        while b < 255 and hist[t * 256 + b] <= r:
            r -= int(hist[t * 256 + b]); b += 1
        prefix |= np.uint64((t * 256 + b) << shift)
    return f64_unkey(prefix)


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """path 'radlong': flow, mask, cent, n_used, frame_rate, param, nbins, perc_lo, perc_hi.
    path 'polar':   flow, mask, n_used, frame_rate, param, nbins, percentile (label 'm' of study()).
    raises: None, or the exception both the host twin and the device call raise; tags: the families the case belongs to."""

    def __init__(self, name, path, flow, mask, n_used, *, cent=None, frame_rate=50.0, param="velocity", nbins=1000, perc_lo=1, perc_hi=99,
                 percentile=99, raises=None, tags=(), info=None):
        self.name, self.path, self.flow, self.mask, self.n_used = name, path, flow, mask, int(n_used)
        self.cent, self.frame_rate, self.param, self.nbins = cent, frame_rate, param, int(nbins)
        self.perc_lo, self.perc_hi, self.percentile, self.raises = perc_lo, perc_hi, percentile, raises
        self.tags, self.info = frozenset(tags), dict(info or {})

    def __repr__(self):
        return (f"Case({self.name!r}, {self.path}, flow {self.flow.dtype}{list(self.flow.shape)}, mask C={self.mask.shape[3]}, n_used={self.n_used}, "
                f"param={self.param}, frame_rate={self.frame_rate!r}, nbins={self.nbins}, perc=({self.perc_lo!r}, {self.perc_hi!r}), "
                f"percentile={self.percentile!r}, raises={self.raises})")

    def study(self):
        return A.FlowStudy(self.flow, {"m": self.mask}, self.frame_rate, nframes=self.n_used)

    def field(self):
        return A.param_field(self.flow, self.mask, self.param, self.frame_rate, self.n_used)

    def planes(self):
        """the two planes the statistics run over, from plain numpy: (rad, long) float64 or (mag, ang) float32"""
        f = self.field()
        if self.path == "radlong":
            return A.calculate_comp_magnitude(f, self.cent)
        return A.cart_to_polar(f[..., 0], f[..., 1])


def _column(name, path, rad, lon=None, *, dtype=np.float32, C=2, empty=(), extra=1, **kw):
    """a one-column study whose planes (velocity) are the given per-frame rows: rad[n] -> -fx, lon[n] -> fy (radlong), or fx = rad[n],
    fy = 0 (polar; lon must be None).  `empty` frames get an all-zero mask; `extra` frames follow n_used for the gradient."""
    rad = np.asarray(rad)
    n, H = rad.shape
    flow = np.zeros((n + extra, H, 1, 2), dtype)
    if path == "radlong":
        lon = -rad[:, ::-1] if lon is None else np.asarray(lon)
        flow[:n, :, 0, 0] = -rad
        flow[:n, :, 0, 1] = lon
    else:
        flow[:n, :, 0, 0] = rad
    for j in range(extra):
        flow[n + j] = flow[j % n][::-1]
    mask = np.ones((n + extra, H, 1, C), bool)
    for f in empty:
        mask[f] = False
    return Case(name, path, flow, mask, n, cent=[CENT] * n if path == "radlong" else None, **kw)


def _image(name, path, seed, N, H, W, *, density=0.7, dtype=np.float16, C=2, empty=(), extra=1, **kw):
    """an ordinary H x W study: float16-quantised speckle, a random mask, interior centroids"""
    rng = np.random.default_rng(seed)
    flow = rng.normal(0, 4, (N + extra, H, W, 2)).astype(np.float16).astype(dtype)
    mask = rng.random((N + extra, H, W, C)) < density
    if C == 2:
        mask[..., 1] = mask[..., 0]
    for f in empty:
        mask[f] = False
    cent = [(float(rng.uniform(0, H)), float(rng.uniform(0, W))) for _ in range(N)] if path == "radlong" else None
    return Case(name, path, flow, mask, N, cent=cent, **kw)


def _f16(rng, shape, scale=4.0):
    return (rng.standard_normal(shape) * scale).astype(np.float16).astype(np.float32)


def _counted_rows(rng, H, counts, polar):
    """one row per count: that many non-zero float16-quantised values at random places, zeros elsewhere"""
    rows = np.zeros((len(counts), H), np.float32)
    for i, c in enumerate(counts):
        v = _f16(rng, c)
        v[v == 0] = 1.0
        rows[i, rng.permutation(H)[:c]] = np.abs(v) if polar else v
    return rows


def _shared_cases(path):
    """the families that apply to both paths; polar rows are magnitudes (fy = 0), so they are kept non-negative there only where
    the sign matters to the case"""
    polar = path == "polar"
    p = "p_" if polar else "r_"
    out = []
    rng = np.random.default_rng(1234 + polar)
    variants = ((np.float16, 2, 50.0), (np.float32, 1, np.float64(49.9)))
    # ties: float16-quantised values, every param, both flow types, both mask layouts, both gradient division types
    for param in A.PARAMS:
        for dt, C, fr in variants:
            rows = np.round(_f16(rng, (6, 777), 1.5) * 2) / 2               # coarse enough that the products of PWR tie as well
            out.append(_column(f"{p}ties_f16_{param}_{np.dtype(dt).name}_C{C}", path, rows, dtype=dt, C=C, frame_rate=fr, param=param,
                               empty=(3,), nbins=1000, perc_lo=5, perc_hi=95, percentile=95, tags=("ties", "empty")))
    rows = rng.choice(np.float32([-1.5, 0.25, 3.0]), (3, 1000))
    out.append(_column(p + "ties_three_values", path, rows, nbins=7, perc_lo=30, perc_hi=70, percentile=70, tags=("ties",), info={"distinct": 3}))
    rows = np.full((3, 515), 2.5, np.float32)
    rows[0, [3, 99, 257, 514]] = [2.75, -4.0, 2.4990234, 7.0]
    rows[1, [0, 256]] = [2.5009766, 1.0]
    rows[2, 300] = 2.5009766 if polar else -2.5
    out.append(_column(p + "ties_one_value_but_a_handful", path, rows, nbins=50, perc_lo=0.5, perc_hi=99.5, percentile=99.5, tags=("ties",)))
    # on the edges
    rows = np.stack([rng.permutation(1025), rng.permutation(1025)]).astype(np.float32) / 128
    out.append(_column(p + "edges_pow2_range_0_8_nbins_1024", path, rows, lon=rows[::-1].copy() if not polar else None, nbins=1024,
                       tags=("edges", "every_datum_on_an_edge"), info={"lo": 0.0, "hi": 8.0}))
    rows = rng.integers(0 if polar else -160, 241, (2, 3001)).astype(np.float32) / 8
    rows[0, :2] = [0 if polar else -20.0, 30.0]
    out.append(_column(p + "edges_nbins_1000_data_on_eighths", path, rows, lon=rows[::-1].copy() if not polar else None, nbins=1000, tags=("edges",),
                       info={"lo": 0.0 if polar else -20.0, "hi": 30.0}))
    # values equal to numpy's own edges and one ulp beside them, the first and the last edge included
    for tag, mn, mx, nb in (("dyadic", np.float32(0.5 if polar else -2.875), np.float32(9.5 if polar else 9.625), 50 if not polar else 36),
                            ("ragged", np.float32(0.7 if polar else -3.7), np.float32(9.3), 50),
                            ("ragged_1000", np.float32(0.013 if polar else -41.3), np.float32(57.9), 1000)):
        e = A._polar_edges(mn, mx, nb) if polar else np.linspace(np.float64(mn), np.float64(mx), nb + 1).astype(np.float32)
        v = np.concatenate([e, np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf)), [mn, mx]]).astype(np.float32)
        v = v[(v >= mn) & (v <= mx) & (v != 0)]
        rows = np.stack([rng.permutation(v), rng.permutation(v)])
        out.append(_column(f"{p}edges_numpys_own_{tag}", path, rows, lon=rows[::-1].copy() if not polar else None, nbins=nb,
                           tags=("edges", "own_edges"), info={"lo": float(mn), "hi": float(mx)}))
    # bin counts
    for nb in NBINS:
        rows = _f16(rng, (2, 3000))
        out.append(_column(f"{p}nbins_{nb}", path, rows, nbins=nb, tags=("nbins",)))
    # percentiles: counts that make the virtual index an integer, a half, and clipped at count - 1
    for lo, hi in PERC_PAIRS:
        rows = _counted_rows(rng, 128, COUNTS, polar)
        out.append(_column(f"{p}percentiles_{lo}_{hi}", path, rows, nbins=50, perc_lo=lo, perc_hi=hi, percentile=hi, tags=("percentiles",),
                           info={"counts": COUNTS}))
    # select keys
    x = np.float32(1.5) * np.exp2(np.arange(-8, 9)).astype(np.float32)
    rows = np.stack([rng.permutation(np.concatenate([x, x if polar else -x, x[:5]])) for _ in range(2)])
    out.append(_column(p + "keys_differ_in_the_top_digit_only", path, rows, nbins=7, perc_lo=40, perc_hi=60, percentile=60, tags=("keys", "top_digit")))
    c = np.float32(3.3)
    cl = [c]
    for _ in range(40):
        cl.append(np.nextafter(cl[-1], np.float32(np.inf)))
    cl = np.float32(cl)
    rows = np.stack([rng.choice(cl, 400), rng.choice(np.concatenate([cl, cl if polar else -cl]), 400)])
    out.append(_column(p + "keys_one_ulp_cluster_f32", path, rows, nbins=3, perc_lo=33, perc_hi=66, percentile=66, tags=("keys", "cluster32")))
    small, large = (1e-14, 1e14) if polar else (1e-45, 3.0e38)              # polar: the range where mag = |fx| exactly
    pool = np.float32([small, 3 * small, 1e-40 if not polar else 1e-13, 1.0, large, large / 3])
    pool = np.concatenate([pool, pool if polar else -pool, [0.0, -0.0]]).astype(np.float32)
    rows = np.stack([rng.choice(pool, 300) for _ in range(2)])
    rows[:, :len(pool)] = pool
    out.append(_column(p + "keys_denormals_and_huge_and_signed_zeros", path, rows, nbins=1000, perc_lo=10, perc_hi=90, percentile=90,
                       tags=("keys", "extremes", "signed_zeros")))
    # empty frames
    for which, empty, exc in (("first", (0,), IndexError if polar else None), ("middle", (2,), None), ("last", (4,), None),
                             ("all", (0, 1, 2, 3, 4), IndexError if polar else None)):
        for param in A.PARAMS:
            rows = _f16(rng, (5, 300))
            if polar:
                rows = np.abs(rows)
            out.append(_column(f"{p}empty_{which}_{param}", path, rows, param=param, empty=empty, nbins=50, raises=exc, frame_rate=np.float64(30.0),
                               tags=("empty", "empty_" + which), info={"empty": empty}))
    # degenerate range: min == max (numpy's +-0.5 rule), and the same value beside zeros (min = 0)
    rows = np.full((2, 130), 2.5, np.float32)
    out.append(_column(p + "degenerate_one_value_no_zero", path, rows, lon=rows.copy() if not polar else None, nbins=50, tags=("degenerate", "min_eq_max")))
    rows = rows.copy()
    rows[:, ::3] = 0
    out.append(_column(p + "degenerate_one_value_and_zeros", path, rows, lon=rows.copy() if not polar else None, nbins=50, tags=("degenerate", "min_zero")))
    # two neighbouring values and more bins than numpy can make between them: both paths raise
    if polar:
        rows = np.float32([[3.3, np.nextafter(np.float32(3.3), np.float32(9))] * 20] * 2)
        out.append(_column(p + "too_many_bins", path, rows, nbins=7, raises=ValueError, tags=("too_many_bins",)))
    else:
        # float64 neighbours need a float64 product: two pixels far below the centroid, u0 = 1 and 1 - 5 ulp, no zero in the plane
        flow = np.zeros((2, 1, 2, 2), np.float32)
        flow[..., 0] = 1.0
        out.append(Case(p + "too_many_bins", path, flow, np.ones((2, 1, 2, 1), bool), 2, cent=[(-3e7, 0.0)] * 2, nbins=50, raises=ValueError,
                        tags=("too_many_bins",)))
    # ordinary studies: above 65 536 pixels per frame the kernels' grid is capped and the stride loop runs more than once
    for param, dt, C, fr in (("velocity", np.float16, 2, 50.0), ("PWR", np.float32, 1, np.float64(49.9))):
        out.append(_image(f"{p}image_300x250_{param}", path, 77, 3, 300, 250, param=param, dtype=dt, C=C, frame_rate=fr, empty=(1,), nbins=1000,
                          tags=("image", "big", "empty")))
    out.append(_image(p + "image_37x129_acceleration", path, 78, 4, 37, 129, param="acceleration", nbins=500, perc_lo=2.5, perc_hi=97.5,
                      percentile=97.5, tags=("image",)))
    out.append(_image(p + "image_1x1", path, 79, 3, 1, 1, density=1.0, nbins=3, extra=0, tags=("image", "single_pixel")))
    return out


def _rays_case():
    """float64 products that differ only in their lowest bits: a constant flow along rays k * (a, b) from an integer centroid, where
    u0 = k a / sqrt(k^2 (a^2 + b^2)) rounds to neighbouring doubles for different k"""
    H, W = 97, 131
    c = (48.0, 65.0)
    mask = np.zeros((3, H, W, 1), bool)
    for a, b in ((1, 2), (2, 1), (3, 1), (1, 3), (-1, 2), (2, -3), (1, 1), (3, 2)):
        for k in range(1, 60):
            r, q = int(c[0]) + k * a, int(c[1]) + k * b
            if 0 <= r < H and 0 <= q < W:
                mask[:, r, q] = True
    flow = np.zeros((3, H, W, 2), np.float32)
    flow[0] = (1.7, 0.0)
    flow[1] = (0.3, -2.9)
    flow[2] = (-1.1, 1.3)
    return Case("r_keys_rays_share_48_key_bits", "radlong", flow, mask, 3, cent=[c] * 3, nbins=1000, perc_lo=35, perc_hi=65, tags=("keys", "cluster48"))


def radlong_cases():
    return _shared_cases("radlong") + [_rays_case()]


# angle populations
_POOL = None


def angle_pool():
    """{k: (fx, fy)}: float32 flow vectors whose cart_to_polar angle rounds to bin k = rint(ang * 100), for every k the sweep reaches"""
    global _POOL
    if _POOL is None:
        th = np.arange(0, 629) / 100.0
        v = np.stack([np.cos(th), np.sin(th)], 1).astype(np.float32) * np.float32(3)
        _, ang = A.cart_to_polar(v[:, 0], v[:, 1])
        k = np.rint(ang * np.float32(100)).astype(int)
        _POOL = {}
        for i in range(len(th)):
            _POOL.setdefault(int(k[i]), (v[i, 0], v[i, 1]))
    return _POOL


def _angle_frame(H, W, counts, rng):
    """a frame with counts[k] pixels of bin k at random places, the rest zero flow"""
    pool = angle_pool()
    fr = np.zeros((H * W, 2), np.float32)
    pos = rng.permutation(H * W)
    o = 0
    for k, c in counts.items():
        fr[pos[o:o + c]] = pool[k]
        o += c
    assert o <= H * W
    return fr.reshape(H, W, 2)


def angle_cases():
    rng = np.random.default_rng(99)
    pool = angle_pool()
    ks = sorted(k for k in pool if k >= 1)
    out = []

    def add(name, frames, want, tags):
        flow = np.stack(frames)
        mask = np.ones(flow.shape[:3] + (1,), bool)
        out.append(Case(name, "polar", flow, mask, len(frames), nbins=1000, percentile=99, tags=("angle",) + tags, info={"want_k": want}))

    H, W = 61, 67
    # k, k + 256, k + 512 fall to one thread of k_polar_mode's stride loop; the smallest wins whatever the order of the counts
    add("a_tie_inside_one_threads_stride", [_angle_frame(H, W, {50: 40, 306: 40, 562: 40, 7: 39}, rng),
                                            _angle_frame(H, W, {562: 25, 306: 25, 120: 24}, rng),
                                            _angle_frame(H, W, {306: 9, 50: 9, 562: 9, 51: 8, 305: 8}, rng)], [50, 306, 50], ("tie_stride",))
    add("a_tie_across_waves", [_angle_frame(H, W, {10: 30, 100: 30, 200: 30, 250: 30, 400: 29}, rng),
                               _angle_frame(H, W, {250: 12, 100: 12, 11: 11}, rng)], [10, 100], ("tie_waves",))
    add("a_every_bin_the_same_count", [_angle_frame(H, W, {k: 3 for k in ks}, rng), _angle_frame(H, W, {k: 1 for k in ks[5:]}, rng)],
        [ks[0], ks[5]], ("all_equal",))
    add("a_only_bin_628", [_angle_frame(H, W, {628: 17}, rng), _angle_frame(H, W, {628: 1}, rng)], [628, 628], ("only_628",))
    tiny = np.zeros((H, W, 2), np.float32)
    tiny[5:9, 3:40] = (3.0, 0.003)                                            # ang = 0.001: not zero, rounds to 0.00
    add("a_nonzero_angles_all_round_to_zero", [tiny, _angle_frame(H, W, {314: 5}, rng), tiny], [0, 314, 0], ("round_to_zero",))
    one = np.zeros((3, 1, 1, 2), np.float32)
    one[0, 0, 0] = pool[157]
    one[2, 0, 0] = pool[471]
    add("a_single_pixel", list(one), [157, 0, 471], ("single_pixel",))
    big = _angle_frame(300, 250, {k: 100 for k in ks[::7]} | {ks[3]: 100, 600: 101}, rng)
    add("a_image_300x250", [big, big[::-1].copy()], [600, 600], ("big",))
    return out


def polar_cases():
    return _shared_cases("polar") + angle_cases()


def all_cases():
    return radlong_cases() + polar_cases()


# ---- numpy against a device call ----------------------------------------------------------------------------------------------
def same(got, want, what):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=False), (what, g.dtype, w.dtype, g.shape, w.shape)


def host_radlong(case):
    """(rad, long, {comp: (freq, edges[:-1], hi, lo)}) from plain numpy: calculate_comp_magnitude of the host param field and
    calc_bidirectional_hist of its planes"""
    rad, lon = case.planes()
    out = {}
    for name, arr in zip(COMPS, (rad, lon)):
        f, e, hi, lo = A.calc_bidirectional_hist(arr, case.n_used, perc_lo=case.perc_lo, perc_hi=case.perc_hi, nbins=case.nbins)
        out[name] = (f, np.asarray(e)[:-1], hi, lo)
    return rad, lon, out


def check_radlong_result(dev, rad, lon, want, case):
    """a device result (return_arrays=True) against numpy: planes, freq, edges, hi, lo, and per frame sum(freq - 1) against the
    count of non-zero in-range values (a lost atomic add cannot hide behind an equal-looking row)"""
    same(dev["rad_arr"], rad, (case.name, "rad_arr"))
    same(dev["long_arr"], lon, (case.name, "long_arr"))
    for comp, arr in zip(COMPS, (rad, lon)):
        for i, k in enumerate(("freq", "edges", "hi", "lo")):
            same(dev[comp][i], want[comp][i], (case.name, comp, k))
        mn, mx = arr.min(), arr.max()
        freq = dev[comp][0]
        prev = None
        for f in range(case.n_used):
            fl = arr[f].ravel()
            n_in = int(np.count_nonzero((fl != 0) & (fl >= mn) & (fl <= mx)))
            if n_in:
                prev = n_in
            expect = prev if prev is not None else 0                          # an empty frame repeats the previous row (ones at the start)
            assert int((freq[f] - 1).sum()) == expect, (case.name, comp, f, int((freq[f] - 1).sum()), expect)


def check_radlong(engine, case):
    """both device entries of a rad/long case against numpy"""
    kw = dict(perc_lo=case.perc_lo, perc_hi=case.perc_hi, nbins=case.nbins, return_arrays=True)
    args = (case.flow, case.mask, case.param, case.frame_rate, case.n_used, case.cent)
    if case.raises is not None:
        for call in (lambda: A.param_radlong_stats(*args, **kw), lambda: A.param_radlong_stats(*args, engine=engine, **kw),
                     lambda: A.radlong_stats_device(engine, case.field(), case.cent, **kw)):
            try:
                call()
            except case.raises:
                continue
            raise AssertionError(f"{case.name}: no {case.raises.__name__}")
        return
    rad, lon, want = host_radlong(case)
    check_radlong_result(A.param_radlong_stats(*args, engine=engine, **kw), rad, lon, want, case)
    check_radlong_result(A.radlong_stats_device(engine, case.field(), case.cent, **kw), rad, lon, want, case)


def check_polar(engine, case):
    """calculate_3dhist, polar_project_param and angle_mode_series on the device against numpy"""
    st = case.study()
    kw = dict(nbins=case.nbins, percentile=case.percentile)
    n = case.n_used
    mm, nz, mode, mag, ang = engine.polar_project_param(case.flow, case.mask, A.PARAMS.index(case.param), 1 / case.frame_rate,
                                                       A.gradient_is_f64(case.frame_rate), n, return_arrays=True)
    hm, ha = case.planes()
    assert np.array_equal(mag.view(np.int32), hm.view(np.int32)) and np.array_equal(ang.view(np.int32), ha.view(np.int32)), case.name
    same(mm, np.float32([hm.min(), hm.max(), ha.min(), ha.max()]), (case.name, "minmax"))
    same(nz, np.stack([(hm != 0).sum((1, 2)), (ha != 0).sum((1, 2))], 1).astype(np.int64), (case.name, "counts"))
    want_mode = np.asarray([A._mode_of_rounded(ha[i]) for i in range(n)], np.float32)
    assert mode.dtype == np.float32 and np.array_equal(mode, want_mode, equal_nan=True), (case.name, mode, want_mode)
    got = A.angle_mode_series(st, case.param, "m", engine=engine)
    assert got.dtype == np.float32 and np.array_equal(got, want_mode, equal_nan=True), (case.name, got, want_mode)
    if case.raises is not None:
        for eng in (None, engine):
            try:
                A.calculate_3dhist(st, case.param, "m", engine=eng, **kw)
            except case.raises:
                continue
            raise AssertionError(f"{case.name}: no {case.raises.__name__}")
        return
    host = A.calculate_3dhist(st, case.param, "m", **kw)
    dev = A.calculate_3dhist(st, case.param, "m", engine=engine, **kw)
    for i, k in enumerate(POLAR_OUTS):
        same(dev[i], host[i], (case.name, k))
    # the magnitude rows hold every non-zero value once: a lost atomic add shows here
    prev = None
    for f in range(n):
        c = int(np.count_nonzero(hm[f]))
        prev = c if c else prev
        assert int((dev[0][f] - 1).sum()) == prev, (case.name, "mag_freq", f)


# ---- non-finite flow --------------------------------------------------------------------------------------------------------
def nonfinite_cases():
    """NaN, +inf, -inf in the flow, and inf - inf through the gradient: np.histogram refuses the range in the host twins (ValueError),
    and so must the device calls"""
    out = []
    rng = np.random.default_rng(31)
    for path in ("radlong", "polar"):
        p = "r_" if path == "radlong" else "p_"
        for tag, val, comp, param, dt in (("nan_velocity", np.nan, 0, "velocity", np.float32), ("nan_in_fy_velocity", np.nan, 1, "velocity", np.float16),
                                          ("negative_nan_velocity", -np.nan, 0, "velocity", np.float32),
                                          ("plus_inf_velocity", np.inf, 0, "velocity", np.float16), ("minus_inf_velocity", -np.inf, 0, "velocity", np.float32),
                                          ("plus_inf_pwr", np.inf, 0, "PWR", np.float32), ("nan_acceleration", np.nan, 1, "acceleration", np.float32)):
            c = _column(p + "nonfinite_" + tag, path, np.abs(_f16(rng, (4, 200))) + 1, dtype=dt, param=param, nbins=50, raises=ValueError,
                        tags=("nonfinite",))
            c.flow[2, 77, 0, comp] = np.copysign(np.float32(np.nan), np.float32(-1)) if tag.startswith("negative_nan") else val
            out.append(c)
        c = _column(p + "nonfinite_inf_minus_inf_in_the_gradient", path, np.abs(_f16(rng, (4, 200))) + 1, dtype=np.float16, param="acceleration",
                    nbins=50, raises=ValueError, frame_rate=np.float64(30.0), tags=("nonfinite",))
        c.flow[1, 5, 0, 0] = c.flow[3, 5, 0, 0] = np.inf                     # frame 2's central difference is inf - inf
        out.append(c)
    return out
