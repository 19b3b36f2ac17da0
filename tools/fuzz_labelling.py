#!/usr/bin/env python3
"""Randomised parity of the calls behind the tiled union-find labeller (csrc/teeflow_ccl.hip.h) with scipy.ndimage: each case draws one of
  clean      DenseFlow.clean_masks(class_map, ids, min_size): 1..3 adversarial masks per frame painted with distinct values over 0; ids
             present, absent, 0 and repeated; min_size mostly on a component's exact size or one above it
  otsu       DenseFlow.otsu_masks(rgb, min_size, return_thresholds=True): frames built from adversarial masks at two grey levels with
             per-channel jitter, so that Otsu's threshold falls between the levels (checked; redrawn and counted otherwise); a tenth are
             plain noise frames, compared with the host twin masks.predict_movie_thres
  centroids  DenseFlow.av_centroids(mask): C in {1, 2}, values True, 1, 255 or mixed non-zero
on frames of tests/labelling_cases.py::adversarial, H in 1..80, W in 1..200, N in 1..6, a fifth of them degenerate or on the 64 x 16
tile's multiples.  The expected results come from the references below, written on scipy.ndimage with integers, not from the host
twins (tests/test_labelling_cases_cpu.py pins the two to each other).  Masks are compared bit for bit with dtype, shape and
contiguity, areas and centroids exactly.  Every fifth case also runs frame by frame (each frame with the neighbours its temporal
window reads) and must equal the batched call.  Stops at the first mismatch and prints the draw and how to run that case alone; never
retries; an error return from the library ends the run.
usage: python tools/fuzz_labelling.py [cases] [seed] [only]      ("only": run just that case number of the same draw)"""
import os
import sys
import time

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S4 = ndimage.generate_binary_structure(2, 1)
S8 = np.ones((3, 3), bool)
SPECIAL_H = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 79, 80)
SPECIAL_W = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193)
CALLS = ("clean", "otsu", "centroids")


# ---- the references: scipy.ndimage and integers ------------------------------------------------------------------------------
def ref_window(planes):
    """moving_avg_mask's defaults over bool [N,H,W]: per frame j the count of set frames among clamp(j-1), j, clamp(j+1), clamp(j+2),
    kept where it is >= 2 (count / 4 > 0.49 without floats)"""
    planes = np.asarray(planes, bool)
    N = planes.shape[0]
    out = np.empty_like(planes)
    for j in range(N):
        count = sum(planes[min(max(k, 0), N - 1)].astype(np.int64) for k in (j - 1, j, j + 1, j + 2))
        out[j] = count >= 2
    return out


def ref_fill(m):
    """(m with its holes filled, whether that changed m): a 4-connected component of the background is a hole iff none of its pixels
    lies on the border"""
    lab, n = ndimage.label(~m, structure=S4)
    open_ = np.zeros(n + 1, bool)
    for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
        open_[edge] = True
    open_[0] = True
    hole = ~open_[lab]
    return m | hole, bool(hole.any())


def ref_sizes(filled):
    """(labels int [H,W], sizes int [n + 1] with sizes[0] the background's count) of the 4-connected components of a bool plane"""
    lab, n = ndimage.label(filled, structure=S4)
    return lab, np.bincount(lab.ravel(), minlength=n + 1)


def ref_small(filled, min_size):
    """(the plane without its components of fewer than min_size pixels, any dropped, any kept)"""
    lab, sizes = ref_sizes(filled)
    keep = sizes >= int(min_size)
    keep[0] = False
    return keep[lab], bool((~keep[1:]).any()), bool(keep[1:].any())


def ref_clean(cmap, ids, min_size):
    """tf_clean_masks: bool [len(ids) + 1, N, H, W], 'bkgd' last"""
    out = []
    for cls in ids:
        m = ref_window(cmap == cls)
        out.append(np.stack([ref_small(ref_fill(m[f])[0], min_size)[0] for f in range(m.shape[0])]))
    return np.stack(out + [~np.any(out, axis=0)])


def ref_otsu(frame_masks, min_size):
    """tf_otsu_masks for frames whose thresholded masks are frame_masks [N,H,W]: fill and size per frame, then the window"""
    return ref_window(np.stack([ref_small(ref_fill(m)[0], min_size)[0] for m in frame_masks]))


def ref_components(frame):
    """the 8-connected components of frame != 0 as integer rows (area, first pixel's raster index, sum of rows, sum of columns)"""
    lab, n = ndimage.label(np.asarray(frame) != 0, structure=S8)
    flat = lab.ravel()
    idx = np.flatnonzero(flat).astype(np.int64)
    lbl = flat[idx]
    rows, cols = np.divmod(idx, lab.shape[1])
    t = np.zeros((n + 1, 4), np.int64)
    t[:, 1] = flat.size
    np.add.at(t[:, 0], lbl, 1)
    np.minimum.at(t[:, 1], lbl, idx)
    np.add.at(t[:, 2], lbl, rows)
    np.add.at(t[:, 3], lbl, cols)
    return t[1:]


def ref_centroid(frame):
    """((row, col), area) of the component of largest area, on a tie the one whose first pixel comes first; ((0, 0), 0) if there is none"""
    t = ref_components(frame)
    if len(t) == 0:
        return (0.0, 0.0), 0
    area, _, sr, sc = (int(v) for v in min(t.tolist(), key=lambda r: (-r[0], r[1])))
    return (float(sr) / float(area), float(sc) / float(area)), area


def tied_at_the_maximum(frame):
    a = np.sort(ref_components(frame)[:, 0])
    return len(a) >= 2 and a[-1] == a[-2]


# ---- the draw --------------------------------------------------------------------------------------------------------------------
class Case:
    """one drawn call: its inputs, the expected result and what the draw covers (`cover`: hole_filled, drops_and_keeps, odd_ids,
    twins_tied [per twins frame], redraws, built, min_kind)"""

    def __init__(self, name, call, **kw):
        self.name, self.call = name, call
        self.cover = dict(hole_filled=False, drops_and_keeps=False, odd_ids=False, twins_tied=[], redraws=0, built=False, min_kind=None)
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def draw_size(rng, lo):
    H, W = int(rng.integers(lo, 81)), int(rng.integers(lo, 201))
    if rng.random() < 0.2:                                                    # degenerate, or on the tile's multiples
        k = int(rng.integers(0, 3))
        if k != 1:
            H = int(rng.choice([v for v in SPECIAL_H if v >= lo]))
        if k != 0:
            W = int(rng.choice([v for v in SPECIAL_W if v >= lo]))
    return H, W


class _Frames:
    """adversarial frames of one call: the families come in a shuffled round, so frames differ in family or, after nine, in seed"""

    def __init__(self, rng, H, W, cover):
        from tests import labelling_cases as LC
        self.LC, self.rng, self.H, self.W, self.cover = LC, rng, H, W, cover
        self.round, self.names = [], []

    def next(self):
        if not self.round:
            self.round = [f for f in self.rng.permutation(self.LC.FAMILIES) if f != "twins" or max(self.H, self.W) >= 3]
        fam = self.round.pop()
        m = self.LC.adversarial(self.rng, self.H, self.W, fam)
        if fam == "twins":
            self.cover["twins_tied"].append(tied_at_the_maximum(m))
        self.names.append(fam)
        return m


def _min_size(rng, planes, HW):
    """(min_size, its kind) for filled planes: a component's exact size or one above it (seven draws in ten), else an edge value"""
    sizes = np.unique(np.concatenate([ref_sizes(p)[1][1:] for p in planes] + [np.zeros(0, np.int64)]))
    r = rng.random()
    if r < 0.7 and len(sizes):
        if r < 0.35:                                                          # keeps that component; not the smallest, so that one is dropped
            return int(rng.choice(sizes[1:] if len(sizes) > 1 else sizes)), "size"
        return int(rng.choice(sizes[:-1] if len(sizes) > 1 else sizes)) + 1, "size+1"   # drops that one; not the largest, so that one is kept
    return int(rng.choice([0, 1, HW, HW + 1, -int(rng.integers(1, 1000))])), "edge"


def _cover_sizes(case, planes, min_size):
    drops = keeps = False
    for p in planes:
        _, d, k = ref_small(p, min_size)
        drops, keeps = drops or d, keeps or k
    case.cover["drops_and_keeps"] = drops and keeps


def draw_clean(rng, name):
    N = int(rng.integers(1, 7))
    H, W = draw_size(rng, 1)
    case = Case(name, "clean")
    fr = _Frames(rng, H, W, case.cover)
    K = int(rng.integers(1, 4))
    values = [int(v) for v in rng.choice(np.arange(1, 256), K, replace=False)]
    if rng.random() < 0.25:
        values[0] = 255 if 255 not in values else values[0]
    cmap = np.zeros((N, H, W), np.uint8)
    for f in range(N):
        for v in values:
            cmap[f][fr.next()] = v
    absent = int(rng.choice([v for v in range(1, 256) if v not in values]))
    ids, kinds = [], []
    for _ in range(int(rng.integers(1, 6))):
        r = rng.random()
        if r < 0.5 or (r >= 0.8 and not ids):
            ids.append(int(rng.choice(values))), kinds.append("present")
        elif r < 0.65:
            ids.append(absent), kinds.append("absent")
        elif r < 0.8:
            ids.append(0), kinds.append("zero")
        else:
            ids.append(int(rng.choice(ids))), kinds.append("repeat")
    filled = []
    for cls in sorted(set(ids)):
        m = ref_window(cmap == cls)
        for f in range(N):
            p, changed = ref_fill(m[f])
            filled.append(p)
            case.cover["hole_filled"] |= changed
    min_size, case.cover["min_kind"] = _min_size(rng, filled, H * W)
    _cover_sizes(case, filled, min_size)
    case.cover["odd_ids"] = len(set(ids)) < len(ids) or absent in ids
    case.cmap, case.ids, case.min_size, case.shape = cmap, ids, min_size, (N, H, W)
    case.want = ref_clean(cmap, ids, min_size)
    case.name += f"_clean_{N}x{H}x{W}_values{values}_ids{ids}_min{min_size}_{'+'.join(fr.names)}"
    return case


def _lumas(rgb):
    """the frame's luma as the host sums it (rgb2gray: the BLAS's order) and as the device does (tests/luma_cases.py): they part by an
    ulp at some triples, which can move a pixel across a histogram edge and Otsu's threshold by a bin"""
    from tee_optical_flow_amd.frames import rgb2gray
    from tests.luma_cases import luma
    return rgb2gray(rgb), luma(rgb)


def build_rgb(rng, mask):
    """uint8 [H,W,3] with the mask at one grey level of [150, 250] over another of [5, 90], each channel jittered by +-3, or None
    where the host's threshold_otsu does not fall strictly between the two levels' lumas, in the host's and in the device's order of
    the luma sum alike.  skimage's threshold is the centre of the background's last occupied bin (every split in the empty bins behind
    it has the same variance; argmax takes the first), so background pixels in that bin's upper half would count as foreground: they
    take the bytes of the brightest background pixel not above the threshold, which is still the level with a jitter of +-3, until
    none is left (the minimum and the bins stay)."""
    from tee_optical_flow_amd.masks import threshold_otsu
    fg, bg = int(rng.integers(150, 251)), int(rng.integers(5, 91))
    rgb = (np.where(mask, fg, bg)[..., None] + rng.integers(-3, 4, mask.shape + (3,))).astype(np.uint8)
    if mask.all() or not mask.any():
        return None
    for _ in range(16):
        above = np.zeros(mask.shape, bool)
        for g in _lumas(rgb):
            thr = threshold_otsu(g)
            if not thr < g[mask].min():
                return None
            above |= ~mask & (g > thr)
        if not above.any():
            return rgb
        below = ~mask & ~above
        if not below.any():
            return None
        rgb[above] = rgb[np.unravel_index(np.argmax(np.where(below, g, -1.0)), mask.shape)]
    return None


def between_levels(rgb, mask, thr):
    """whether thr parts the frame's two levels in the device's luma"""
    g = _lumas(rgb)[1]
    return bool(g[~mask].max() < thr < g[mask].min())


def draw_otsu(rng, name):
    N = int(rng.integers(2, 7))
    H, W = draw_size(rng, 2)
    case = Case(name, "otsu")
    case.shape = (N, H, W)
    if rng.random() < 0.1:                                                    # the threshold itself is the subject: against the host twin
        from tee_optical_flow_amd import masks
        while True:                                                           # (redrawn where the two orders of the luma sum part on a pixel)
            case.rgb = rng.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
            if all(np.array_equal(a > masks.threshold_otsu(a), b > masks.threshold_otsu(b)) for a, b in (_lumas(fr) for fr in case.rgb)):
                break
            case.cover["redraws"] += 1
        case.min_size = int(rng.choice([0, 1, int(rng.integers(2, 30)), H * W + 1, -1]))
        case.want = masks.predict_movie_thres(case.rgb, config=_Cfg(case.min_size))["otsu"][..., 0]
        case.levels = None
        case.name += f"_otsu_noise_{N}x{H}x{W}_min{case.min_size}"
        return case
    case.cover["built"] = True
    fr = _Frames(rng, H, W, case.cover)
    frames, fmasks = [], []
    for f in range(N):
        for _ in range(100):
            m = fr.next()
            rgb = build_rgb(rng, m)
            if rgb is not None:
                break
            case.cover["redraws"] += 1
            fr.names[-1] += "(redrawn)"
        else:
            raise RuntimeError(f"{name}: no frame with Otsu's threshold between its levels in 100 draws")
        frames.append(rgb), fmasks.append(m)
    filled = []
    for m in fmasks:
        p, changed = ref_fill(m)
        filled.append(p)
        case.cover["hole_filled"] |= changed
    case.min_size, case.cover["min_kind"] = _min_size(rng, filled, H * W)
    _cover_sizes(case, filled, case.min_size)
    case.rgb, case.fmasks = np.stack(frames), np.stack(fmasks)
    case.want = ref_otsu(fmasks, case.min_size)
    case.name += f"_otsu_{N}x{H}x{W}_min{case.min_size}_{'+'.join(fr.names)}"
    return case


def draw_centroids(rng, name):
    N = int(rng.integers(1, 7))
    H, W = draw_size(rng, 1)
    C = int(rng.integers(1, 3))
    kind = str(rng.choice(["bool", "one", "255", "mixed"]))
    case = Case(name, "centroids")
    fr = _Frames(rng, H, W, case.cover)
    m = np.stack([fr.next() for _ in range(N)])
    if kind == "bool":
        a = np.zeros((N, H, W, C), bool)
        a[..., 0] = m
        a[..., 1:] = rng.random((N, H, W, C - 1)) < 0.5                       # channel 1 is not read
    else:
        a = np.zeros((N, H, W, C), np.uint8)
        a[..., 0] = m * (1 if kind == "one" else 255 if kind == "255" else rng.integers(1, 256, (N, H, W)))
        a[..., 1:] = rng.integers(0, 256, (N, H, W, C - 1))
    case.mask, case.shape = a, (N, H, W)
    case.want = [ref_centroid(m[f]) for f in range(N)]
    case.name += f"_centroids_{N}x{H}x{W}x{C}_{kind}_{'+'.join(fr.names)}"
    return case


class _Cfg:
    def __init__(self, min_size):
        self.min_mask_size = min_size


def draw(seed, c):
    rng = np.random.default_rng([seed, c])
    call = CALLS[int(rng.choice(3, p=[0.4, 0.35, 0.25]))]
    return {"clean": draw_clean, "otsu": draw_otsu, "centroids": draw_centroids}[call](rng, f"fuzz_{seed}_{c}")


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def _same_planes(got, want, what):
    """got: the device's bool [..., H, W, 2]; want: bool [..., H, W]"""
    assert got.dtype == np.bool_ and got.shape == want.shape + (2,) and got.flags.c_contiguous, (what, got.dtype, got.shape)
    raw = got.view(np.uint8)
    assert raw.max(initial=0) <= 1, (what, "a byte that is neither 0 nor 1")
    for ch in (0, 1):
        bad = np.argwhere(got[..., ch] != want)
        assert len(bad) == 0, f"{what}: channel {ch} differs at {len(bad)} pixels, first at {tuple(bad[0])}"


def _window_span(j, N):
    return max(j - 1, 0), min(j + 2, N - 1)


def check(eng, case, per_frame):
    N = case.shape[0]
    if case.call == "clean":
        got = eng.clean_masks(case.cmap, case.ids, case.min_size)
        _same_planes(got, case.want, "clean_masks")
        if per_frame and N > 1:
            for j in range(N):
                lo, hi = _window_span(j, N)
                one = eng.clean_masks(case.cmap[lo:hi + 1], case.ids, case.min_size)
                assert np.array_equal(one[:, j - lo], got[:, j]), f"clean_masks: frame {j} alone differs from the batched call"
    elif case.call == "otsu":
        got, thr = eng.otsu_masks(case.rgb, case.min_size, return_thresholds=True)
        got, thr = got.copy(), thr.copy()
        assert thr.dtype == np.float64 and thr.shape == (N,)
        if case.cover["built"]:
            for f in range(N):
                assert between_levels(case.rgb[f], case.fmasks[f], thr[f]), f"otsu_masks: frame {f}'s threshold {thr[f]} is not between the levels"
        _same_planes(got, case.want, "otsu_masks")
        if per_frame:
            for j in range(N):
                lo, hi = _window_span(j, N)
                one, t1 = eng.otsu_masks(case.rgb[lo:hi + 1], case.min_size, return_thresholds=True)
                assert np.array_equal(one[j - lo], got[j]) and t1[j - lo] == thr[j], f"otsu_masks: frame {j} alone differs from the batched call"
    else:
        cent, area = eng.av_centroids(case.mask)
        assert cent.dtype == np.float64 and cent.shape == (N, 2) and area.dtype == np.int64 and area.shape == (N,)
        for f in range(N):
            (r, c), a = case.want[f]
            assert int(area[f]) == a and float(cent[f, 0]) == r and float(cent[f, 1]) == c, \
                f"av_centroids: frame {f} gives area {area[f]} centroid {tuple(cent[f])}, expected {a} {(r, c)}"
        if per_frame:
            for f in range(N):
                c1, a1 = eng.av_centroids(case.mask[f:f + 1])
                assert a1[0] == area[f] and np.array_equal(c1[0], cent[f]), f"av_centroids: frame {f} alone differs from the batched call"


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    only = int(sys.argv[3]) if len(sys.argv) > 3 else None
    assert all((k / 4 > 0.49) == (k >= 2) for k in range(5))                 # the window's float rule is the integer rule
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    t0 = time.time()
    done = 0
    for c in range(cases) if only is None else [only]:
        case = draw(seed, c)
        try:
            check(eng, case, per_frame=c % 5 == 0)
        except AssertionError as e:
            print(f"MISMATCH case {c} (seed {seed}): {case!r}\n  {e}\n  rerun alone: python tools/fuzz_labelling.py {cases} {seed} {c}", flush=True)
            eng.close()
            sys.exit(1)
        done += 1
        print(f"case {c}: {case!r} ok", flush=True)
    eng.close()
    print(f"{done}/{done} cases identical in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
