"""The luma front door (luma_f64 of csrc/teeflow_cond.hip.h and its three consumers: conditioning, Otsu's histogram and threshold, the
float16 echo): an order-explicit float64 reference and the named frames that tests/test_luma_cpu.py and tests/test_gpu_luma.py share.

The reference is elementwise numpy float64 with one ufunc call per operation -- no `@`, dot, matmul or einsum, so nothing can be fused
or reordered by the host's BLAS and the values are the same on every host.  (frames.rgb2gray, the twin of skimage's `rgb @ coeffs`,
is not: DESIGN.md section 9, row a1.)  Nothing in this module is collected."""
import functools

import numpy as np

from tee_optical_flow_amd import masks

NBINS = 256


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def luma(rgb):
    """uint8 [...,3] -> float64 [...]: ((R/255)*0.2125 + (G/255)*0.7154) + (B/255)*0.0721, the order luma_f64 evaluates"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.shape[-1] == 3
    r = np.multiply(np.divide(rgb[..., 0].astype(np.float64), 255.0), 0.2125)
    g = np.multiply(np.divide(rgb[..., 1].astype(np.float64), 255.0), 0.7154)
    b = np.multiply(np.divide(rgb[..., 2].astype(np.float64), 255.0), 0.0721)
    return np.add(np.add(r, g), b)


def minmax(rgb):
    """uint8 [N,H,W,3] -> float64 [N,2]: each frame's (min, max) of the luma"""
    return np.array([[g.min(), g.max()] for g in map(luma, rgb)], np.float64).reshape(len(rgb), 2)


def condition_luma(g):
    """k_cond_norm's rule on one frame's luma: rint(((g - mn) / mx) * 255) clipped to [0, 255]; NaN (the 0/0 frame) gives 0"""
    mn, mx = g.min(), g.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.rint(np.multiply(np.divide(np.subtract(g, mn), mx), 255.0))
    return np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 255.0)).astype(np.uint8)


def condition(rgb):
    """uint8 [N,H,W,3] -> uint8 [N,H,W], per frame"""
    return np.stack([condition_luma(luma(f)) for f in rgb])


def echo_bits(rgb):
    """uint8 [N,H,W,3] -> uint16 [N,H,W]: the bits of the luma rounded once, from float64, to float16"""
    return luma(rgb).astype(np.float16).view(np.uint16)


def hist_luma(g):
    mn, mx = g.min(), g.max()
    if mn == mx:
        return np.zeros(NBINS, np.int64)
    return np.histogram(g.ravel(), NBINS, range=(mn, mx))[0]


def hist(rgb):
    """uint8 [N,H,W,3] -> int64 [N,256]: np.histogram(g, 256, range=(mn, mx)) per frame; all zeros for a one-valued frame"""
    return np.stack([hist_luma(luma(f)) for f in rgb])


def threshold(rgb):
    """uint8 [N,H,W,3] -> float64 [N]: masks.threshold_otsu (skimage's) of each frame's luma"""
    return np.array([masks.threshold_otsu(luma(f)) for f in rgb], np.float64)


def reference(rgb):
    """all of the above for one call, each frame's luma made once: {"cond", "minmax", "hist", "thr", "echo"}"""
    out = {"cond": [], "minmax": [], "hist": [], "thr": [], "echo": []}
    for f in rgb:
        g = luma(f)
        out["cond"].append(condition_luma(g))
        out["minmax"].append([g.min(), g.max()])
        out["hist"].append(hist_luma(g))
        out["thr"].append(masks.threshold_otsu(g))
        out["echo"].append(g.astype(np.float16).view(np.uint16))
    return {k: np.array(v) for k, v in out.items()}


def numpy_hist_model(g):
    """hist_bin's rule (csrc/teeflow_otsu.hip.h) restated in numpy for one frame's luma with mn < mx: the division-first estimate
    truncated, the clamp to [0, 255], one decrement and one increment against the edges i * step + mn (the last edge is mx).
    -> (counts int64 [256], pixels that took the decrement, pixels that took the increment)"""
    g = np.asarray(g, np.float64).ravel()
    mn, mx = g.min(), g.max()
    assert mn < mx
    step = np.divide(np.subtract(mx, mn), float(NBINS))

    def edge(i):
        return np.where(i == NBINS, mx, np.add(np.multiply(i.astype(np.float64), step), mn))
    i = np.multiply(np.divide(np.subtract(g, mn), np.subtract(mx, mn)), float(NBINS)).astype(np.int64)
    i = np.clip(i, 0, NBINS - 1)
    dec = (g < edge(i)) & (i > 0)
    i = i - dec
    inc = (i != NBINS - 1) & (g >= edge(i + 1))
    i = i + inc
    return np.bincount(i, minlength=NBINS), int(dec.sum()), int(inc.sum())


def ties(g):
    """pixels of one frame's luma at which ((g - mn) / mx) * 255 is exactly k + 0.5: where rint, round and floor(x + .5) part"""
    x = np.multiply(np.divide(np.subtract(g, g.min()), g.max()), 255.0)
    return int((np.subtract(x, np.floor(x)) == 0.5).sum())


# ---- the named frames ---------------------------------------------------------------------------------------------------------------
def _grey(v, shape):
    """grey values v (any shape that fits) -> uint8 RGB of `shape` + (3,)"""
    return np.ascontiguousarray(np.repeat(np.asarray(v, np.uint8).reshape(shape)[..., None], 3, axis=-1))


@functools.lru_cache(maxsize=None)
def cube_frames():
    """the 2^24 triples, [256,256,256,3]: frame = R, row = G, column = B; 256 different (mn, mx)"""
    r = np.arange(256, dtype=np.uint8)
    cube = np.ascontiguousarray(np.stack(np.broadcast_arrays(r[:, None, None], r[None, :, None], r[None, None, :]), -1))
    cube.setflags(write=False)
    return cube


def cube_one_frame():
    """the same bytes as one 4096 x 4096 frame: 128 passes of k_cond_minmax's stride loop, mn = 0, mx = 1.0"""
    return cube_frames().reshape(1, 4096, 4096, 3)


FLAT_SHAPE = (5, 7)


def flat():
    """[3,5,7,3]: all black (0/0), all white and constant (9, 9, 9) (zero contrast): each conditions to all zeros"""
    return np.stack([_grey(np.full(FLAT_SHAPE, v), FLAT_SHAPE) for v in (0, 255, 9)])


def one_lit():
    """[2,5,7,3]: black with one (1, 0, 0) pixel (mx is the smallest positive luma), black with one white pixel"""
    out = np.zeros((2,) + FLAT_SHAPE + (3,), np.uint8)
    out[0, 2, 3] = (1, 0, 0)
    out[1, 4, 6] = 255
    return out


RAMP_SHAPE = (24, 37)                  # 888 pixels: four blocks, the last one partly filled; every ramp fits more than three times
RAMPS_FIXED = ((0, 132), (0, 160), (1, 9), (17, 18), (254, 255))


def grey_ramp(lo, hi):
    """[24,37,3]: the grey values lo..hi, repeated to fill the frame"""
    return _grey(np.resize(np.arange(lo, hi + 1), RAMP_SHAPE), RAMP_SHAPE)


def _ramp_fixups(grey_luma, lo, hi):
    _, d, i = numpy_hist_model(grey_luma[lo:hi + 1])
    return d, i


@functools.lru_cache(maxsize=None)
def searched_ramps():
    """-> (five ranges whose ramp fires hist_bin's decrement, five whose ramp fires its increment): the grey ranges [lo, hi] are walked
    in order (lo ascending, then hi), a range counts for the first step it fires that still wants one, and each lo gives at most one
    range per step, so that the ten ranges have different (mn, mx) and are not all anchored at mn = 0.  The fixed ranges are left out."""
    g = np.arange(256, dtype=np.uint8)
    grey_luma = luma(np.stack([g, g, g], -1))
    dec, inc = [], []
    for lo in range(255):
        want_d, want_i = len(dec) < 5, len(inc) < 5
        for hi in range(lo + 1, 256):
            if not (want_d or want_i):
                break
            if (lo, hi) in RAMPS_FIXED:
                continue
            d, i = _ramp_fixups(grey_luma, lo, hi)
            if d and want_d:
                dec.append((lo, hi))
                want_d = False
            elif i and want_i:
                inc.append((lo, hi))
                want_i = False
    assert len(dec) == 5 and len(inc) == 5
    return tuple(dec), tuple(inc)


def ramp_ranges():
    """the fixed ranges, then the searched ones"""
    dec, inc = searched_ramps()
    return RAMPS_FIXED + dec + inc


def ramps():
    """[15,24,37,3]: every grey_ramp of ramp_ranges(), as one call"""
    return np.stack([grey_ramp(lo, hi) for lo, hi in ramp_ranges()])


PLANTED_SHAPES = {131072: (256, 512), 131073: (1, 131073), 262145: (1, 262145)}
_PLANTED_AT = (0, 63, 64, 255, 256, 131071, 131072)
PLANTED_BASE, PLANTED_MIN, PLANTED_MAX = 100, 7, 250


def planted_positions(npx):
    """a wave's last lane and the next wave's first (63, 64), a block's last thread and the next block's first (255, 256), the last pixel
    of the 512-block grid's first pass and the first of its second (131071, 131072), and the frame's last pixel"""
    return sorted({p for p in _PLANTED_AT + (npx - 1,) if p < npx})


def planted(npx, at_min, at_max):
    """[H,W,3] of npx pixels: every pixel (100, 100, 100), one (7, 7, 7) at flat index at_min, one (250, 250, 250) at at_max"""
    assert at_min != at_max
    v = np.full(npx, PLANTED_BASE, np.uint8)
    v[at_min], v[at_max] = PLANTED_MIN, PLANTED_MAX
    return _grey(v, PLANTED_SHAPES[npx])


def planted_pairs(npx):
    pos = planted_positions(npx)
    return [(a, b) for a in pos for b in pos if a != b]


def planted_call(npx):
    """every ordered pair of different positions, one frame each, as one call"""
    return np.stack([planted(npx, a, b) for a, b in planted_pairs(npx)])


SIZES_SHAPES = tuple((1, n) for n in (1, 63, 64, 65, 255, 256, 257, 1021)) + ((1021, 1),)
SIZES_REVERSED = (1, 257)              # the N = 5 call that is repeated with its frames in reverse order


def sizes_calls():
    """{name: [N,H,W,3]} of seeded random frames: N = 1 and N = 5 (other frames) of every shape, and two frames of 1 x 1021.  A call's
    N * H * W pixels are what k_echo_f16 sees: their tails past a multiple of four are 1 and 3 for the odd shapes whatever the N, so
    the pair of 1 x 1021 frames (2042 pixels) is here for the tail of two."""
    out = {}
    for k, (H, W) in enumerate(SIZES_SHAPES):
        for N in (1, 5):
            out[f"{N}x{H}x{W}"] = np.random.default_rng(1000 + 10 * k + N).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    out["2x1x1021"] = np.random.default_rng(2000).integers(0, 256, (2, 1, 1021, 3), dtype=np.uint8)
    return out


def corpus_calls(cube=True):
    """{name: [N,H,W,3]}: every call of the corpus (the two cube forms only with `cube`)"""
    out = {"flat": flat(), "one_lit": one_lit(), "ramps": ramps()}
    for npx in PLANTED_SHAPES:
        out[f"planted_{npx}"] = planted_call(npx)
    out.update({"sizes_" + k: v for k, v in sizes_calls().items()})
    if cube:
        out["cube_frames"] = cube_frames()
        out["cube_one_frame"] = cube_one_frame()
    return out


def two_valued():
    """[2,8,8,3]: black with a 2-row band of 200; Otsu's threshold is the centre of bin 0"""
    f = np.zeros((2, 8, 8, 3), np.uint8)
    f[:, 2:4] = 200
    return f


TWO_VALUED_THRESHOLD = 0.001531862745098039


def study(H, W, seed=77):
    """[6,H,W,3]: speckle, black, speckle, constant (9, 9, 9), black with one lit pixel, speckle (independent noise per channel)"""
    from tee_optical_flow_amd.synth import speckle_sequence
    rng = np.random.default_rng(seed)
    g = speckle_sequence(seed, 6, H, W).astype(np.int16)
    rgb = np.empty((6, H, W, 3), np.uint8)
    for c in range(3):
        rgb[..., c] = np.clip(g + rng.integers(-12, 13, g.shape, dtype=np.int16), 0, 255)
    rgb[1] = 0
    rgb[3] = 9
    rgb[4] = 0
    rgb[4, H // 2, W // 3] = (40, 200, 90)
    return rgb
