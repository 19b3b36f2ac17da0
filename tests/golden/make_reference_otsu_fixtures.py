#!/opt/conda/bin/python3.9
"""Generates tests/golden/reference_otsu.npz by IMPORTING the reference's own predict_movie_thres
(/root/reference/optical_flow/calculate_optical_flow.py:184-213: skimage's rgb2gray, threshold_otsu and remove_small_objects,
scipy's binary_fill_holes, the reference's moving_avg_mask) in THIS container and recording what it returns.

Run (build container only; the reference never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tests/golden/make_reference_otsu_fixtures.py

cv2, pydicom, torch, ... are MagicMock stubs, as in make_reference_clean_mask_fixtures.py.  Each case stores its frames
(`<case>/in`, uint8 [N,H,W,3]; or `<case>/in_of`, the name of the case whose frames it shares), min_mask_size (`<case>/min_size`),
channel 0 of the returned bool [N,H,W,2] mask (`<case>/otsu`, uint8; the generator checks that both channels are equal) and, per
frame, skimage.filters.threshold_otsu(skimage.color.rgb2gray(frame)) (`<case>/thr`, float64 [N]).  Fixtures are DATA (inputs +
outputs); no reference source text is stored.

Every case is also computed with a plain-order luma, ((r/255)*0.2125 + (g/255)*0.7154) + (b/255)*0.0721 in float64 -- what the
device kernel evaluates -- in place of skimage's `rgb @ coeffs`, and a case is recorded only if masks and thresholds are identical:
the golden file must not bake in a BLAS that fuses the multiply and the add.  The BLAS of this container's
numpy does fuse: about one luma value in ten differs by an ulp, and where that moves a frame's minimum or maximum, the bin edges and
the threshold move by an ulp with it.  Such a seed is reported on the console and the next one is taken (`<case>/seed` records the one
used); no case is recorded on which the two orders disagree, and none is left out of the check.
"""
import os
import sys
from dataclasses import replace
from unittest.mock import MagicMock

import numpy as np

for m in ["cv2", "pydicom", "torch", "torchvision", "torchvision.transforms", "peakutils", "polars", "tsmoothie",
          "tsmoothie.smoother", "neurokit2", "models", "models.sam", "imageio.v2"]:
    sys.modules[m] = MagicMock()
sys.modules["cv2"].cuda.getCudaEnabledDeviceCount.return_value = 0
sys.path.insert(0, "/root/reference")
import optical_flow.calculate_optical_flow as R  # noqa: E402
from optical_flow.config import default_optical_flow_config  # noqa: E402
from scipy.ndimage import binary_fill_holes  # noqa: E402
from skimage.color import rgb2gray  # noqa: E402
from skimage.filters import threshold_otsu  # noqa: E402
from skimage.morphology import remove_small_objects  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
arrs = {}
inputs = {}


def plain_luma(frame):
    a = frame.astype(np.float64) / 255.0
    return (a[..., 0] * 0.2125 + a[..., 1] * 0.7154) + a[..., 2] * 0.0721


def record(name, build, min_size, in_of=None, seed0=None):
    """`build(rng)` makes the frames.  A seed whose frames the plain-order twin does not reproduce bit for bit (this container's BLAS
    fuses, which moves about one luma value in ten by an ulp, and with a frame's minimum or maximum its bin edges) is reported and
    the next one is taken: the recorded case is one on which both orders agree, and it says which seed that was."""
    if in_of is not None:
        assert attempt(name, inputs[in_of], min_size, in_of), f"{name}: the plain-order luma disagrees on shared frames"
        return
    for seed in range(seed0, seed0 + 200):
        if attempt(name, build(np.random.default_rng(seed)), min_size, None):
            arrs[f"{name}/seed"] = np.array(seed, dtype=np.int64)
            return
        print(f"{name}: seed {seed}: the plain-order luma and skimage's rgb @ coeffs disagree here; next seed")
    raise AssertionError(f"{name}: no agreeing seed")


def attempt(name, frames, min_size, in_of):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    assert frames.ndim == 4 and frames.shape[3] == 3 and min(frames.shape[:3]) >= 2
    cfg = replace(default_optical_flow_config(), min_mask_size=min_size)
    res = R.predict_movie_thres(frames, verbose=False, config=cfg)
    assert list(res) == ["otsu"]
    v = res["otsu"]
    assert v.dtype == bool and v.shape == frames.shape[:3] + (2,) and np.array_equal(v[..., 0], v[..., 1])
    thr = np.array([threshold_otsu(rgb2gray(f)) for f in frames], dtype=np.float64)
    # the plain-order twin: every case, none left out
    t_thr, t_masks = [], []
    for f in frames:
        g = plain_luma(f)
        t = threshold_otsu(g)
        t_thr.append(t)
        t_masks.append(remove_small_objects(binary_fill_holes(g > t), min_size=min_size))
    t_out = R.moving_avg_mask(np.squeeze(np.stack(t_masks)))
    if not (np.array_equal(np.array(t_thr, dtype=np.float64), thr) and np.array_equal(t_out, v[..., 0])):
        return False
    if in_of is None:
        arrs[f"{name}/in"] = frames
        inputs[name] = frames
    else:
        assert np.array_equal(inputs[in_of], frames)
        arrs[f"{name}/in_of"] = np.array(in_of)
    arrs[f"{name}/min_size"] = np.array(min_size, dtype=np.int64)
    arrs[f"{name}/otsu"] = v[..., 0].astype(np.uint8)
    arrs[f"{name}/thr"] = thr
    print(f"{name}: {frames.shape}, min_size {min_size}, foreground per frame {v[..., 0].sum(axis=(1, 2)).tolist()}")
    return True


def blobs(rng, N, H, W, n_blobs=4, noise=14.0, rgb=False, drift=1.5):
    """bright blobs, some with a dark core, drifting over a dim background; Gaussian noise (per channel when `rgb`)"""
    yy, xx = np.mgrid[:H, :W]
    shapes = [(rng.uniform(0, H), rng.uniform(0, W), rng.uniform(4, H / 3), rng.uniform(4, W / 3), rng.uniform(-drift, drift, 2),
               rng.uniform(90, 230), rng.integers(0, 2)) for _ in range(n_blobs)]
    out = np.zeros((N, H, W, 3), np.uint8)
    tint = rng.uniform(0.6, 1.0, 3) if rgb else np.ones(3)
    for f in range(N):
        img = np.full((H, W), 25.0)
        for cy, cx, ry, rx, v, amp, core in shapes:
            d = ((yy - cy - v[0] * f) / ry) ** 2 + ((xx - cx - v[1] * f) / rx) ** 2
            img = np.maximum(img, amp * np.exp(-d))
            if core:
                img[d < 0.06] = 20.0
        for c in range(3):
            n = rng.normal(0, noise, (H, W)) if (rgb or c == 0) else n
            out[f, :, :, c] = np.clip(img * tint[c] + n, 0, 255).astype(np.uint8)
    return out


def sector(rng, N, H, W):
    """an ultrasound-style sector of speckle on a zero background, with dark chambers (holes) that move"""
    yy, xx = np.mgrid[:H, :W]
    r = np.hypot(yy + 4.0, xx - W / 2.0)
    ang = np.arctan2(xx - W / 2.0, yy + 4.0)
    inside = (r < H * 0.98) & (r > 8) & (np.abs(ang) < 0.72)
    out = np.zeros((N, H, W, 3), np.uint8)
    for f in range(N):
        speckle = rng.rayleigh(55.0, (H, W))
        tissue = 0.35 + 0.65 * ((np.sin(yy / 9.0 + 0.3 * f) * np.cos(xx / 11.0) > -0.2))
        img = speckle * tissue
        for cy, cx, rad in ((H * 0.45, W * 0.42 + f, H / 7.0), (H * 0.7, W * 0.6 - f, H / 9.0)):
            img[np.hypot(yy - cy, xx - cx) < rad] *= 0.08
        g = np.clip(np.where(inside, img, 0.0), 0, 255).astype(np.uint8)
        out[f] = g[:, :, None]
    return out


record("grey_6x64x80_min500", lambda rng: blobs(rng, 6, 64, 80), 500, seed0=100)
record("rgb_noise_6x61x83_min500", lambda rng: blobs(rng, 6, 61, 83, rgb=True, noise=22.0), 500, seed0=200)
record("sector_8x97x131_min500", lambda rng: sector(rng, 8, 97, 131), 500, seed0=300)
record("odd_6x41x67_min30", lambda rng: blobs(rng, 6, 41, 67, rgb=True), 30, seed0=400)       # not multiples of the device's 64 x 16 tile
record("odd_4x17x65_min5", lambda rng: blobs(rng, 4, 17, 65, n_blobs=2), 5, seed0=500)


def constant_frame(rng):
    """one constant frame in the stack (threshold_otsu's early return: the frame's mask is empty)"""
    st = blobs(rng, 5, 40, 48, noise=30.0)
    st[2] = 77
    return st


def constant_rgb_ends(rng):
    """constant frames at both ends of the stack, one of them not grey"""
    st = blobs(rng, 4, 40, 48, rgb=True, noise=30.0)
    st[0] = (10, 200, 31)
    st[3] = 0
    return st


def two_valued(rng):
    """a two-valued frame (two occupied bins: the first and the last), and one whose two values are neighbours"""
    st = blobs(rng, 5, 40, 48, noise=30.0)
    two = np.full((40, 48), 30, np.uint8)
    two[8:30, 10:40] = 200
    two[14:20, 18:26] = 30                            # a hole
    two[35:37, 2:4] = 200                             # a small object
    st[1] = two[:, :, None]
    st[4] = np.where((np.mgrid[:40, :48].sum(0) % 7 < 3)[:, :, None], (255, 255, 255), (254, 255, 255)).astype(np.uint8)
    return st


record("constant_frame_5x40x48_min20", constant_frame, 20, seed0=600)
record("constant_rgb_ends_4x40x48_min0", constant_rgb_ends, 0, seed0=700)
record("two_valued_5x40x48_min10", two_valued, 10, seed0=800)

record("minsize_6x40x56_min0", lambda rng: blobs(rng, 6, 40, 56, rgb=True, noise=35.0, n_blobs=5), 0, seed0=900)
for ms in (1, 500, 40 * 56 + 1):
    record(f"minsize_6x40x56_min{ms}", None, ms, in_of="minsize_6x40x56_min0")

record("n2_2x45x52_min20", lambda rng: blobs(rng, 2, 45, 52, noise=30.0, drift=6.0), 20, seed0=1000)      # the window's clamps
record("n3_3x45x52_min20", lambda rng: blobs(rng, 3, 45, 52, rgb=True, noise=30.0, drift=6.0), 20, seed0=1100)

path = os.path.join(OUT, "reference_otsu.npz")
np.savez_compressed(path, **arrs)
print(f"{len([k for k in arrs if k.endswith('/otsu')])} cases written, {os.path.getsize(path)} bytes")
