#!/opt/conda/bin/python3.9
"""Generates tests/golden/reference_clean_mask.npz by IMPORTING the reference's own clean_mask
(/root/reference/optical_flow/calculate_optical_flow.py:90-111 moving_avg_mask, :113-182 clean_mask; skimage's
remove_small_objects and scipy's binary_fill_holes) in THIS container and recording what it returns.

Run (build container only; the reference never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tests/golden/make_reference_clean_mask_fixtures.py

cv2, pydicom, torch, ... are MagicMock stubs, as in make_reference_host_fixtures.py.  Each case stores its class map
(`<case>/in`, uint8 [N,H,W]), mode and min_mask_size (`<case>/mode`, `<case>/min_size`), the key order the reference
returned (`<case>/keys`) and, per key, channel 0 of the bool [N,H,W,2] mask (`<case>/<key>`, uint8; the generator checks
that both channels are equal).  Fixtures are DATA (inputs + outputs); no reference source text is stored.
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

OUT = os.path.dirname(os.path.abspath(__file__))
arrs = {}


def record(name, arr, mode, min_size):
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    res = R.clean_mask(arr, mode=mode, verbose=False, config=replace(default_optical_flow_config(), min_mask_size=min_size))
    arrs[f"{name}/in"] = arr
    arrs[f"{name}/mode"] = np.array(mode)
    arrs[f"{name}/min_size"] = np.array(min_size, dtype=np.int64)
    arrs[f"{name}/keys"] = np.array(list(res))
    for k, v in res.items():
        assert v.dtype == bool and v.shape == arr.shape + (2,) and np.array_equal(v[..., 0], v[..., 1])
        arrs[f"{name}/{k}"] = v[..., 0].astype(np.uint8)


def blobs(rng, N, H, W, n_cls, n_blobs, drift=2):
    """class map of random rectangles and discs that drift a little from frame to frame (and some salt noise)"""
    yy, xx = np.mgrid[:H, :W]
    shapes = []
    for _ in range(n_blobs):
        shapes.append((int(rng.integers(1, n_cls + 1)), int(rng.integers(0, 2)), rng.uniform(-5, H + 5), rng.uniform(-5, W + 5),
                       rng.uniform(2, max(3, H / 3)), rng.uniform(2, max(3, W / 3)), rng.uniform(-drift, drift, 2)))
    out = np.zeros((N, H, W), np.uint8)
    for f in range(N):
        m = out[f]
        for c, kind, cy, cx, ry, rx, v in shapes:
            cy, cx = cy + v[0] * f, cx + v[1] * f
            if kind == 0:
                sel = (np.abs(yy - cy) < ry) & (np.abs(xx - cx) < rx)
            else:
                sel = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
            m[sel] = c
            hole = ((yy - cy) / (ry / 3 + 1)) ** 2 + ((xx - cx) / (rx / 3 + 1)) ** 2 < 1.0    # a hole in most shapes
            if kind == 1:
                m[hole] = 0
        salt = rng.random((H, W)) < 0.01
        m[salt] = rng.integers(0, n_cls + 1, int(salt.sum()))
    return out


rng = np.random.default_rng(2026)
# random studies, sizes that are not tile multiples (64 x 16 tiles on the device)
for ms in (500, 5):
    record(f"rvio_9x37x53_min{ms}", blobs(rng, 9, 37, 53, 2, 6), "RVIO_2class", ms)
    record(f"a4c_5x129x257_min{ms}", blobs(rng, 5, 129, 257, 8, 24), "A4C", ms)
record("mouse_7x70x90_min30", blobs(rng, 7, 70, 90, 2, 8), "MouseRV_A4C", 30)
record("a4c_12x48x80_min0", blobs(rng, 12, 48, 80, 8, 14, drift=6), "A4C", 0)
record("rvio_4x33x65_uniform_min40", rng.integers(0, 3, (4, 33, 65)), "RVIO_2class", 40)


def still(frame, n=3):
    return np.repeat(np.asarray(frame, np.uint8)[None], n, axis=0)


H, W = 150, 170
# a spiral foreground line (2 px wide, 2 px gaps) crossing every tile
sp = np.zeros((H, W), np.uint8)
top, left, bot, right = 1, 1, H - 2, W - 2
while top + 1 < bot and left + 1 < right:
    sp[top:top + 2, left:right + 1] = 1
    sp[top:bot + 1, right - 1:right + 1] = 1
    sp[bot - 1:bot + 1, left + 4:right + 1] = 1
    sp[top + 4:bot + 1, left + 4:left + 6] = 1
    top, left, bot, right = top + 4, left + 4, bot - 4, right - 4
record("hard_spiral_min500", still(sp), "RVIO_2class", 500)
record("hard_spiral_min5", still(sp), "RVIO_2class", 5)

# a serpentine background channel (1 px) through a full foreground, reaching the border only at its one end: NOT filled;
# plus an enclosed background pocket: filled
sv = np.ones((H, W), np.uint8)
for k, r in enumerate(range(3, H - 3, 4)):
    sv[r, 3:W - 3] = 0
    c = W - 4 if k % 2 == 0 else 3
    if r + 4 < H - 3:
        sv[r:r + 5, c] = 0
sv[3, 0:4] = 0                                   # the channel's only way out
sv[H - 2, 40:60] = 0                             # enclosed (row H-2 is not a border row)
record("hard_serpentine_min500", still(sv), "RVIO_2class", 500)

# holes open to the outside only diagonally: filled under 4-connectivity
dg = np.zeros((H, W), np.uint8)
for (y0, x0) in ((10, 10), (60, 90), (100, 20)):
    dg[y0:y0 + 30, x0:x0 + 30] = 1
    dg[y0 + 1:y0 + 29, x0 + 1:x0 + 29] = 0
    dg[y0, x0] = 0                               # corner knocked out: the inside meets it only diagonally
dg[0:12, 140:152] = 1
dg[1:11, 141:151] = 0
dg[0, 141:151] = 0                               # a ring on the top border, opened ON the border row: not filled
record("hard_diagonal_min5", still(dg), "RVIO_2class", 5)
record("hard_diagonal_min500", still(dg), "RVIO_2class", 500)

# two squares touching only at a corner (100 px each; 200 together under 8-connectivity): removed at min_size 150;
# components of exactly min_size (500) and min_size - 1 (499)
ct = np.zeros((H, W), np.uint8)
ct[10:20, 10:20] = 1
ct[20:30, 20:30] = 1
ct[50:70, 10:35] = 1                             # 500
ct[50:70, 60:85] = 1
ct[50, 60] = 0                                   # 499
ct[100:120, 100:125] = 2                         # 500 of the other label
ct[100:120, 130:155] = 2
ct[119, 154] = 0                                 # 499
record("hard_corner_min150", still(ct), "RVIO_2class", 150)
record("hard_exact_min500", still(ct), "RVIO_2class", 500)

# checkerboards (1 px and 3 px squares)
yy, xx = np.mgrid[:H, :W]
record("hard_checker1_min5", still(((yy + xx) % 2).astype(np.uint8)), "RVIO_2class", 5)
record("hard_checker3_min5", still((((yy // 3) + (xx // 3)) % 2 + 1).astype(np.uint8)), "RVIO_2class", 5)

# frames entirely empty or entirely one class, changing over time (the moving average at work)
seq = np.zeros((8, 37, 53), np.uint8)
seq[2:5] = 1
seq[5] = 2
seq[7] = 1
record("hard_empty_full_min500", seq, "RVIO_2class", 500)
record("hard_all_one_a4c_min500", np.full((4, 37, 53), 3, np.uint8), "A4C", 500)

# a foreground cross touching all four borders; background quadrants touch the borders (kept), an enclosed pocket (filled)
cr = np.zeros((H, W), np.uint8)
cr[60:90, :] = 1
cr[:, 70:100] = 1
cr[70:80, 80:90] = 0
cr[0:H, 0] = 2                                   # the other label along the whole left and bottom borders
cr[H - 1, 0:W] = 2
record("hard_borders_min5", still(cr), "RVIO_2class", 5)
record("hard_borders_min500", still(cr), "RVIO_2class", 500)

np.savez_compressed(os.path.join(OUT, "reference_clean_mask.npz"), **arrs)
print(f"{len([k for k in arrs if k.endswith('/in')])} cases written")
