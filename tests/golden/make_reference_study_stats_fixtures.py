#!/opt/conda/bin/python3.9
"""Generates tests/golden/reference_study_stats.npz by RUNNING the reference's own consumer step on a study file:
calc_AV_centroid and calculate_3dhist_radlong(ds, param) (/root/reference/optical_flow/analyze_optical_flow.py:202-244, 320-343)
on an OpticalFlowDataset (optical_flow_dataset.py) that opened a real HDF5 file in the study layout.

Run (build container only; the reference never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tests/golden/make_reference_study_stats_fixtures.py

That interpreter has skimage, scipy 1.7, h5py and numpy 1.26; cv2, imageio, peakutils, polars, tsmoothie and neurokit2 are
MagicMock stubs so the modules import.  Stored, as data: the study's inputs (`flow` float16 [N,H,W,2] as the file holds it,
`rv` / `av` bool [N,H,W,2], `frame_rate`, `nframes` = attrs['nframes'] - 2) and the reference's outputs:
  `cent_nofilter`  calc_AV_centroid(av, nframes, filter=False)                 float64 [nframes, 2]
  `cent_sg9`       calc_AV_centroid(av, nframes, savgol_window=9)              (scipy 1.7 refuses the default even window of 10)
  `<param>/<radial|longitudinal>/<freq|edges|hi|lo>`  calculate_3dhist_radlong(ds, param, av_filter_flag=False)
  `case/*`         which frames carry the labelling cases (empty frames, a tie in area, a diagonal join across a tile corner,
                   a checkerboard), for the tests to check that they are there.
The file's frame_rate is an h5py np.float64; numpy 1.26 divides np.gradient's float32 field by it in float32.  Numpy 2 (NEP 50)
would divide in float64, so a test that compares acceleration or PWR with this fixture passes frame_rate as a Python float, which
divides in float32 under both.
"""
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np

for m in ["cv2", "pydicom", "torch", "torchvision", "torchvision.transforms", "peakutils", "polars", "tsmoothie",
          "tsmoothie.smoother", "neurokit2", "models", "models.sam", "imageio", "imageio.v2"]:
    sys.modules[m] = MagicMock()
sys.path.insert(0, "/root/reference")
sys.path.insert(0, "/root/reference/optical_flow")          # analyze_optical_flow imports optical_flow_dataset as a top-level module
import h5py  # noqa: E402
import optical_flow.analyze_optical_flow as A  # noqa: E402
from optical_flow_dataset import OpticalFlowDataset  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
N, H, W = 14, 70, 150                                       # 64 x 16 tiles: 3 tile columns, 5 tile rows, ragged both ways
FRAME_RATE = 29.97
rng = np.random.default_rng(20261016)
yy, xx = np.mgrid[:H, :W]

# flow: quantised speckle (compresses), a few exact zeros
flow = (np.round(rng.normal(0, 3, (N, H, W, 2)) * 4) / 4).astype(np.float16)
flow[:, 30:34, 100:110, :] = 0

# rv: a drifting ellipse
rv = np.zeros((N, H, W), bool)
for f in range(N):
    rv[f] = ((yy - 35 - 0.7 * f) / 24.0) ** 2 + ((xx - 70 + 1.5 * f) / 55.0) ** 2 < 1.0

# av: one labelling case per frame
av = np.zeros((N, H, W), bool)
case = {}
for f in range(N):
    cy, cx = 40 + (f % 5) - 2, 30 + 6 * f
    av[f] = ((yy - cy) / 9.0) ** 2 + ((xx - cx) / 12.0) ** 2 < 1.0          # a plain blob (about 340 px)
    av[f, 2, 2] = True                                                     # and a stray pixel
case["empty"] = np.array([0, 7])
av[0] = False
av[7] = False
# tie: two 10 x 10 squares of equal area, the larger ones; the first in raster order (the upper one, further right) wins
case["tie"] = np.array([3])
av[3] = False
av[3, 50:60, 100:110] = True
av[3, 20:30, 130:140] = True
av[3, 5:8, 5:8] = True
# diagonal: two 11 x 14 blocks that touch only at the tile corner (15, 63) / (16, 64): one component of 308 px under 8-connectivity,
# two of 154 under 4-connectivity, where a 200 px block would win instead
case["diagonal"] = np.array([5])
av[5] = False
av[5, 5:16, 50:64] = True
av[5, 16:27, 64:78] = True
av[5, 45:55, 110:130] = True
# checkerboard: a 20 x 20 board across tile edges is one 200 px component under 8-connectivity (many single pixels under 4);
# a 150 px block would win under 4-connectivity
case["checker"] = np.array([9])
av[9] = False
board = ((yy + xx) % 2 == 0) & (yy >= 8) & (yy < 28) & (xx >= 54) & (xx < 74)
av[9] |= board
av[9, 45:55, 110:125] = True
# one-pixel staircases (8-connected only): a 30 px one at slope 1/2 and a 38 px diagonal through the tile corner (15, 127) / (16, 128)
case["staircase"] = np.array([11])
av[11] = False
for k in range(30):
    av[11, 5 + k // 2, 10 + k] = True
for k in range(38):
    av[11, k, 112 + k] = True

nframes_attr = N
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "study.hdf5")
    with h5py.File(path, "w") as fh:
        fh.create_dataset("echo", data=np.zeros((N, H, W), np.float16))
        d = fh.create_dataset("flow", data=flow)
        d.attrs["frame_rate"] = FRAME_RATE
        d.attrs["nframes"] = nframes_attr
        d.attrs["pixel_spacing"] = 0.05
        d.attrs["ID"] = "study"
        d.attrs["HR"] = 0
        d.attrs["no_saliency"] = True
        d.attrs["mode"] = "RVIO_2class"
        d.attrs["units_converted"] = True
        d.attrs["waveforms_present"] = False
        fh.create_dataset("rv", data=np.stack([rv, rv], axis=-1))
        fh.create_dataset("av", data=np.stack([av, av], axis=-1))
        d.attrs["labels"] = ["rv", "av"]
    ds = OpticalFlowDataset(path)
    assert ds.nframes == N - 2 and isinstance(ds.frame_rate, np.float64) and ds.accel_array.dtype == np.float32
    out = {"flow": flow, "rv": ds.get_mask("rv"), "av": ds.get_mask("av"), "frame_rate": np.float64(ds.frame_rate),
           "nframes": np.int64(ds.nframes)}
    out["cent_nofilter"] = np.asarray(A.calc_AV_centroid(ds.get_mask("av"), ds.nframes, filter=False), np.float64)
    out["cent_sg9"] = np.asarray(A.calc_AV_centroid(ds.get_mask("av"), ds.nframes, filter=True, savgol_window=9, savgol_poly=4))
    for param in ("velocity", "acceleration", "PWR"):
        res = A.calculate_3dhist_radlong(ds, param, av_filter_flag=False)
        for comp in ("radial", "longitudinal"):
            freq, edges, hi, lo = res[comp]
            out[f"{param}/{comp}/freq"] = np.asarray(freq)
            out[f"{param}/{comp}/edges"] = np.asarray(edges)
            out[f"{param}/{comp}/hi"] = np.asarray(hi)
            out[f"{param}/{comp}/lo"] = np.asarray(lo)
    ds.close()
for k, v in case.items():
    out[f"case/{k}"] = v
np.savez_compressed(os.path.join(OUT, "reference_study_stats.npz"), **out)
print({k: (np.shape(v), np.asarray(v).dtype) for k, v in out.items() if not k.startswith("case/")})
