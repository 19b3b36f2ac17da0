#!/opt/conda/bin/python3.9
"""Generates tests/golden/reference_area_series.npz by RUNNING the reference's own AreaDetector.detect
(/root/reference/optical_flow/cardiac_cycle_detection.py:146-179, its per-frame loop :159-172: skimage.measure.label, regionprops,
props[0].area) on an OpticalFlowDataset (optical_flow_dataset.py) that opened a real HDF5 file in the study layout.

Run (build container only; the reference never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tests/golden/make_reference_area_fixtures.py

That interpreter has skimage 0.18.3, scipy 1.7, h5py and numpy 1.26; cv2, imageio, peakutils, polars, tsmoothie and neurokit2 are
MagicMock stubs so the modules import.  One stand-in carries behaviour: cardiac_cycle_detection.SpectralSmoother is replaced with a
recorder whose smooth(x) keeps list(x) and raises a private exception, which this script catches: the list the detector hands to its
smoother is its area_list, and nothing after the smoother (baseline, peaks, intervals) runs.
Stored, as data:
  `mask`     uint8 [16,70,150,2]: the study's one label, channel 1 different from channel 0 (the detector reads channel 0 only)
  `nframes`  attrs['nframes'] - 2 = 14
  `area`     int64 [14]: the detector's area_list
  `case/*`   which frame carries which case, for the tests to check that they are there.
"""
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np

for m in ["cv2", "pydicom", "torch", "torchvision", "torchvision.transforms", "peakutils", "peakutils.peak", "polars", "tsmoothie",
          "tsmoothie.smoother", "neurokit2", "models", "models.sam", "imageio", "imageio.v2"]:
    sys.modules[m] = MagicMock()
sys.path.insert(0, "/root/reference")
sys.path.insert(0, "/root/reference/optical_flow")          # the reference imports optical_flow_dataset as a top-level module
import h5py  # noqa: E402
import optical_flow.cardiac_cycle_detection as CCD  # noqa: E402
from optical_flow_dataset import OpticalFlowDataset  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
N, H, W = 16, 70, 150                                       # 64 x 16 tiles: 3 tile columns, 5 tile rows, ragged both ways
LABEL = "rv"
yy, xx = np.mgrid[:H, :W]


class _Recorded(Exception):
    pass


class RecordingSmoother:
    received = []

    def __init__(self, *a, **k):
        pass

    def smooth(self, data):
        RecordingSmoother.received.append(list(data))
        raise _Recorded()


CCD.SpectralSmoother = RecordingSmoother


def blob(f):
    cy, cx = 40 + (f % 5) - 2, 30 + 6 * f
    return ((yy - cy) / 9.0) ** 2 + ((xx - cx) / 12.0) ** 2 < 1.0          # 327 px at frame 2


m0 = np.zeros((N, H, W), np.uint8)
for f in range(N):
    m0[f][blob(f)] = 1
case = {}
case["empty"] = np.array([0, 1])                            # both give 0: nothing to carry yet
m0[0] = 0
m0[1] = 0
case["blob"] = np.array([2])
case["lone_pixel"] = np.array([3])                          # (2, 2) comes first in raster order: area 1, not the blob's
m0[3, 2, 2] = 1
case["carry"] = np.array([5])                               # empty in the middle: frame 4's area again
m0[5] = 0
# two 11 x 14 blocks that touch only at the tile corner (15, 63) / (16, 64), the seed in the upper one: 308 px; a larger block later on
case["diagonal"] = np.array([6])
m0[6] = 0
m0[6, 5:16, 50:64] = 1
m0[6, 16:27, 64:78] = 1
m0[6, 45:65, 100:130] = 1
# a 20 x 20 checkerboard across tile edges: one region of 200 px; a larger block later on
case["checker"] = np.array([7])
m0[7] = 0
m0[7][((yy + xx) % 2 == 0) & (yy >= 8) & (yy < 28) & (xx >= 54) & (xx < 74)] = 1
m0[7, 45:65, 100:130] = 1
# a 10 x 12 block of value 2 touching a 10 x 30 block of value 1, the seed in the value-2 block: only that block counts (120)
case["two_values"] = np.array([8])
m0[8] = 0
m0[8, 10:20, 58:70] = 2
m0[8, 10:20, 70:100] = 1
m0[8, 20:24, 58:70] = 1
# frame 2's blob drawn with value 255
case["value_255"] = np.array([9])
m0[9] = 0
m0[9][blob(2)] = 255
# a region on the image border (the corner), and one in the opposite corner
case["border"] = np.array([10])
m0[10] = 0
m0[10, 0:10, 0:12] = 1
m0[10, 55:70, 130:150] = 1
case["full"] = np.array([11])
m0[11] = 1
mask = np.stack([m0, (m0 == 0).astype(np.uint8)], axis=-1)

with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "study.hdf5")
    with h5py.File(path, "w") as fh:
        fh.create_dataset("echo", data=np.zeros((N, H, W), np.float16))
        d = fh.create_dataset("flow", data=np.zeros((N, H, W, 2), np.float16))
        d.attrs["frame_rate"] = 29.97
        d.attrs["nframes"] = N
        d.attrs["pixel_spacing"] = 0.05
        d.attrs["ID"] = "study"
        d.attrs["HR"] = 0
        d.attrs["no_saliency"] = True
        d.attrs["mode"] = "RVIO_2class"
        d.attrs["units_converted"] = True
        d.attrs["waveforms_present"] = False
        fh.create_dataset(LABEL, data=mask)
        d.attrs["labels"] = [LABEL]
    ds = OpticalFlowDataset(path)
    assert ds.nframes == N - 2 and ds.get_mask(LABEL).dtype == np.uint8
    try:
        CCD.create_detector("area").detect(ds, label=LABEL)
    except _Recorded:
        pass
    assert len(RecordingSmoother.received) == 1 and len(RecordingSmoother.received[0]) == ds.nframes
    out = {"mask": ds.get_mask(LABEL), "nframes": np.int64(ds.nframes), "area": np.asarray(RecordingSmoother.received[0], np.int64)}
    ds.close()
a = out["area"]
assert a[0] == 0 and a[1] == 0 and a[3] == 1 and a[5] == a[4] and a[6] == 308 and a[7] == 200 and a[8] == 120 and a[9] == a[2] \
    and a[10] == 120 and a[11] == H * W, a
for k, v in case.items():
    out[f"case/{k}"] = v
np.savez_compressed(os.path.join(OUT, "reference_area_series.npz"), **out)
print(a.tolist())
