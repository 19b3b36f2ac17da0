#!/usr/bin/env python3
"""Generates tests/golden/reference_polar.npz by RUNNING the reference's own consumer steps on cv2.cartToPolar:
calculate_3dhist(ds, param, label) (optical_flow/analyze_optical_flow.py:909-966) and AngleDetector.detect's per-frame angle
mode (optical_flow/cardiac_cycle_detection.py:100-120, reached as sysdia_frames_by_angle), on the reference's own
OpticalFlowDataset, whose __init__ runs on a stand-in h5py file that holds the study's arrays.

Run with the interpreter the tests run (build container only; the reference never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_polar_fixtures.py
Made with numpy 2.2.6 and scipy 1.15.3.  Under numpy 2 np.histogram builds float32 bin edges for float32 data (linspace runs in
float32) and np.percentile of float32 data returns np.float32, with q / 100 and the virtual index in float32; numpy 1.x builds
float64 edges and computes the percentile in float64, so a numpy 1.x run gives other edges, other bins near the edges and
float64 percentiles.  The study's frame_rate is a np.float64, as h5py returns the attribute: under numpy 2 (NEP 50) np.gradient
divides the float32 field by it in float64.

Stand-ins: h5py, skimage, matplotlib, imageio, peakutils, polars, neurokit2, pydicom and torch(vision) are MagicMock stubs so the
modules import.  Two stand-ins carry behaviour:
  cv2.cartToPolar   is tee_optical_flow_amd.analysis.cart_to_polar, the project's restatement of OpenCV 4.x's CV_32F arithmetic
                    (AVX2 / NEON body).  It is the ONE piece of this fixture that is not the reference's own code: cv2 is not
                    installed where the fixture was made, and parity with cv2 stays unpinned.
  tsmoothie.smoother.SpectralSmoother  an identity smoother that records what smooth() receives: AngleDetector's ang_mode_arr.
Stored, as data:
  `stress/flow` float32 [N,H,W,2], `stress/<label>` bool [N,H,W,2], `stress/frame_rate`, `stress/nframes`: a synthetic study with
      angle stress (see below); the other study is the flow and masks of reference_study_stats.npz (`study`), read from that file.
  `<study>/<param>/<label>/<mag_freq|ang_freq|mag_edges|ang_edges|hi>`  calculate_3dhist(ds, param, label), or
      `<study>/<param>/<label>/raises` = 'IndexError' where the reference raises it (the study's 'av' label is empty on frame 0)
  `<study>/<param>/<label>/ang_mode`  the array AngleDetector.detect(ds, param, label) passed to its smoother
  `stress/case/*`  where the stress cases are, for the tests to check that they are there.
"""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tee_optical_flow_amd.analysis import cart_to_polar  # noqa: E402

for m in ["h5py", "skimage", "skimage.color", "skimage.morphology", "skimage.util", "skimage.transform", "skimage.measure",
          "skimage.feature", "matplotlib", "matplotlib.pyplot", "matplotlib.colors", "matplotlib.cm", "imageio", "imageio.v2",
          "peakutils", "polars", "neurokit2", "pydicom", "torch", "torchvision", "torchvision.transforms", "models", "models.sam"]:
    sys.modules[m] = MagicMock()
cv2 = MagicMock()
cv2.cartToPolar = lambda x, y: cart_to_polar(x, y)
sys.modules["cv2"] = cv2


class RecordingSmoother:
    received = []

    def __init__(self, *a, **k):
        pass

    def smooth(self, data):
        RecordingSmoother.received.append(np.array(data, copy=True))
        self.smooth_data = np.asarray(data)[None]


ts = types.ModuleType("tsmoothie")
ts.smoother = types.ModuleType("tsmoothie.smoother")
ts.smoother.SpectralSmoother = RecordingSmoother
sys.modules["tsmoothie"], sys.modules["tsmoothie.smoother"] = ts, ts.smoother

REF = os.environ.get("TEEFLOW_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "optical_flow"))
import h5py  # noqa: E402  (the stub)
import optical_flow.analyze_optical_flow as A  # noqa: E402
from optical_flow_dataset import OpticalFlowDataset  # noqa: E402


class _Dataset:
    def __init__(self, arr, attrs=None):
        self.arr, self.attrs = arr, attrs or {}

    def __getitem__(self, key):
        assert key == ()
        return self.arr.copy()


class _File:
    def __init__(self, d):
        self.d = d

    def __getitem__(self, k):
        return self.d[k]

    def __contains__(self, k):
        return k in self.d

    def close(self):
        pass


def open_study(flow, masks, frame_rate):
    """the reference's OpticalFlowDataset.__init__ on a stand-in file: flow [N,H,W,2] with attrs['nframes'] = N"""
    N, H, W, _ = flow.shape
    attrs = {"nframes": N, "mode": "RVIO_2class", "waveforms_present": False, "units_converted": True, "frame_rate": frame_rate,
             "pixel_spacing": 0.05, "ID": "study", "labels": np.array(list(masks))}
    d = {"flow": _Dataset(flow, attrs), "echo": _Dataset(np.zeros((N, H, W), np.float16))}
    d.update({k: _Dataset(v) for k, v in masks.items()})
    h5py.File = lambda path, mode="r": _File(d)
    ds = OpticalFlowDataset("study.hdf5")
    assert ds.nframes == N - 2 and ds.vel_array.dtype == np.float32 and isinstance(ds.frame_rate, np.float64)
    return ds


def run(ds, tag, labels, out):
    for param in ("velocity", "acceleration", "PWR"):
        for label in labels:
            k = f"{tag}/{param}/{label}"
            try:
                mf, af, me, ae, hi = A.calculate_3dhist(ds, param, label)
            except IndexError:                     # an empty first frame: the reference's perc_hi[-1]
                out[k + "/raises"] = np.str_("IndexError")
            else:
                out[k + "/mag_freq"], out[k + "/ang_freq"], out[k + "/hi"] = mf, af, hi
                out[k + "/mag_edges"], out[k + "/ang_edges"] = np.asarray(me), np.asarray(ae)
            RecordingSmoother.received.clear()
            ds.CARDIACCYCLE_CALCULATED = False
            try:
                A.sysdia_frames_by_angle(ds, param, label, recalculate=True)
            except Exception as e:                 # the steps after the smoother (find_start_stop) may trip on a short series
                print(f"  {k}: after the smoother: {e!r}")
            assert len(RecordingSmoother.received) == 1
            out[k + "/ang_mode"] = RecordingSmoother.received[0]


def near_rounding_boundary(rng, count):
    """(x, y) float32 pairs whose angle * 100.f lies within one ulp of a .5 (np.round's tie), some exactly on it"""
    got_x, got_y, exact = [], [], 0
    while len(got_x) < count:
        x = rng.uniform(-3, 3, 2_000_000).astype(np.float32)
        y = rng.uniform(-3, 3, 2_000_000).astype(np.float32)
        _, ang = cart_to_polar(x, y)
        r = ang * np.float32(100)
        d = np.abs(r - (np.floor(r) + np.float32(0.5)))
        hit = d <= np.spacing(r)
        on = d == 0
        exact += int(on.sum())
        sel = np.flatnonzero(on)[:count // 2].tolist() + np.flatnonzero(hit & ~on)[:count].tolist()
        got_x += x[sel].tolist()
        got_y += y[sel].tolist()
    return np.float32(got_x[:count]), np.float32(got_y[:count]), exact


def stress_study():
    """9 flow frames (7 analysed) of 24 x 40, float32, labels 'all' and 'late' (empty from frame 4 on)"""
    rng = np.random.default_rng(20261017)
    N, H, W = 9, 24, 40
    flow = rng.normal(0, 2, (N, H, W, 2)).astype(np.float32)
    case = {}
    # frame 0, row 0: signed zeros and both signs of each axis, |x| = |y|
    s = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (1.5, 0.0), (-1.5, 0.0), (0.0, 1.5), (0.0, -1.5), (-2.0, -0.0),
         (-0.0, -2.0), (3.0, 3.0), (-3.0, 3.0), (-3.0, -3.0), (3.0, -3.0), (1e-45, 0.0), (-1e-45, -1e-45), (2.5, -0.0)]
    for j, (a, b) in enumerate(s):
        flow[0, 0, j] = (a, b)
    case["signed"] = np.array([0, 0, len(s)])
    # frames 0-2, rows 1-3: angles within an ulp of np.round's .5 tie
    bx, by, _ = near_rounding_boundary(rng, 3 * 3 * W)
    flow[0:3, 1:4, :, 0] = bx.reshape(3, 3, W)
    flow[0:3, 1:4, :, 1] = by.reshape(3, 3, W)
    # frame 3: flow along +x only, so every angle is 0 while the magnitudes are not
    flow[3, ..., 0] = np.abs(flow[3, ..., 0]) + 0.25
    flow[3, ..., 1] = 0.0
    case["no_angle"] = np.array([3])
    # frame 5: a tie in the mode: 40 pixels on +y (k 157) and 40 on -x (k 314), the rest scattered
    _, a5 = cart_to_polar(flow[5, ..., 0], flow[5, ..., 1])
    k5 = np.rint(a5 * np.float32(100))
    flow[5][(k5 == 157) | (k5 == 314)] = (1.0, 0.5)          # no scattered pixel joins either side of the tie
    flow[5, 5, :, :] = (0.0, 2.0)
    flow[5, 6, :, :] = (-2.0, 0.0)
    case["mode_tie"] = np.array([5])
    yy, xx = np.mgrid[:H, :W]
    roi = ((yy - 12) / 11.5) ** 2 + ((xx - 20) / 19.5) ** 2 < 1.0
    allm = np.repeat(roi[None], N, 0)
    allm[:, 0, :len(s)] = True
    allm[0:3, 1:4, :] = True
    allm[5, 5:7, :] = True
    late = allm.copy()
    late[4:] = False
    case["late_empty"] = np.array([4])
    masks = {"all": np.stack([allm, allm], -1), "late": np.stack([late, late], -1)}
    return flow, masks, np.float64(29.97), case


if __name__ == "__main__":
    assert np.__version__ == "2.2.6" and scipy.__version__ == "1.15.3", (np.__version__, scipy.__version__)
    out = {}
    with np.load(os.path.join(HERE, "reference_study_stats.npz")) as z:
        ds = open_study(z["flow"], {"rv": z["rv"], "av": z["av"]}, np.float64(z["frame_rate"]))
    run(ds, "study", ("rv", "av"), out)
    flow, masks, fr, case = stress_study()
    ds = open_study(flow, masks, fr)
    run(ds, "stress", ("all", "late"), out)
    out["stress/flow"], out["stress/frame_rate"], out["stress/nframes"] = flow, fr, np.int64(ds.nframes)
    for k, v in masks.items():
        out[f"stress/{k}"] = v
    for k, v in case.items():
        out[f"stress/case/{k}"] = v
    np.savez_compressed(os.path.join(HERE, "reference_polar.npz"), **out)
    print({k: (np.shape(v), np.asarray(v).dtype) for k, v in out.items() if "/velocity/" in k or k.startswith("stress/")})
