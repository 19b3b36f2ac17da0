#!/opt/conda/bin/python3.9
"""Generates tests/golden/reference_overlay.npz by RUNNING the reference's own overlay renderers on study files:
visualize_radlong(ds, param, save_dir) (/root/reference/optical_flow/analyze_optical_flow.py:488-560) and
VisualizationManager.visualize_radlong (optical_flow/visualization.py:241-297, 1045-1051), on OpticalFlowDatasets
(optical_flow_dataset.py) that opened real HDF5 files in the study layout.

Run (build container only; the reference never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 /opt/conda/bin/python3.9 tests/golden/make_reference_overlay_fixtures.py

That interpreter has matplotlib 3.4.3, skimage, scipy 1.7, h5py and numpy 1.26; cv2, imageio, peakutils, polars, tsmoothie and
neurokit2 are MagicMock stubs so the modules import.  The video writer (`iio.get_writer` in both modules) is replaced by a recorder
that keeps the path, the fps, every frame handed to append_data and whether close was called: the frames are the fixture, the
encoding is not part of it.  matplotlib 3.4.3 has no `matplotlib.colormaps` registry, which VisualizationManager indexes by name;
the generator gives it a mapping whose __getitem__ is matplotlib.cm.get_cmap (the same colormap objects the registry of a later
matplotlib returns).

Stored, as data: per study `<study>/flow` float16 [N,H,W,2], `<study>/rv`, `<study>/av` bool [N,H,W,2], `<study>/echo` (float16 or
uint8 [N,H,W]), shared `frame_rate` and `nframes` = attrs['nframes'] - 2; and per case `<case>/frames` uint8 [nframes,H,2W,3], the
recorded frames, with `<case>/path` and `<case>/fps`.  Cases (all with av_filter_flag=False: scipy 1.7 refuses the default even
Savitzky-Golay window):
  main/<param>   visualize_radlong for velocity, acceleration, PWR; float16 echo; W = 45 (odd, not a multiple of 4); frame 0 is
                 quiet and later frames are not, so that later values fall outside +-half on both sides (asserted below)
  u8/velocity    the same study with a uint8 echo
  empty0/velocity  frame 0's rv mask is empty: half == 0
  vm/velocity    VisualizationManager.visualize_radlong with colormap_rad='BrBG', colormap_long='PiYG': m2 != 1 (asserted below)
frame_rate is an h5py np.float64; numpy 1.26 divides np.gradient's float32 field by it in float32, so a test that compares
acceleration or PWR with this fixture passes frame_rate as a Python float (see make_reference_study_stats_fixtures.py).
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
import matplotlib  # noqa: E402
import matplotlib.cm  # noqa: E402
import optical_flow.analyze_optical_flow as A  # noqa: E402
import optical_flow.visualization as V  # noqa: E402
from optical_flow.config import VisualizationConfig  # noqa: E402
from optical_flow_dataset import OpticalFlowDataset  # noqa: E402


class _Colormaps:
    def __getitem__(self, name):
        return matplotlib.cm.get_cmap(name)


if not hasattr(matplotlib, "colormaps"):
    matplotlib.colormaps = _Colormaps()


class Recorder:
    def __init__(self):
        self.calls = []

    def get_writer(self, path, fps=None):
        rec = {"path": path, "fps": fps, "frames": [], "closed": False}
        self.calls.append(rec)
        w = MagicMock()
        w.append_data = lambda fr: rec["frames"].append(np.array(fr))
        w.close = lambda: rec.__setitem__("closed", True)
        return w


OUT = os.path.dirname(os.path.abspath(__file__))
N, H, W = 8, 30, 45
FRAME_RATE = 29.97
rng = np.random.default_rng(20261017)
yy, xx = np.mgrid[:H, :W]

# flow: quantised speckle, quiet in frame 0 and growing afterwards; a few exact zeros
amp = np.array([0.5, 1, 2, 3, 4, 4, 3, 2], np.float64)[:, None, None, None]
flow = (np.round(rng.normal(0, 1, (N, H, W, 2)) * amp * 4) / 4).astype(np.float16)
flow[:, 12:15, 30:36, :] = 0
rv = np.zeros((N, H, W), bool)
av = np.zeros((N, H, W), bool)
for f in range(N):
    rv[f] = ((yy - 15 - 0.5 * f) / 11.0) ** 2 + ((xx - 22 + f) / 18.0) ** 2 < 1.0
    av[f] = ((yy - 8) / 4.0) ** 2 + ((xx - 10 - 2 * f) / 5.0) ** 2 < 1.0
# echo: a quantised sector image (few grey levels: it compresses), the study file's float16; and the same as uint8
grey = np.clip(np.round((np.hypot(yy - 2, xx - 22)[None] * 6 + rng.integers(0, 3, (N, H, W)) * 16) / 16) * 16, 0, 240)
grey[:, :3, :] = 0
echo16 = grey.astype(np.float16)
echo8 = grey.astype(np.uint8)
rv_empty0 = rv.copy()
rv_empty0[0] = False

STUDIES = {"main": (echo16, rv), "u8": (echo8, rv), "empty0": (echo16, rv_empty0)}


def write_study(path, echo, rvm):
    with h5py.File(path, "w") as fh:
        fh.create_dataset("echo", data=echo)
        d = fh.create_dataset("flow", data=flow)
        d.attrs["frame_rate"] = FRAME_RATE
        d.attrs["nframes"] = N
        d.attrs["pixel_spacing"] = 0.05
        d.attrs["ID"] = "study"
        d.attrs["HR"] = 0
        d.attrs["no_saliency"] = True
        d.attrs["mode"] = "RVIO_2class"
        d.attrs["units_converted"] = True
        d.attrs["waveforms_present"] = False
        fh.create_dataset("rv", data=np.stack([rvm, rvm], axis=-1))
        fh.create_dataset("av", data=np.stack([av, av], axis=-1))
        d.attrs["labels"] = ["rv", "av"]


out = {"frame_rate": np.float64(FRAME_RATE), "nframes": np.int64(N - 2)}
rec = Recorder()
A.iio = rec
V.iio = rec


def keep(case, call, n):
    assert call["closed"] and len(call["frames"]) == n
    fr = np.stack(call["frames"])
    assert fr.dtype == np.uint8 and fr.shape == (n, H, 2 * W, 3)
    out[f"{case}/frames"] = fr
    out[f"{case}/path"] = np.array(os.path.basename(call["path"]))
    out[f"{case}/fps"] = np.int64(call["fps"])


with tempfile.TemporaryDirectory() as td:
    for name, (echo, rvm) in STUDIES.items():
        path = os.path.join(td, f"{name}.hdf5")
        write_study(path, echo, rvm)
        ds = OpticalFlowDataset(path)
        n = ds.nframes
        assert n == N - 2 and isinstance(ds.frame_rate, np.float64) and ds.get_echo().dtype == echo.dtype
        out[f"{name}/flow"] = flow
        out[f"{name}/rv"] = ds.get_mask("rv")
        out[f"{name}/av"] = ds.get_mask("av")
        out[f"{name}/echo"] = ds.get_echo()
        out[f"{name}/filename"] = np.array(ds.filename)
        for param in (("velocity", "acceleration", "PWR") if name == "main" else ("velocity",)):
            A.visualize_radlong(ds, param, os.path.join(td, "videos"), fps=24, av_filter_flag=False)
            keep(f"{name}/{param}", rec.calls[-1], n)
        cent = A.calc_AV_centroid(ds.get_mask("av"), n, filter=False)
        rad, lon = A.calculate_comp_magnitude(ds.get_masked_arr("velocity", "rv"), cent)
        half = np.max(np.abs(rad[0]))
        if name == "main":
            # later frames leave +-half on both sides, in both components
            for arr in (rad, lon):
                assert half > 0 and (arr[1:] > half).any() and (arr[1:] < -half).any()
            vm = V.VisualizationManager(vis_config=VisualizationConfig(colormap_rad="BrBG", colormap_long="PiYG", fps=12))
            vm.visualize_radlong(rad, lon, ds.get_echo(), cent, ds.filename, os.path.join(td, "videos", "vm.mp4"), n)
            keep("vm/velocity", rec.calls[-1], n)
            # m2 of that case, from the colours the reference's own calls produce
            nrm = matplotlib.colors.CenteredNorm()
            cols = [matplotlib.cm.get_cmap(c)(nrm(a))[..., :3] for i in range(n) for c, a in (("BrBG", rad[i]), ("PiYG", lon[i]))]
            m2 = max(c.max() for c in cols)
            assert m2 != 1.0, m2
            out["vm/m2"] = np.float64(m2)
        if name == "empty0":
            assert half == 0 and (rad[1:] != 0).any()
        ds.close()
np.savez_compressed(os.path.join(OUT, "reference_overlay.npz"), **out)
print({k: (np.shape(v), np.asarray(v).dtype) for k, v in out.items()})
print(os.path.getsize(os.path.join(OUT, "reference_overlay.npz")), "bytes")
