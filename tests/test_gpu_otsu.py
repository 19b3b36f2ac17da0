"""The Otsu segmentation mode on the device (tf_otsu_masks, DenseFlow.otsu_masks): bit-equal to the reference's own
predict_movie_thres (tests/golden/reference_otsu.npz, reference_host_side.npz) and to the host path at study sizes, on both solver
handles, beside submitted solves on the same engine, and through process_video and process_folder.  No tolerance anywhere."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tee_optical_flow_amd import masks
from tests import luma_cases
from tests.test_otsu_cpu import _Cfg, fixture_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_H5 = "/opt/conda/bin/python3.9"


def _sector(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    ang = np.arctan2(xx - W / 2, yy + H * 0.05)
    return (np.abs(ang) < 0.7) & (np.hypot(xx - W / 2, yy + H * 0.05) < H * 0.98)


def _speckle_rgb(seed, N, H, W):
    """speckle frames with independent noise per channel (true RGB), bright and dark regions"""
    from tee_optical_flow_amd.synth import speckle_sequence
    rng = np.random.default_rng(seed)
    g = speckle_sequence(seed, N, H, W).astype(np.int16)
    out = np.empty((N, H, W, 3), np.uint8)
    for c in range(3):
        out[..., c] = np.clip(g + rng.integers(-12, 13, g.shape, dtype=np.int16), 0, 255)
    return out


def _sector_grey(seed, N, H, W):
    """sector-masked speckle (a large zero background) with a dark chamber that moves"""
    from tee_optical_flow_amd.synth import speckle_sequence
    g = np.where(_sector(H, W)[None], speckle_sequence(seed, N, H, W), 0).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(N):
        g[f][np.hypot(yy - H * 0.5, xx - W * 0.45 - f) < H / 8] //= 12
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=3))


def _check(got, want):
    assert got.dtype == want.dtype == np.bool_ and got.shape == want.shape and got.flags.c_contiguous
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case", fixture_cases(), ids=lambda c: c[0])
def test_device_equals_reference_fixture(engine, case):
    name, frames, min_size, ref, thr = case
    got, got_thr = engine.otsu_masks(frames, min_size, return_thresholds=True)
    assert got.dtype == np.bool_ and got.shape == frames.shape[:3] + (2,) and got.flags.c_contiguous
    assert got_thr.dtype == np.float64 and np.array_equal(got_thr, thr), (got_thr - thr).tolist()
    assert np.array_equal(got[..., 0], ref) and np.array_equal(got[..., 1], ref)
    assert np.array_equal(got.view(np.uint8)[..., 0], ref.astype(np.uint8))               # bytes 0 / 1
    d = masks.predict_movie_thres(frames, config=_Cfg(min_size), engine=engine)
    assert list(d) == ["otsu"] and np.array_equal(d["otsu"], got)


def test_device_equals_the_host_side_fixture(engine):
    """the Otsu case tests/test_golden.py pins for the host path"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_host_side.npz"))
    got = masks.predict_movie_thres(z["otsu_in"], engine=engine)
    _check(got["otsu"], z["otsu_out"].astype(bool))


@pytest.mark.parametrize("kind,N,H,W,min_size", [
    ("speckle", 65, 512, 512, 500),
    ("sector", 65, 600, 800, 500),
    ("speckle", 7, 333, 1025, 500),
    ("sector", 120, 600, 800, 500),                 # two chunks of frames (10 B of labelling scratch per pixel and frame, 512 MiB: 111 frames)
    ("speckle", 5, 97, 131, 0),
    ("sector", 2, 97, 131, 30),
])
def test_device_equals_host(engine, kind, N, H, W, min_size):
    frames = (_speckle_rgb if kind == "speckle" else _sector_grey)(N + H, N, H, W)
    if kind == "sector" and N >= 65:
        frames[N // 2] = 9                           # a constant frame inside a study (and, at 120 frames, not at the chunk boundary)
    want = masks.predict_movie_thres(frames, config=_Cfg(min_size))["otsu"]
    got, thr = engine.otsu_masks(frames, min_size, return_thresholds=True)
    _check(got, want)
    for f in sorted({0, N // 2, N - 1}):
        # the host luma goes through numpy's BLAS, whose summation order is its own: compare the thresholds of
        # the plain-order luma, which is what the device evaluates
        assert thr[f] == masks.threshold_otsu(luma_cases.luma(frames[f])), f
    assert want.any() and not want.all()


def test_both_solver_handles_give_the_same_masks(engine):
    import tee_optical_flow_amd as T
    frames = _speckle_rgb(11, 9, 200, 264)
    a, ta = engine.otsu_masks(frames, 50, return_thresholds=True)
    deep = T.DenseFlow(device_id=0, algo="deepflow")
    try:
        b, tb = deep.otsu_masks(frames, 50, return_thresholds=True)
    finally:
        deep.close()
    _check(a, b)
    assert np.array_equal(ta, tb)
    _check(a, masks.predict_movie_thres(frames, config=_Cfg(50))["otsu"])


@pytest.mark.parametrize("algo", ["TVL1", "deepflow"])
def test_masks_beside_two_submitted_studies(algo):
    """two studies submitted (tf_submit_seq) and still in flight on the engine's lanes, Otsu masks made on the same engine before the
    waits: masks and flows equal their serial runs"""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_sequence
    g1, g2 = speckle_sequence(31, 24, 256, 256), speckle_sequence(32, 20, 256, 256)
    frames = _sector_grey(5, 33, 512, 512)
    host = masks.predict_movie_thres(frames, config=_Cfg(500))["otsu"]
    eng = T.DenseFlow(device_id=0, algo=algo)
    try:
        s1, s2 = eng.calc_batch(g1).copy(), eng.calc_batch(g2).copy()
        alone = eng.otsu_masks(frames, 500)
        t1 = eng.submit_batch(g1)
        t2 = eng.submit_batch(g2)
        got = eng.otsu_masks(frames, 500)
        f2 = np.array(eng.wait(t2))
        f1 = np.array(eng.wait(t1))
    finally:
        eng.close()
    _check(got, host)
    _check(alone, host)
    assert np.array_equal(f1, s1) and np.array_equal(f2, s2)


def test_repeated_calls_do_not_grow_device_memory(engine):
    from tee_optical_flow_amd import _lib
    hip = _lib.load()

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    frames = _speckle_rgb(3, 12, 256, 320)
    first = engine.otsu_masks(frames, 100).copy()
    free = []
    for _ in range(6):
        assert np.array_equal(engine.otsu_masks(frames, 100), first)
        engine.otsu_masks(frames[:5, :100, :200], 100)                    # a smaller call reuses the scratch as well
        free.append(free_bytes())
    assert min(free[1:]) >= free[0] - (8 << 20), [f >> 20 for f in free]  # MiB free after each round


def test_process_video_makes_the_otsu_masks_on_the_flow_model(engine, monkeypatch):
    """process_video(mode='otsu') makes its masks on the flow model (given or its own) and hands the writer what a run given
    mask_dict= from the host path hands it; with mask_dict= the engine is not asked"""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.pipeline import process_video
    nparr = _sector_grey(12, 8, 96, 128)
    md = {"pixel_spacing": 0.04, "frame_rate": 50.0, "R_wave_data_present": False, "R_times": None}
    calls = []
    real = T.DenseFlow.otsu_masks

    def counted(self, *a, **k):
        calls.append(a[0].shape)
        return real(self, *a, **k)
    monkeypatch.setattr(T.DenseFlow, "otsu_masks", counted)
    host_masks = masks.predict_movie_thres(nparr)
    assert calls == []
    jobs = {}
    kw = dict(verbose=False, mode="otsu", no_saliency=True, nparr=nparr, metadata=md)
    ref = process_video(None, "ref.hdf5", None, flow_model=engine, mask_dict=host_masks, _defer_save=lambda j: jobs.setdefault("ref", j), **kw)
    assert calls == []
    dev = process_video(None, "dev.hdf5", None, flow_model=engine, _defer_save=lambda j: jobs.setdefault("dev", j), **kw)
    assert calls == [(8, 96, 128, 3)]
    own = process_video(None, "own.hdf5", None, _defer_save=lambda j: jobs.setdefault("own", j), **kw)      # the call makes its own model
    assert len(calls) == 2
    assert np.array_equal(dev, ref) and np.array_equal(own, ref)
    for name in ("dev", "own"):
        assert list(jobs[name].mask_dict) == ["otsu"]
        _check(np.asarray(jobs[name].mask_dict["otsu"]), host_masks["otsu"])
        assert np.array_equal(jobs[name].flow, jobs["ref"].flow)


SCRIPT = r"""
import sys, json, os, hashlib, numpy as np
sys.path.insert(0, ROOT)
import h5py
import tee_optical_flow_amd as T
from tee_optical_flow_amd import masks
from tee_optical_flow_amd.pipeline import process_folder, process_video
from tee_optical_flow_amd.synth import speckle_sequence
src = os.path.join(TMP, "in")
os.makedirs(src)
studies = {}
yy, xx = np.mgrid[0:128, 0:160]
sector = (np.abs(np.arctan2(xx - 80, yy + 6)) < 0.7) & (np.hypot(xx - 80, yy + 6) < 125)
for k in range(4):
    g = np.where(sector[None], speckle_sequence(300 + k, 7, 128, 160), 0).astype(np.uint8)
    studies[f"st{k}"] = np.repeat(g[..., None], 3, axis=3)
    np.savez(os.path.join(src, f"st{k}.npz"), nparr=studies[f"st{k}"], pixel_spacing=0.04, frame_rate=50.0, patient_id=f"SYN{k}", heart_rate=60)
def content(path):
    # everything the file holds: size, and per dataset its name, type, shape, filter, attributes and the bytes of its values.  (The
    # files themselves differ in the object headers' modification times, second by second, whatever wrote them.)
    with h5py.File(path, "r") as f:
        items = [(k, str(f[k].dtype), tuple(f[k].shape), f[k].compression, f[k].compression_opts,
                  sorted((a, repr(np.asarray(v).tolist())) for a, v in f[k].attrs.items()),
                  hashlib.sha256(np.ascontiguousarray(f[k][...]).tobytes()).hexdigest()) for k in sorted(f.keys())]
    return repr((os.path.getsize(path), items))
calls = []
real = T.DenseFlow.otsu_masks
def counted(self, *a, **k):
    calls.append(tuple(a[0].shape))
    return real(self, *a, **k)
T.DenseFlow.otsu_masks = counted
out = {"errors": {}, "calls": {}, "same": {}}
digest = {}
kw = dict(nchunks=1, chunk_index=0, mode="otsu", verbose=False, extensions=("npz",), OF_algo="TVL1")
for tag, extra in (("host", dict(otsu_masks="host")), ("device", dict(otsu_masks="device")), ("default", {}),
                   ("device_threads", dict(otsu_masks="device", workers="thread", studies_in_flight=1))):
    n0 = len(calls)
    dst = os.path.join(TMP, "out_" + tag)
    out["errors"][tag] = process_folder(src, dst, None, **kw, **extra)
    out["calls"][tag] = len(calls) - n0
    digest[tag] = {f: content(os.path.join(dst, f)) for f in sorted(os.listdir(dst))}
out["files"] = sorted(digest["host"])
for tag in digest:
    out["same"][tag] = digest[tag] == digest["host"]
# process_video: masks on the engine against mask_dict= from the host path
md = {"pixel_spacing": 0.04, "frame_rate": 50.0, "R_wave_data_present": False, "R_times": None}
eng = T.DenseFlow(device_id=0)
nparr = studies["st1"]
n0 = len(calls)
pv = dict(verbose=False, mode="otsu", no_saliency=True, nparr=nparr, metadata=md, patient_id="SYN1", heart_rate=60, flow_model=eng)
process_video(None, os.path.join(TMP, "pv_host.hdf5"), None, mask_dict=masks.predict_movie_thres(nparr), **pv)
out["pv_calls_host"] = len(calls) - n0
process_video(None, os.path.join(TMP, "pv_dev.hdf5"), None, **pv)
out["pv_calls_dev"] = len(calls) - n0
eng.close()
a, b = (content(os.path.join(TMP, n)) for n in ("pv_host.hdf5", "pv_dev.hdf5"))
out["pv_same"] = a == b and os.path.getsize(os.path.join(TMP, "pv_dev.hdf5")) > 1000
with h5py.File(os.path.join(TMP, "pv_dev.hdf5"), "r") as f:
    out["pv_mask_any"] = bool(f["otsu"][...].any()) if "otsu" in f else sorted(f.keys())
print(json.dumps(out, default=str))
"""


def test_process_video_and_process_folder_write_the_same_files(tmp_path):
    """process_folder(otsu_masks='device') against 'host' (the default), and process_video with the masks made on the engine against
    mask_dict= from the host path: the HDF5 files have the same size and hold the same datasets, attributes and values, byte for
    byte (two writes of one study already differ in the modification times of the object headers, so the files' own bytes are not
    compared)"""
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    env = {**os.environ, "PYTHONDONTWRITEBYTECODE": "1"}
    sys_stdcpp = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"       # conda ships an older libstdc++ than libamdhip64 needs
    if os.path.exists(sys_stdcpp):
        env["LD_PRELOAD"] = " ".join(filter(None, [os.environ.get("LD_PRELOAD"), sys_stdcpp]))
    script = SCRIPT.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp_path)))
    r = subprocess.run([PY_H5, "-c", script], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    g = json.loads(r.stdout.strip().splitlines()[-1])
    assert g["files"] == ["st0.hdf5", "st1.hdf5", "st2.hdf5", "st3.hdf5"]
    assert all(e == [] for e in g["errors"].values()), g["errors"]
    assert g["calls"] == {"host": 0, "default": 0, "device": 4, "device_threads": 4}      # the default is the host form
    assert all(g["same"].values()), g["same"]
    assert g["pv_calls_host"] == 0 and g["pv_calls_dev"] == 1 and g["pv_same"] and g["pv_mask_any"] is True
