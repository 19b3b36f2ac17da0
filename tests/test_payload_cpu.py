"""process_folder / process_video(payload="device") on the CPU: the walk's side of the float16 hand-over.  The flow models are TEST DOUBLES
(the product's model has no CPU path): one offers the float16 study calls (`device_payload`), computed with numpy from the host twins, and
RAISES from the float32 study calls; the other offers only the float32 ones.  Both walks must write the same files, byte for byte
(tests/payload_cases.py same_file: all but HDF5's own time stamps).
h5py lives only in the image's second interpreter, so the walks run there."""
import json
import logging
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_H5 = "/opt/conda/bin/python3.9"

FAKES = r"""
import numpy as np
from tee_optical_flow_amd.frames import rgb2gray

def _flow32(rgb, scale, pad_last, sal=False):
    g = rgb[..., 1 if sal else 0].astype(np.float32)
    d = (g[1:] - g[:-1]) / (48 if sal else 64)
    f = np.stack([d, -0.5 * d], -1) * np.float32(scale)
    return np.concatenate([f, f[-1:]]) if pad_last else f

class HostFake:                         # the float32 study calls only (what DenseFlow offered before the float16 ones)
    device_unit_scale = True
    def __init__(self): self.log, self.jobs, self.n = [], {}, 0
    def calc_study(self, rgb, scale=1.0, pad_last=False):
        self.log.append("calc_study"); return _flow32(rgb, scale, pad_last)
    def calc_study_saliency(self, rgb, scale=1.0, pad_last=False, map_dtype="f32"):
        self.log.append("calc_study_saliency"); return _flow32(rgb, scale, pad_last, sal=True)
    def submit_study(self, rgb, scale=1.0, pad_last=False):
        self.n += 1; self.log.append("submit_study"); self.jobs[self.n] = _flow32(rgb, scale, pad_last); return self.n
    def wait(self, t): return self.jobs.pop(t)
    def close(self): pass

class PayloadFake:                      # the float16 study calls, from the host twins; the float32 ones must not be used
    device_unit_scale = True
    device_payload = True
    def __init__(self): self.log, self.jobs, self.n = [], {}, 0
    def _pair(self, rgb, scale, pad_last, echo, sal=False):
        assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
        return _flow32(rgb, scale, pad_last, sal).astype(np.float16), rgb2gray(rgb).astype(np.float16) if echo else None
    def calc_study_payload(self, rgb, scale=1.0, pad_last=True, echo=True):
        self.log.append(("calc_study_payload", bool(echo))); return self._pair(rgb, scale, pad_last, echo)
    def calc_study_saliency_payload(self, rgb, scale=1.0, pad_last=True, echo=True, map_dtype="f32"):
        self.log.append(("calc_study_saliency_payload", bool(echo))); return self._pair(rgb, scale, pad_last, echo, sal=True)
    def submit_study_payload(self, rgb, scale=1.0, pad_last=True, echo=True):
        self.n += 1; self.log.append(("submit_study_payload", bool(echo))); self.jobs[self.n] = self._pair(rgb, scale, pad_last, echo); return self.n
    def wait(self, t): return self.jobs.pop(t)
    def _no(self, *a, **k): raise RuntimeError("a float32 study call was used under payload='device'")
    calc_study = calc_study_saliency = submit_study = calc_batch = _no
    def close(self): pass
"""

WALK_DRIVER = r"""
import sys, json, os, logging, numpy as np
sys.path.insert(0, ROOT)
import h5py
from concurrent.futures import ProcessPoolExecutor
from tee_optical_flow_amd import pipeline
from tee_optical_flow_amd.pipeline import process_folder
from tee_optical_flow_amd.synth import speckle_sequence
FAKES

warnings, want_echo = [], []
class Grab(logging.Handler):
    def emit(self, rec):
        if rec.levelno >= logging.WARNING: warnings.append(rec.getMessage())
pipeline.logger.addHandler(Grab())

# what the reader stage is asked for: _prepare_study(reader, path, mode, flipLR, config, want_echo, otsu_ahead), in a thread or a process
real_prepare, real_submit = pipeline._prepare_study, ProcessPoolExecutor.submit
def spy_prepare(reader, path, mode, flipLR, config, want_echo_, otsu_ahead=True):
    want_echo.append(bool(want_echo_)); return real_prepare(reader, path, mode, flipLR, config, want_echo_, otsu_ahead)
def spy_submit(self, fn, *args, **kwargs):
    if fn is pipeline._prepare_study_shm: want_echo.append(bool(args[5]))
    return real_submit(self, fn, *args, **kwargs)
pipeline._prepare_study = spy_prepare
ProcessPoolExecutor.submit = spy_submit

from tests.payload_cases import same_file
def same_files(a, b):
    names = sorted(os.listdir(a))
    return names == sorted(os.listdir(b)) and len(names) == 3 and all(same_file(os.path.join(a, n), os.path.join(b, n)) for n in names)

if __name__ == "__main__":
    src = os.path.join(TMP, "in"); os.makedirs(src)
    for k in range(3):
        rng = np.random.default_rng(700 + k)
        g = speckle_sequence(700 + k, 5, 48, 56)
        rgb = np.stack([g, np.roll(g, 3, axis=2), rng.integers(0, 256, g.shape, dtype=np.uint8)], -1)     # a real RGB study: R != G != B
        np.savez(os.path.join(src, f"s{k}.npz"), nparr=rgb, pixel_spacing=0.05, frame_rate=40.0, patient_id=f"P{k}", heart_rate=70)
    kw = dict(nchunks=1, chunk_index=0, mode="otsu", verbose=False, extensions=("npz",))
    out = {}
    def walk(tag, model, **more):
        del warnings[:], want_echo[:]
        before = dict(pipeline._shm_stats)
        errs = process_folder(src, os.path.join(TMP, tag), None, flow_model=model, **{**kw, **more})
        out[tag] = {"errors": errs, "log": model.log, "left": len(model.jobs), "warnings": list(warnings), "want_echo": list(want_echo),
                    "shm": {k: pipeline._shm_stats[k] - before[k] for k in before}}
        return os.path.join(TMP, tag)
    proc = dict(workers="process", n_readers=2, n_writers=2)
    shm_before = set(os.listdir("/dev/shm")) if os.path.isdir("/dev/shm") else set()
    h_thr = walk("h_thr", HostFake(), workers="thread", payload="host")
    d_thr = walk("d_thr", PayloadFake(), workers="thread", payload="device")
    d_thr1 = walk("d_thr1", PayloadFake(), workers="thread", payload="device", studies_in_flight=1)
    h_prc = walk("h_prc", HostFake(), payload="host", **proc)
    d_prc = walk("d_prc", PayloadFake(), payload="device", **proc)
    h_sal = walk("h_sal", HostFake(), workers="thread", payload="host", no_saliency=False)
    d_sal = walk("d_sal", PayloadFake(), workers="thread", payload="device", no_saliency=False)
    fb_thr = walk("fb_thr", HostFake(), workers="thread", payload="device")          # no device_payload: the host path, one message
    fb_prc = walk("fb_prc", HostFake(), payload="device", **proc)
    out["same"] = {"d_thr": same_files(h_thr, d_thr), "d_thr1": same_files(h_thr, d_thr1), "h_prc": same_files(h_thr, h_prc),
                   "d_prc": same_files(h_thr, d_prc), "d_sal": same_files(h_sal, d_sal), "sal_differs": not same_files(h_thr, h_sal),
                   "fb_thr": same_files(h_thr, fb_thr), "fb_prc": same_files(h_thr, fb_prc)}
    out["shm_left"] = sorted((set(os.listdir("/dev/shm")) if os.path.isdir("/dev/shm") else set()) - shm_before)
    with h5py.File(os.path.join(d_prc, "s0.hdf5"), "r") as f:
        out["dtypes"] = {k: str(f[k].dtype) for k in ("flow", "echo")}
        out["flow_nonzero"] = bool(np.any(f["flow"][...] != 0))
    print(json.dumps(out, default=str))
"""


def _run(tmp_path, text, name, env=None):
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    script = tmp_path / name
    script.write_text(text.replace("FAKES", FAKES).replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp_path))))
    r = subprocess.run([PY_H5, str(script)], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1", **(env or {})})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "leaked shared_memory" not in r.stderr, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    # 1 KB threshold: these small studies' frames, masks, echo and flow all travel as shared-memory blocks, as real studies' do
    return _run(tmp_path_factory.mktemp("payload"), WALK_DRIVER, "walks.py", env={"TEEFLOW_SHM_MIN_BYTES": "1024"})


def test_device_payload_walk_writes_the_host_walks_files(walks):
    """The model whose float32 study calls raise serves every study through the float16 calls; threads or worker processes, studies in
    flight or one by one, gray or saliency branch: each file has the bytes of the payload="host" walk's."""
    for tag in ("h_thr", "d_thr", "d_thr1", "h_prc", "d_prc", "h_sal", "d_sal"):
        assert walks[tag]["errors"] == [] and walks[tag]["left"] == 0, (tag, walks[tag])
    assert all(walks["same"].values()), walks["same"]
    assert walks["dtypes"] == {"flow": "float16", "echo": "float16"} and walks["flow_nonzero"]
    assert walks["d_thr"]["log"] == [["submit_study_payload", True]] * 3 and walks["d_prc"]["log"] == [["submit_study_payload", True]] * 3
    assert walks["d_thr1"]["log"] == [["calc_study_payload", True]] * 3
    assert walks["d_sal"]["log"] == [["calc_study_saliency_payload", True]] * 3
    assert not walks["d_thr"]["warnings"] and not walks["d_prc"]["warnings"]
    assert walks["shm_left"] == [], "shared-memory blocks left behind"


def test_device_payload_walk_asks_the_reader_stage_for_no_echo(walks):
    """payload="device": _prepare_study gets want_echo=False, also in worker processes (where the host walk asks for it); a study then
    maps frames + Otsu masks and creates two blocks, flow and echo, where the host walk maps three and creates one."""
    assert walks["d_prc"]["want_echo"] == [False] * 3 and walks["d_thr"]["want_echo"] == [False] * 3
    assert walks["h_prc"]["want_echo"] == [True] * 3
    assert walks["h_prc"]["shm"] == {"mapped": 9, "created": 3}
    assert walks["d_prc"]["shm"] == {"mapped": 6, "created": 6}


def test_model_without_device_payload_falls_back_and_says_so_once(walks):
    for tag in ("fb_thr", "fb_prc"):
        w = walks[tag]
        assert w["errors"] == [] and w["log"] == ["submit_study"] * 3, w
        said = [m for m in w["warnings"] if "payload='device' not used" in m]
        # (one message per process: the second walk of the driver finds the reason already logged)
        assert len(said) == (1 if tag == "fb_thr" else 0) and (not said or "HostFake" in said[0]), w["warnings"]
    assert walks["fb_prc"]["want_echo"] == [True] * 3            # the host path's reader stage makes the echo


def test_unknown_payload_is_a_configuration_error(tmp_path):
    from tee_optical_flow_amd.exceptions import ConfigurationError
    from tee_optical_flow_amd.pipeline import process_folder, process_video
    (tmp_path / "in").mkdir()
    with pytest.raises(ConfigurationError, match="payload"):
        process_folder(str(tmp_path / "in"), str(tmp_path / "out"), None, payload="bogus")
    with pytest.raises(ConfigurationError, match="payload"):
        process_video(None, None, None, mode="otsu", no_saliency=True, nparr=np.zeros((3, 8, 8, 3), np.uint8), payload="f16")


def test_wase_falls_back_to_the_host_path(caplog):
    """Background compensation works on float32 flows: payload="device" with bkgd_comp="WASE" takes the host path (the float16 calls of
    this stand-in raise), returns the float32 flows of payload="host" and logs why."""
    from tee_optical_flow_amd import pipeline
    from tee_optical_flow_amd.synth import speckle_sequence

    class Model:
        device_payload = True

        def calc_batch(self, frames, scale=1.0):
            d = (frames[1:].astype(np.float32) - frames[:-1].astype(np.float32)) / 64
            return np.stack([d, -0.5 * d], -1) * np.float32(scale)

        def _no(self, *a, **k):
            raise RuntimeError("a float16 study call was used under bkgd_comp='WASE'")
        calc_study_payload = submit_study_payload = calc_study_saliency_payload = _no

    g = speckle_sequence(5, 5, 40, 48)
    nparr = np.repeat(g[..., None], 3, axis=3)
    bk = np.zeros((5, 40, 48, 2), bool)
    bk[:, :10] = True
    kw = dict(verbose=False, mode="RVIO_2class", bkgd_comp="WASE", no_saliency=True, nparr=nparr, mask_dict={"bkgd": bk}, flow_model=Model())
    pipeline._payload_fallbacks.clear()
    with caplog.at_level(logging.WARNING, logger=pipeline.logger.name):
        dev = pipeline.process_video(None, None, None, payload="device", **kw)
        dev2 = pipeline.process_video(None, None, None, payload="device", **kw)
    host = pipeline.process_video(None, None, None, payload="host", **kw)
    assert dev.dtype == np.float32 and np.array_equal(dev, host) and np.array_equal(dev2, host)
    said = [r.getMessage() for r in caplog.records if "payload='device' not used" in r.getMessage()]
    assert len(said) == 1 and "WASE" in said[0]


WRITER_DRIVER = r"""
import sys, json, os, numpy as np
sys.path.insert(0, ROOT)
from tee_optical_flow_amd.config import default_optical_flow_config
from tee_optical_flow_amd.frames import rgb2gray
from tee_optical_flow_amd.hdf5_out import save_optical_flow_to_hdf5
rng = np.random.default_rng(11)
nparr = rng.integers(0, 256, (5, 40, 48, 3), dtype=np.uint8)
flow = (rng.standard_normal((5, 40, 48, 2)) * np.float32(3)).astype(np.float32)
flow[0, 0, 0] = (6.1e-5, 70000.0)                       # a float16 subnormal and an overflow to inf
masks = {"otsu": rng.random((5, 40, 48, 2)) > 0.5}
md = {"pixel_spacing": 0.05, "frame_rate": 40.0, "R_wave_data_present": False, "R_times": None}
rest = (md, {}, "P", 60, default_optical_flow_config(), "otsu", True, False, None)
a, b, c = (os.path.join(TMP, n) for n in ("a.hdf5", "b.hdf5", "c.hdf5"))
save_optical_flow_to_hdf5(a, flow, nparr, masks, *rest)
save_optical_flow_to_hdf5(b, flow.astype(np.float16), nparr, masks, *rest, echo=rgb2gray(nparr).astype(np.float16))
save_optical_flow_to_hdf5(c, flow.astype(np.float16), None, masks, *rest, echo=rgb2gray(nparr).astype(np.float16), nframes=5)
from tests.payload_cases import same_file
print(json.dumps({"same": same_file(a, b) and same_file(a, c), "size": os.path.getsize(a)}))
"""


def test_writer_takes_float16_flow_and_echo_and_writes_the_same_bytes(tmp_path):
    g = _run(tmp_path, WRITER_DRIVER, "writer.py")
    assert g["same"] and g["size"] > 1000
