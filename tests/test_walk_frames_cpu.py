"""process_video / process_folder(frames="device") on the CPU: the walk's side of the held frames.  The flow model is a TEST DOUBLE (the
product's model has no CPU path): tests/frames_cases.NumpyFrames' hold_frames / download_frames, the study calls computed with numpy
from whatever frames argument they get -- an array, or the token resolved the way the library's armed call reads it.  .npz studies of
every `photometric` value go through both walks; the files must be the same byte for byte (tests/payload_cases.py same_file: all but
HDF5's own time stamps), the host side converting with the twin.  h5py lives only in the image's second interpreter, so the walks run
there."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_H5 = "/opt/conda/bin/python3.9"

DRIVER = r"""
import sys, json, os, logging, itertools, zlib, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tee_optical_flow_amd import pipeline, masks as masks_mod
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.dense_flow import HeldFrames
from tee_optical_flow_amd.frames import rgb2gray
from tee_optical_flow_amd.pipeline import process_folder, process_video, read_study, read_study_stored
from tee_optical_flow_amd.synth import speckle_sequence
from tests.payload_cases import same_file
from tests.frames_cases import NumpyFrames

def _flow32(rgb, scale, sal=False):
    g = rgb[..., 1 if sal else 0].astype(np.float32)
    d = (g[1:] - g[:-1]) / (48 if sal else 64)
    f = np.stack([d, -0.5 * d], -1) * np.float32(scale)
    return np.concatenate([f, f[-1:]])

def _record(arr, chunks):
    stored = []
    for off in itertools.product(*[range(0, s, c) for s, c in zip(arr.shape, chunks)]):
        full = np.zeros(chunks, arr.dtype)
        blk = arr[tuple(slice(o, min(o + c, s)) for o, c, s in zip(off, chunks, arr.shape))]
        full[tuple(slice(0, n) for n in blk.shape)] = blk
        stored.append((off, 0, zlib.compress(full.tobytes(), 9)))
    return A.chunks_record(arr.shape, arr.dtype, chunks, stored)

class Plain:                              # no hold_frames: every frames argument is an array
    device_unit_scale = device_payload = True
    device_study_chunks = False
    device_id = 0
    def __init__(self): self.log, self.jobs, self.n, self.held, self.tokens = [], {}, 0, None, 0
    def _rgb(self, frames, min_frames=1):
        assert not isinstance(frames, HeldFrames)
        return np.asarray(frames)
    def _pair(self, name, frames, scale, echo, sal=False, hold=False):
        rgb = self._rgb(frames, 2)
        self.log.append(name)
        assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
        pair = _flow32(rgb, scale, sal).astype(np.float16), rgb2gray(rgb).astype(np.float16) if echo else None
        if hold: self.held = pair
        return pair
    def calc_study(self, frames, scale=1.0, pad_last=False):
        self.log.append("calc_study"); return _flow32(self._rgb(frames, 2), scale)
    def submit_study(self, frames, scale=1.0, pad_last=False):
        self.n += 1; self.log.append("submit_study"); self.jobs[self.n] = _flow32(self._rgb(frames, 2), scale); return self.n
    def calc_study_saliency(self, frames, scale=1.0, pad_last=False, map_dtype="f32"):
        self.log.append("calc_study_saliency"); return _flow32(self._rgb(frames, 2), scale, sal=True)
    def calc_study_payload(self, frames, scale=1.0, pad_last=True, echo=True, hold=False):
        return self._pair("calc_study_payload", frames, scale, echo, hold=hold)
    def calc_study_saliency_payload(self, frames, scale=1.0, pad_last=True, echo=True, map_dtype="f32", hold=False):
        return self._pair("calc_study_saliency_payload", frames, scale, echo, sal=True, hold=hold)
    def submit_study_payload(self, frames, scale=1.0, pad_last=True, echo=True):
        self.n += 1; self.jobs[self.n] = self._pair("submit_study_payload", frames, scale, echo); return self.n
    def wait(self, t): return self.jobs.pop(t)
    def calc_batch(self, gray, scale=1.0):                                   # (frames that are not uint8 RGB: the conditioned frames)
        self.log.append("calc_batch")
        d = (gray[1:].astype(np.float32) - gray[:-1].astype(np.float32)) / 64
        return np.stack([d, -0.5 * d], -1) * np.float32(scale)
    def held_deflate(self, what, chunks):
        self.log.append("held_deflate:" + what)
        return _record(self.held[0 if what == "flow" else 1], tuple(chunks))
    def otsu_masks(self, frames, min_size):
        self.log.append("otsu_masks")
        class Cfg: min_mask_size = min_size
        return masks_mod.predict_movie_thres(self._rgb(frames, 2), config=Cfg())["otsu"]
    def close(self): pass

class Holder(NumpyFrames, Plain):         # hold_frames & co.; a frames argument may be the token
    def __init__(self): NumpyFrames.__init__(self); Plain.__init__(self)
    def hold_frames(self, arr, form="RGB", flip=False):
        self.log.append(("hold_frames", form, bool(flip))); return NumpyFrames.hold_frames(self, arr, form, flip)
    def download_frames(self):
        self.log.append("download_frames"); return NumpyFrames.download_frames(self)
    def _rgb(self, frames, min_frames=1):
        self.tokens += isinstance(frames, HeldFrames)
        return self.resolve(frames, min_frames)

class HolderNoOtsu(Holder):               # Otsu on the host: from one download
    otsu_masks = property()

class Segmentor:                          # a stand-in for the SAM module on the host: evaluate_1_slice is replaced below
    pass
def fake_slice(frame, model):
    g = np.asarray(frame)[..., 0]
    return np.where(g > 150, 1, np.where(g < 60, 2, 0)).astype(np.uint8)
masks_mod.evaluate_1_slice = fake_slice

warnings = []
class Grab(logging.Handler):
    def emit(self, rec):
        if rec.levelno >= logging.WARNING: warnings.append(rec.getMessage())
pipeline.logger.addHandler(Grab())

def same_files(a, b):
    names = sorted(os.listdir(a))
    return bool(names) and names == sorted(os.listdir(b)) and all(same_file(os.path.join(a, n), os.path.join(b, n)) for n in names)

def stored(seed, photometric, n=5, h=48, w=56):
    rng = np.random.default_rng(seed)
    g = speckle_sequence(seed, n, h, w)
    if photometric == "MONOCHROME2":
        return g
    if photometric == "RGB":
        return np.stack([g, np.roll(g, 3, axis=2), rng.integers(0, 256, g.shape, dtype=np.uint8)], -1)
    return np.stack([g, rng.integers(64, 192, g.shape, dtype=np.uint8), rng.integers(64, 192, g.shape, dtype=np.uint8)], -1)   # Y, Cb, Cr

if __name__ == "__main__":
    tmp = TMP
    src = os.path.join(tmp, "in"); os.makedirs(src)
    kinds = ["RGB", "YBR_FULL", "YBR_FULL_422", "MONOCHROME2", None]
    for k, ph in enumerate(kinds):
        extra = {} if ph is None else {"photometric": ph}
        np.savez(os.path.join(src, f"s{k}.npz"), nparr=stored(900 + k, ph or "RGB"), pixel_spacing=0.05, frame_rate=40.0, patient_id=f"P{k}", heart_rate=70, **extra)
    out = {"walks": {}, "same": {}}
    base = dict(nchunks=1, chunk_index=0, verbose=False, extensions=("npz",), workers="thread")

    # two studies whose `flow` and `echo` are above create_gzip9's min_parallel_bytes, for deflate="device"
    big = os.path.join(tmp, "big"); os.makedirs(big)
    for k, ph in enumerate(["YBR_FULL", "MONOCHROME2"]):
        np.savez(os.path.join(big, f"b{k}.npz"), nparr=stored(950 + k, ph, 9, 240, 256), pixel_spacing=0.05, frame_rate=40.0, photometric=ph)

    def walk(tag, model, **more):
        del warnings[:]
        errs = process_folder(more.pop("folder", src), os.path.join(tmp, tag), more.pop("segmentor_model", None), flow_model=model, **{**base, **more})
        out["walks"][tag] = {"errors": errs, "log": [list(x) if isinstance(x, tuple) else x for x in model.log], "warnings": list(warnings),
                             "uploads": getattr(model, "uploads", None), "tokens": model.tokens, "left": len(model.jobs)}
        return os.path.join(tmp, tag)

    def both(tag, dev_model=Holder, **more):
        h = walk(tag + "_host", Plain(), frames="host", **more)
        d = walk(tag + "_dev", dev_model(), frames="device", **more)
        out["same"][tag] = same_files(h, d)

    for flip in (False, True):
        f = "_flip" if flip else ""
        both("otsu_dev" + f, mode="otsu", otsu_masks="device", flipLR=flip)
        both("otsu_host" + f, dev_model=HolderNoOtsu, mode="otsu", otsu_masks="host", flipLR=flip)
        both("payload" + f, mode="otsu", otsu_masks="device", payload="device", flipLR=flip)
        both("deflate" + f, folder=big, mode="otsu", otsu_masks="device", payload="device", deflate="device", no_saliency=False, flipLR=flip)
        both("segmentor" + f, mode="RVIO_2class", segmentor_model=Segmentor(), payload="device", flipLR=flip)
    both("in_flight_1", mode="otsu", otsu_masks="device", payload="device", studies_in_flight=1)
    # fallbacks: a model without hold_frames; a reader of the caller's
    fb = walk("fb_model", Plain(), frames="device", mode="otsu", otsu_masks="device")
    out["same"]["fb_model"] = same_files(os.path.join(tmp, "otsu_dev_host"), fb)
    fb = walk("fb_reader", Holder(), frames="device", mode="otsu", otsu_masks="device", reader=lambda p: read_study(p))
    out["same"]["fb_reader"] = same_files(os.path.join(tmp, "otsu_dev_host"), fb)
    # process_video, a study read from its file and frames injected; a grey stack of one frame and float frames take the host path
    pv = {}
    for k, ph in enumerate(kinds):
        path = os.path.join(src, f"s{k}.npz")
        for flip in (False, True):
            a, b = os.path.join(tmp, f"pv_h_{k}_{flip}.hdf5"), os.path.join(tmp, f"pv_d_{k}_{flip}.hdf5")
            m = Holder()
            fh = process_video(path, a, mode="otsu", flipLR=flip, no_saliency=True, flow_model=Plain(), frames="host")
            fd = process_video(path, b, mode="otsu", flipLR=flip, no_saliency=True, flow_model=m, frames="device")
            pv[f"{ph}{'_flip' if flip else ''}"] = [same_file(a, b), bool(np.array_equal(fh, fd)), m.log[0] if m.log else None, m.uploads == np.load(path)["nparr"].nbytes]
    out["process_video"] = pv
    del warnings[:]
    pipeline._frames_fallbacks.clear()
    m = Holder()
    rgb = stored(5, "RGB")
    inj_h = process_video(None, None, mode="otsu", no_saliency=True, flow_model=Plain(), nparr=rgb, flipLR=True)
    inj_d = process_video(None, None, mode="otsu", no_saliency=True, flow_model=m, nparr=rgb, flipLR=True, frames="device")
    out["injected"] = [bool(np.array_equal(inj_h, inj_d)), m.log[0]]
    m = Holder()
    f32 = process_video(None, None, mode="otsu", no_saliency=True, flow_model=m, nparr=stored(5, "MONOCHROME2").astype(np.float32) / 255, frames="device",
                        mask_dict={"otsu": np.ones((5, 48, 56, 2), bool)})
    out["float_frames"] = [m.log, list(warnings)]
    st = read_study_stored(os.path.join(src, "s1.npz"))
    out["stored"] = [st[1], bool(np.array_equal(st[0], np.load(os.path.join(src, "s1.npz"))["nparr"])),
                     bool(np.array_equal(read_study(os.path.join(src, "s1.npz"))[0], F.ybr_full_to_rgb(st[0]))), len(read_study(os.path.join(src, "s1.npz")))]
    np.savez(os.path.join(tmp, "bad.npz"), nparr=rgb, photometric="PALETTE COLOR")
    try:
        read_study(os.path.join(tmp, "bad.npz")); out["bad_photometric"] = "accepted"
    except Exception as e:
        out["bad_photometric"] = type(e).__name__
    print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    tmp = tmp_path_factory.mktemp("frames_walk")
    script = tmp / "walks.py"
    script.write_text(DRIVER.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp))))
    r = subprocess.run([PY_H5, str(script)], capture_output=True, text=True, timeout=600, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_device_frames_walks_write_the_host_walks_files(walks):
    assert all(not w["errors"] for w in walks["walks"].values()), {k: w["errors"] for k, w in walks["walks"].items() if w["errors"]}
    assert walks["same"] and all(walks["same"].values()), walks["same"]
    assert len(walks["same"]) == 13


def test_each_study_is_held_once_in_the_form_its_file_stores(walks):
    forms = ["RGB", "YBR_FULL", "YBR_FULL", "GRAY", "RGB"]                # s0 .. s4: RGB, YBR_FULL, YBR_FULL_422, MONOCHROME2, no key
    for tag, w in walks["walks"].items():
        if not tag.endswith("_dev"):
            continue
        holds = [x for x in w["log"] if isinstance(x, list) and x[0] == "hold_frames"]
        big = tag.startswith("deflate")                                    # (the two studies large enough for deflate="device")
        assert [h[1] for h in holds] == (["YBR_FULL", "GRAY"] if big else forms) and all(h[2] == ("_flip" in tag) for h in holds), (tag, holds)
        # what crossed the bus: every study's pixel data once, as stored (3 B per pixel, 1 B for the grey study)
        assert w["uploads"] == (9 * 240 * 256 * (3 + 1) if big else 5 * 48 * 56 * (3 * 4 + 1)), (tag, w["uploads"])
        assert w["tokens"] >= len(holds) and not w["warnings"] and w["left"] == 0, (tag, w)   # every study's solve (and masks) took the token


def test_the_host_gets_the_rgb_by_one_download_only_where_it_works_on_it(walks):
    n = lambda tag: walks["walks"][tag]["log"].count("download_frames")
    # masks and echo from the device: nothing comes back
    assert n("payload_dev") == n("payload_flip_dev") == n("deflate_dev") == n("in_flight_1_dev") == 0
    # float32 flows, the writer makes `echo` from the RGB: once per study; host Otsu shares that download
    assert n("otsu_dev_dev") == 5 and n("otsu_host_dev") == 5
    # a host segmentor with the device's echo: once per study, for the segmentor
    assert n("segmentor_dev") == 5
    assert "otsu_masks" in walks["walks"]["otsu_dev_dev"]["log"] and "otsu_masks" not in walks["walks"]["otsu_host_dev"]["log"]
    assert walks["walks"]["deflate_dev"]["log"].count("held_deflate:flow") == walks["walks"]["deflate_dev"]["log"].count("held_deflate:echo") == 2


def test_fallbacks_say_why_once_per_walk(walks):
    w = walks["walks"]["fb_model"]
    assert len(w["warnings"]) == 1 and "frames='device' not used" in w["warnings"][0] and "has no hold_frames" in w["warnings"][0]
    w = walks["walks"]["fb_reader"]
    assert len(w["warnings"]) == 1 and "only the default reader" in w["warnings"][0]
    assert not any(isinstance(x, list) for x in w["log"]) and w["uploads"] > 0          # nothing was held: arrays went in
    log, warned = walks["float_frames"]
    assert not any(isinstance(x, list) for x in log) and len(warned) == 1 and "not uint8" in warned[0]


def test_process_video_reads_the_study_as_stored(walks):
    pv = walks["process_video"]
    assert len(pv) == 10
    for name, (same, flows, first, once) in pv.items():
        assert same and flows and once, (name, pv[name])
        form = {"RGB": "RGB", "None": "RGB", "YBR_FULL": "YBR_FULL", "YBR_FULL_422": "YBR_FULL", "MONOCHROME2": "GRAY"}[name.replace("_flip", "")]
        assert first == ["hold_frames", form, name.endswith("_flip")], (name, first)
    assert walks["injected"] == [True, ["hold_frames", "RGB", True]]
    assert walks["stored"] == ["YBR_FULL", True, True, 4]                               # read_study's return value is what it was
    assert walks["bad_photometric"] == "DICOMReadError"


def test_frames_is_checked_before_any_work(tmp_path):
    from tee_optical_flow_amd.exceptions import ConfigurationError
    from tee_optical_flow_amd.pipeline import process_folder, process_video
    with pytest.raises(ConfigurationError, match="frames must be"):
        process_folder(str(tmp_path), str(tmp_path / "out"), frames="gpu")
    with pytest.raises(ConfigurationError, match="frames must be"):
        process_video(None, None, nparr=np.zeros((2, 4, 4, 3), np.uint8), mode="otsu", frames="gpu")
