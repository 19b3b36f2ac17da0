"""The folder walk's side of JPEG Lossless studies, without a GPU, with stand-in models: a 5-frame 24 x 32 JPEG Lossless .npz study must
give the files its decoded `nparr` gives, byte for byte -- frames="host" (the host decodes: PIL where it imports and takes the stream, else
the twin) and frames="device" (hold_frames_jpeg_lossless; the twin stands for the device) -- and a model without
hold_frames_jpeg_lossless, and a study the device gives a status for, take the host's decode with one logged reason per walk.  h5py lives
only in the image's second interpreter, so the walks run there."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_H5 = "/opt/conda/bin/python3.9"

DRIVER = r"""
import sys, json, os, logging, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tee_optical_flow_amd import pipeline, masks as masks_mod
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.dense_flow import HeldFrames
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
from tee_optical_flow_amd.pipeline import process_folder, process_video
from tests.payload_cases import same_file
from tests.frames_cases import NumpyFrames

def _flow32(rgb, scale):
    g = rgb[..., 0].astype(np.float32)
    d = (g[1:] - g[:-1]) / 64
    f = np.stack([d, -0.5 * d], -1) * np.float32(scale)
    return np.concatenate([f, f[-1:]])

class Plain:                              # no held frames: every frames argument is an array
    device_unit_scale = True
    device_id = 0
    def __init__(self): self.log, self.jobs, self.n = [], {}, 0
    def _rgb(self, frames, min_frames=1):
        assert not isinstance(frames, HeldFrames)
        return np.asarray(frames)
    def calc_study(self, frames, scale=1.0, pad_last=False):
        self.log.append("calc_study"); return _flow32(self._rgb(frames, 2), scale)
    def submit_study(self, frames, scale=1.0, pad_last=False):
        self.n += 1; self.log.append("submit_study"); self.jobs[self.n] = _flow32(self._rgb(frames, 2), scale); return self.n
    def wait(self, t): return self.jobs.pop(t)
    def otsu_masks(self, frames, min_size):
        self.log.append("otsu_masks")
        class Cfg: min_mask_size = min_size
        return masks_mod.predict_movie_thres(self._rgb(frames, 2), config=Cfg())["otsu"]
    def close(self): pass

class Holder(NumpyFrames, Plain):         # hold_frames & co.; a frames argument may be the token
    def __init__(self): NumpyFrames.__init__(self); Plain.__init__(self)
    def hold_frames(self, arr, form="RGB", flip=False):
        self.log.append(("hold_frames", form, bool(flip))); return NumpyFrames.hold_frames(self, arr, form, flip)
    def _rgb(self, frames, min_frames=1):
        return self.resolve(frames, min_frames)

class LosslessHolder(Holder):             # ... and hold_frames_jpeg_lossless: the compressed bytes cross the bus, the twin stands for the device
    def hold_frames_jpeg_lossless(self, record, H, W, samples, form="RGB", flip=False):
        blob, off, ln = record
        self.log.append(("hold_frames_jpeg_lossless", form, bool(flip), int(np.asarray(blob).size)))
        raw = np.asarray(blob, np.uint8).tobytes()
        dec = [F.jpegll_decode_frame(raw[int(o):int(o) + int(n)], H, W, samples) for o, n in zip(off, ln)]
        bad = [(i, st) for i, (_, st) in enumerate(dec) if st]
        if bad:
            raise OpticalFlowCalculationError(f"tf_hold_frames_jpegll: frame {bad[0][0]} did not decode: status {bad[0][1]}")
        up = self.uploads
        tok = NumpyFrames.hold_frames(self, np.stack([a for a, _ in dec]), form, flip)
        self.uploads = up + int(np.asarray(ln).sum())
        return tok

warnings = []
class Grab(logging.Handler):
    def emit(self, rec):
        if rec.levelno >= logging.WARNING: warnings.append(rec.getMessage())
pipeline.logger.addHandler(Grab())

def same_files(a, b):
    names = sorted(os.listdir(a))
    return bool(names) and names == sorted(os.listdir(b)) and all(same_file(os.path.join(a, n), os.path.join(b, n)) for n in names)

def study(seed, samples):
    # 5 frames of 24 x 32 that drift
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (24, 40, samples)).astype(np.uint8)
    g[:, :6] = 0
    dec = np.stack([g[:, i:i + 32] for i in range(5)])
    dec = dec[..., 0] if samples == 1 else dec
    return [F.jpegll_encode_frame(f, i % 3) for i, f in enumerate(dec)], np.ascontiguousarray(dec)

if __name__ == "__main__":
    tmp = TMP
    kinds = [(3, "RGB"), (3, "YBR_FULL"), (1, "MONOCHROME2"), (3, None)]         # (samples, photometric)
    dirs = {"arr": os.path.join(tmp, "in_arr"), "ll": os.path.join(tmp, "in_ll"), "bad": os.path.join(tmp, "in_bad")}
    for d in dirs.values(): os.makedirs(d)
    sizes = []
    for k, (samples, ph) in enumerate(kinds):
        bufs, dec = study(k, samples)
        blob, off, ln = F.jpegll_record(bufs)
        extra = dict(pixel_spacing=0.05, frame_rate=40.0, patient_id=f"P{k}", heart_rate=70)
        if ph is not None:
            extra["photometric"] = ph
        np.savez(os.path.join(dirs["arr"], f"s{k}.npz"), nparr=dec, **extra)
        np.savez(os.path.join(dirs["ll"], f"s{k}.npz"), jpegll_blob=blob, jpegll_off=off, jpegll_len=ln, rows=24, cols=32, samples=samples, **extra)
        sizes.append(int(blob.size))
    # a study whose last frame is cut in its entropy data: the device gives status 3, the host's decode is asked and finds the same
    bufs, dec = study(9, 3)
    cut = bufs[4][:len(bufs[4]) // 2]
    blob, off, ln = F.jpegll_record(bufs[:4] + [cut])
    np.savez(os.path.join(dirs["bad"], "s0.npz"), jpegll_blob=blob, jpegll_off=off, jpegll_len=ln, rows=24, cols=32, samples=3, photometric="RGB")
    out = {"sizes": sizes, "walks": {}, "same": {}, "video": {}}
    base = dict(nchunks=1, chunk_index=0, verbose=False, extensions=("npz",), workers="thread", mode="otsu", otsu_masks="device", no_saliency=True)

    def walk(tag, src, model, **more):
        del warnings[:]
        errs = process_folder(dirs[src], os.path.join(tmp, tag), None, flow_model=model, **{**base, **more})
        out["walks"][tag] = {"errors": errs, "log": [list(x) if isinstance(x, tuple) else x for x in model.log], "warnings": list(warnings),
                             "uploads": getattr(model, "uploads", None), "left": len(model.jobs)}
        return os.path.join(tmp, tag)

    for flip in (False, True):
        f = "_flip" if flip else ""
        want = walk("arr_host" + f, "arr", Plain(), frames="host", flipLR=flip)
        out["same"]["host" + f] = same_files(want, walk("ll_host" + f, "ll", Plain(), frames="host", flipLR=flip))
        out["same"]["device" + f] = same_files(want, walk("ll_dev" + f, "ll", LosslessHolder(), frames="device", flipLR=flip))
    want = os.path.join(tmp, "arr_host")
    out["same"]["no_ll_model"] = same_files(want, walk("fb_no_ll", "ll", Holder(), frames="device"))    # hold_frames, but no hold_frames_jpeg_lossless
    out["same"]["no_hold_model"] = same_files(want, walk("fb_plain", "ll", Plain(), frames="device"))
    walk("fb_status", "bad", LosslessHolder(), frames="device")                   # the device gives a status: the host's decode is asked, once
    for k in range(len(kinds)):
        a, b, c = (os.path.join(tmp, f"pv_{t}_{k}.hdf5") for t in "abc")
        m = LosslessHolder()
        fa = process_video(os.path.join(dirs["arr"], f"s{k}.npz"), a, mode="otsu", no_saliency=True, flow_model=Plain(), frames="host", flipLR=True)
        fb = process_video(os.path.join(dirs["ll"], f"s{k}.npz"), b, mode="otsu", no_saliency=True, flow_model=Plain(), frames="host", flipLR=True)
        fc = process_video(os.path.join(dirs["ll"], f"s{k}.npz"), c, mode="otsu", no_saliency=True, flow_model=m, frames="device", flipLR=True)
        out["video"][k] = [same_file(a, b), same_file(a, c), bool(np.array_equal(fa, fb) and np.array_equal(fa, fc)), m.log[0], m.uploads]
    print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    tmp = tmp_path_factory.mktemp("jpegll_walk")
    script = tmp / "walks.py"
    script.write_text(DRIVER.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp))))
    r = subprocess.run([PY_H5, str(script)], capture_output=True, text=True, timeout=600, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


HOLDS = ["RGB", "YBR_FULL", "GRAY", "RGB"]                                  # s0 .. s3


def test_jpeg_lossless_studies_write_the_decoded_studies_files(walks):
    ok = {k: w["errors"] for k, w in walks["walks"].items() if w["errors"] and k != "fb_status"}
    assert not ok, ok
    assert len(walks["same"]) == 6 and all(walks["same"].values()), walks["same"]
    for k, (host, dev, flows, first, uploads) in walks["video"].items():
        assert host and dev and flows, (k, walks["video"][k])
        assert first == ["hold_frames_jpeg_lossless", HOLDS[int(k)], True, walks["sizes"][int(k)]] and uploads == walks["sizes"][int(k)], (k, first, uploads)


def test_the_device_walk_holds_each_study_from_its_compressed_bytes(walks):
    for tag, flip in (("ll_dev", False), ("ll_dev_flip", True)):
        w = walks["walks"][tag]
        holds = [x for x in w["log"] if isinstance(x, list)]
        assert holds == [["hold_frames_jpeg_lossless", form, flip, size] for form, size in zip(HOLDS, walks["sizes"])], (tag, holds)
        assert w["uploads"] == sum(walks["sizes"]) and not w["warnings"] and w["left"] == 0, (tag, w)
    for tag in ("ll_host", "arr_host"):
        assert not any(isinstance(x, list) for x in walks["walks"][tag]["log"]) and not walks["walks"][tag]["warnings"]


def test_the_fallback_says_why_once_per_walk(walks):
    w = walks["walks"]["fb_no_ll"]                                          # the host decodes, the decoded array is held as ever
    assert len(w["warnings"]) == 1 and w["warnings"][0].startswith("JPEG Lossless pixel data not decoded on the device, the host decodes it instead: ")
    assert "has no hold_frames_jpeg_lossless" in w["warnings"][0]
    assert [x[:2] for x in w["log"] if isinstance(x, list)] == [["hold_frames", form] for form in HOLDS]
    w = walks["walks"]["fb_plain"]
    assert len(w["warnings"]) == 2 and any("has no hold_frames_jpeg_lossless" in x for x in w["warnings"])
    assert any("has no hold_frames" in x and "frames='device' not used" in x for x in w["warnings"])
    w = walks["walks"]["fb_status"]                                         # a frame cut short: the device's status, then the host's decode finds the same
    said = [x for x in w["warnings"] if "the host decodes it instead" in x]
    assert len(said) == 1 and "the device did not decode it" in said[0] and "frame 4 did not decode: status 3" in said[0]
    assert len(w["errors"]) == 1 and "JPEG Lossless frame 4 did not decode" in str(w["errors"])
