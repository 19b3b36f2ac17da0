"""process_folder(deflate="device") on the CPU: the walk's side of the compressed hand-over.  The flow models are TEST DOUBLES (the
product's model has no CPU path): their study_chunks and held_deflate are numpy + zlib.compress(chunk, 9) over analysis.chunks_record,
and the one that serves deflate="device" RAISES from every float16 and float32 study call that would hand an array over.  The yardstick is
the deflate="host" walk of the same studies: the files must be the same byte for byte (tests/payload_cases.py same_file).
h5py lives only in the image's second interpreter, so the walks run there, started with a plain environment."""
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
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
from tee_optical_flow_amd import pipeline, hdf5_out, masks as masks_mod
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.frames import rgb2gray
from tee_optical_flow_amd.pipeline import process_folder, read_study
from tee_optical_flow_amd.synth import speckle_sequence
from tests.payload_cases import same_file

def _flow32(rgb, scale, sal=False, bkgd=None):
    g = rgb[..., 1 if sal else 0].astype(np.float32)
    d = (g[1:] - g[:-1]) / (48 if sal else 64)
    f = np.stack([d, -0.5 * d], -1)
    if bkgd is not None:
        f = f - np.array([f[k][bkgd[0]].mean() for k in range(len(f))], np.float32)[:, None, None, None]
    f = f * np.float32(scale)
    return np.concatenate([f, f[-1:]])

def _record(arr, chunks):
    stored = []
    for off in itertools.product(*[range(0, s, c) for s, c in zip(arr.shape, chunks)]):
        full = np.zeros(chunks, arr.dtype)
        blk = arr[tuple(slice(o, min(o + c, s)) for o, c, s in zip(off, chunks, arr.shape))]
        full[tuple(slice(0, n) for n in blk.shape)] = blk
        stored.append((off, 0, zlib.compress(full.tobytes(), 9)))
    return A.chunks_record(arr.shape, arr.dtype, chunks, stored)

class Fake:
    # arrays: the float16 study calls hand arrays over (the deflate="host" yardstick, and the fallbacks); without it they raise unless
    # the call holds.  chunks: study_chunks is offered.  bad: the n-th study_chunks call returns a flow record of other chunks.
    device_unit_scale = device_payload = device_wase = True
    def __init__(self, arrays=False, chunks=True, bad=None):
        self.log, self.arrays, self.device_study_chunks, self.bad, self.held, self.n = [], arrays, chunks, bad, None, 0
    def _payload(self, name, rgb, scale, sal=False, bkgd=None, hold=False):
        self.log.append(name + ("+hold" if hold else ""))
        if not (self.arrays or hold):
            raise RuntimeError(f"{name}: a float16 array was asked for under deflate='device'")
        assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
        pair = _flow32(rgb, scale, sal, bkgd).astype(np.float16), rgb2gray(rgb).astype(np.float16)
        if hold: self.held = pair
        return pair
    def calc_study_payload(self, rgb, scale=1.0, pad_last=True, echo=True, hold=False):
        return self._payload("calc_study_payload", rgb, scale, hold=hold)
    def submit_study_payload(self, rgb, scale=1.0, pad_last=True, echo=True):
        self.n += 1; self.jobs = getattr(self, "jobs", {}); self.jobs[self.n] = self._payload("submit_study_payload", rgb, scale); return self.n
    def wait(self, t): return self.jobs.pop(t)
    def calc_study_saliency_payload(self, rgb, scale=1.0, pad_last=True, echo=True, map_dtype="f32", hold=False):
        return self._payload("calc_study_saliency_payload", rgb, scale, sal=True, hold=hold)
    def calc_study_wase_payload(self, rgb, bkgd, scale=1.0, pad_last=True, echo=True, hold=False):
        return self._payload("calc_study_wase_payload", rgb, scale, bkgd=bkgd, hold=hold) + (np.zeros(len(rgb) - 1, np.float32),)
    def held_deflate(self, what, chunks):
        self.log.append("held_deflate:" + what)
        return _record(self.held[0 if what == "flow" else 1], tuple(chunks))
    def study_chunks(self, rgb, scale, flow_chunks, echo_chunks=None, chain=False):
        self.log.append("study_chunks"); self.n += 1
        assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3 and echo_chunks is not None
        flow = _flow32(rgb, scale).astype(np.float16)
        if self.bad == self.n:
            flow_chunks = (1,) + tuple(flow_chunks)[1:]
        return {"flow": _record(flow, tuple(flow_chunks)), "echo": _record(rgb2gray(rgb).astype(np.float16), tuple(echo_chunks))}
    def _no(self, *a, **k): raise RuntimeError("a float32 study call was used under payload='device'")
    calc_study = calc_study_saliency = submit_study = calc_batch = calc_study_wase = _no
    def close(self): pass

class PayloadOnly(Fake):                 # the float16 study calls and neither route to the chunks
    study_chunks = held_deflate = property()
    def __init__(self): Fake.__init__(self, arrays=True, chunks=False)

class GrayFake(Fake):                    # frames that are not uint8 RGB take the host path: calc_batch on the conditioned frames
    def calc_batch(self, frames, scale=1.0):
        self.log.append("calc_batch")
        d = (frames[1:].astype(np.float32) - frames[:-1].astype(np.float32)) / 64
        return np.stack([d, -0.5 * d], -1) * np.float32(scale)

def fake_predict_movie(nparr, segmentor_model, mode="A4C", verbose=True, config=None, engine=None):
    g = np.asarray(nparr)[..., 0]
    return {"bkgd": np.repeat((g < 90)[..., None], 2, axis=3), "rv": np.repeat((g > 150)[..., None], 2, axis=3)}
masks_mod.predict_movie = fake_predict_movie

def dying_reader(path):                  # picklable; the worker PROCESS that is asked for s2 dies; in a thread of the caller it reads
    import multiprocessing
    if multiprocessing.parent_process() is not None and path.endswith("s2.npz"):
        os._exit(3)
    return read_study(path)

messages = []
class Grab(logging.Handler):
    def emit(self, rec): messages.append((rec.levelno, rec.getMessage()))
pipeline.logger.addHandler(Grab()); pipeline.logger.setLevel(logging.INFO)

# what the parent process sees: the writer's zlib calls (thread mode), what is handed to the writer stage, the blocks it creates
class CountingZlib:
    calls = 0
    def compress(self, *a, **k): CountingZlib.calls += 1; return zlib.compress(*a, **k)
    def __getattr__(self, name): return getattr(zlib, name)
hdf5_out.zlib = CountingZlib()
handed, created = [], []
def big_f16(x):
    if isinstance(x, np.ndarray): return x.dtype == np.float16 and x.nbytes >= 1024
    if pipeline._is_shm(x): return np.dtype(x[3]) == np.float16
    if isinstance(x, dict): return any(big_f16(v) for v in x.values())
    if isinstance(x, (tuple, list)): return any(big_f16(v) for v in x)
    return False
def spy(real):
    def submit(self, fn, *args, **kwargs):
        # the writer stage's two callables: the hand-over record's write (threads), _save_study_shm of a packed record (processes)
        rec = args[0] if fn is pipeline._save_study_shm else getattr(fn, "__self__", None) if getattr(fn, "__func__", None) is pipeline._HandOver.write else None
        if rec is not None:
            assert isinstance(rec, pipeline._HandOver) and len(args) == (1 if fn is pipeline._save_study_shm else 0) and not kwargs
            handed.append({"pool": "process" if isinstance(self, ProcessPoolExecutor) else "thread", "f16": big_f16(vars(rec)),
                           "described": [type(a).__name__ for a in (rec.flow, rec.echo) if isinstance(a, hdf5_out.Described)]})
        return real(self, fn, *args, **kwargs)
    return submit
ProcessPoolExecutor.submit = spy(ProcessPoolExecutor.submit)
ThreadPoolExecutor.submit = spy(ThreadPoolExecutor.submit)
real_new = pipeline._shm_new
def spy_new(shape, dtype):
    got = real_new(shape, dtype)
    if got[1] is not None: created.append((tuple(int(v) for v in shape), np.dtype(dtype).str))
    return got
pipeline._shm_new = spy_new

def shm_now(): return set(os.listdir("/dev/shm")) if os.path.isdir("/dev/shm") else set()
def chunk_counts(folder):
    n = {"payload": 0, "masks": 0}
    for name in sorted(os.listdir(folder)):
        with h5py.File(os.path.join(folder, name), "r") as f:
            for k in f:
                n["payload" if k in ("flow", "echo") else "masks"] += f[k].id.get_num_chunks() if f[k].nbytes >= hdf5_out.MIN_PARALLEL_BYTES else 0
    return n
def same_files(a, b, names=None):
    if names is None:
        names = sorted(os.listdir(a))
        if names != sorted(os.listdir(b)) or len(names) != 3:
            return False
    return all(same_file(os.path.join(a, n), os.path.join(b, n)) for n in names)

def study(seed, n, h, w, gray=False):
    rng = np.random.default_rng(seed)
    g = speckle_sequence(seed, n, h, w)
    rgb = np.stack([g, np.roll(g, 3, axis=2), rng.integers(0, 256, g.shape, dtype=np.uint8)], -1)
    return rgb.astype(np.uint16) if gray else rgb         # (a gray uint8 stack is made RGB by the walk itself: uint16 frames are what is not uint8 RGB)

if __name__ == "__main__":
    big, small, gray = (os.path.join(TMP, n) for n in ("big", "small", "gray"))
    for folder, shape, is_gray in ((big, (9, 240, 256), False), (small, (5, 48, 56), False), (gray, (9, 240, 256), True)):
        os.makedirs(folder)
        for k in range(3):
            np.savez(os.path.join(folder, f"s{k}.npz"), nparr=study(800 + k, *shape, gray=is_gray), pixel_spacing=0.05, frame_rate=40.0, patient_id=f"P{k}", heart_rate=70)
    base = dict(nchunks=1, chunk_index=0, verbose=False, extensions=("npz",), payload="device")
    otsu, seg = dict(mode="otsu"), dict(mode="RVIO_2class")
    proc, thr = dict(workers="process", n_readers=2, n_writers=2), dict(workers="thread")
    out = {"walks": {}, "same": {}}
    def walk(tag, src, model, **more):
        del messages[:], handed[:], created[:]
        CountingZlib.calls = 0
        dst = os.path.join(TMP, tag)
        errs = process_folder(src, dst, object() if more.get("mode") == "RVIO_2class" else None, flow_model=model, **{**base, **more})
        out["walks"][tag] = {"errors": errs, "log": model.log, "zlib": CountingZlib.calls, "handed": list(handed), "created": list(created),
                             "warnings": [m for lv, m in messages if lv >= logging.WARNING], "info": [m for lv, m in messages if lv == logging.INFO],
                             "chunks": chunk_counts(dst), "files": sorted(os.listdir(dst))}
        return dst
    shm_before = shm_now()
    # the larger set: flow and echo are handed to HDF5 as whole chunks
    for kind, more in (("plain", otsu), ("sal", dict(no_saliency=False, **otsu)), ("wase", dict(bkgd_comp="WASE", **seg))):
        host = walk(f"{kind}_host", big, Fake(arrays=True), deflate="host", **thr, **more)
        for mode_tag, mode in (("thr", thr), ("prc", proc)):
            dev = walk(f"{kind}_dev_{mode_tag}", big, Fake(), deflate="device", **mode, **more)
            out["same"][f"{kind}_dev_{mode_tag}"] = same_files(host, dev)
    out["same"]["sal_differs"] = not same_files(os.path.join(TMP, "plain_host"), os.path.join(TMP, "sal_host"))
    # the smaller set: both under min_parallel_bytes, HDF5's own filter, the host path
    s_host = walk("small_host", small, Fake(arrays=True), deflate="host", **thr, **otsu)
    out["same"]["small_dev_thr"] = same_files(s_host, walk("small_dev_thr", small, Fake(arrays=True), deflate="device", **thr, **otsu))
    out["same"]["small_dev_prc"] = same_files(s_host, walk("small_dev_prc", small, Fake(arrays=True), deflate="device", **proc, **otsu))
    # fallbacks: a model with neither route; frames that are not uint8 RGB
    p_host = os.path.join(TMP, "plain_host")
    out["same"]["fb_model"] = same_files(p_host, walk("fb_model", big, PayloadOnly(), deflate="device", **thr, **otsu))
    g_host = walk("gray_host", gray, GrayFake(arrays=True), deflate="host", **thr, **otsu)
    out["same"]["fb_gray"] = same_files(g_host, walk("fb_gray", gray, GrayFake(), deflate="device", **thr, **otsu))
    # a record that does not fit its dataset: that study fails in the writer stage, the walk goes on
    for mode_tag, mode in (("thr", thr), ("prc", proc)):
        bad = walk(f"bad_{mode_tag}", big, Fake(bad=2), deflate="device", **mode, **otsu)
        out["same"][f"bad_{mode_tag}"] = same_files(p_host, bad, names=["s0.hdf5", "s2.hdf5"])
    # a worker process dies mid-walk: the stages go on in threads
    died = walk("died", big, Fake(), deflate="device", workers="process", n_readers=1, n_writers=2, reader=dying_reader, **otsu)
    out["same"]["died"] = same_files(p_host, died)
    out["shm_left"] = sorted(shm_now() - shm_before)
    try:
        process_folder(big, os.path.join(TMP, "cfg"), None, flow_model=Fake(), **{**base, "payload": "host", "deflate": "device"}, **otsu)
        out["config"] = "no error"
    except Exception as e:
        out["config"] = f"{type(e).__name__}: {e}"
    print(json.dumps(out, default=str))
"""


def _run(tmp_path, text, name, env):
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    script = tmp_path / name
    script.write_text(text.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp_path))))
    r = subprocess.run([PY_H5, str(script)], capture_output=True, text=True, timeout=900,
                       env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1", **env})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "leaked shared_memory" not in r.stderr, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("walk_deflate"), DRIVER, "walks.py", {"TEEFLOW_SHM_MIN_BYTES": "1024"})


KINDS = ("plain", "sal", "wase")
DEV = [f"{k}_dev_{m}" for k in KINDS for m in ("thr", "prc")]


def test_device_deflate_walk_writes_the_host_walks_files(walks):
    """Threads or 2 + 2 worker processes; the plain branch through study_chunks, no_saliency=False and bkgd_comp="WASE" through the payload
    call with hold=True and held_deflate: every file has the bytes of the deflate="host" walk's."""
    for tag in DEV + [f"{k}_host" for k in KINDS]:
        w = walks["walks"][tag]
        assert w["errors"] == [] and w["files"] == ["s0.hdf5", "s1.hdf5", "s2.hdf5"] and not w["warnings"], (tag, w)
    assert all(walks["same"][tag] for tag in DEV) and walks["same"]["sal_differs"], walks["same"]
    for m in ("thr", "prc"):
        assert walks["walks"][f"plain_dev_{m}"]["log"] == ["study_chunks"] * 3
        assert walks["walks"][f"sal_dev_{m}"]["log"] == ["calc_study_saliency_payload+hold", "held_deflate:flow", "held_deflate:echo"] * 3
        assert walks["walks"][f"wase_dev_{m}"]["log"] == ["calc_study_wase_payload+hold", "held_deflate:flow", "held_deflate:echo"] * 3
    # the host walk submits its solves (studies_in_flight=2); a device-deflate study is solved synchronously, and the walk says so once
    assert walks["walks"]["plain_host"]["log"] == ["submit_study_payload"] * 3
    said = [m for m in walks["walks"]["plain_dev_thr"]["info"] if "studies_in_flight" in m]
    assert len(said) == 1 and "no effect" in said[0]
    # the studies are what the issue asks for: flow and echo are handed to HDF5 as whole chunks
    assert walks["walks"]["plain_host"]["chunks"]["payload"] > 0


def test_writer_stage_compresses_the_masks_only(walks):
    """Thread mode, where the counting zlib wrapper of hdf5_out sees the writer stage: the host walk compresses every chunk of flow, echo
    and masks, the device walk exactly the masks' chunks."""
    for k in KINDS:
        host, dev = walks["walks"][f"{k}_host"], walks["walks"][f"{k}_dev_thr"]
        assert host["chunks"] == dev["chunks"] and dev["chunks"]["masks"] > 0 and dev["chunks"]["payload"] > 0
        assert host["zlib"] == host["chunks"]["payload"] + host["chunks"]["masks"], (k, host["zlib"], host["chunks"])
        assert dev["zlib"] == dev["chunks"]["masks"], (k, dev["zlib"], dev["chunks"])


def test_no_float16_array_reaches_the_writer_stage(walks):
    """The hand-over record the writer stage gets, in its thread pool or (through _save_study_shm) its process pool: two Described and no
    float16 array or float16 shared-memory block; the blocks the walk creates per study are the two blobs."""
    for tag in DEV:
        w = walks["walks"][tag]
        assert len(w["handed"]) == 3, (tag, w["handed"])
        for h in w["handed"]:
            assert h["pool"] == ("process" if tag.endswith("prc") else "thread")
            assert not h["f16"] and h["described"] == ["Described", "Described"], (tag, h)
    for k in KINDS:
        w = walks["walks"][f"{k}_dev_prc"]
        assert len(w["created"]) == 6 and all(len(shape) == 1 and dt == "|u1" for shape, dt in w["created"]), w["created"]
        assert walks["walks"][f"{k}_dev_thr"]["created"] == []
    host = walks["walks"]["plain_host"]
    assert all(h["f16"] and not h["described"] for h in host["handed"]) and len(host["handed"]) == 3


def test_small_datasets_go_through_hdf5s_own_filter(walks):
    """flow and echo under create_gzip9's min_parallel_bytes are not asked of the deflater: such a study takes the host path (its
    arrays are needed), says why once per walk, and the files are the host's."""
    assert walks["same"]["small_dev_thr"] and walks["same"]["small_dev_prc"]
    for tag in ("small_dev_thr", "small_dev_prc"):
        w = walks["walks"][tag]
        assert w["errors"] == [] and w["log"] == ["submit_study_payload"] * 3 and w["chunks"]["payload"] == 0, w
        said = [m for m in w["warnings"] if "deflate='device' not used" in m]
        assert len(said) == 1 and "min_parallel_bytes" in said[0], w["warnings"]


def test_fallbacks_say_why_once_per_walk(walks):
    assert walks["same"]["fb_model"] and walks["same"]["fb_gray"]
    w = walks["walks"]["fb_model"]
    said = [m for m in w["warnings"] if "deflate='device' not used" in m]
    assert w["errors"] == [] and w["log"] == ["submit_study_payload"] * 3 and len(said) == 1 and "PayloadOnly" in said[0] and "neither" in said[0], w
    w = walks["walks"]["fb_gray"]
    said = [m for m in w["warnings"] if "deflate='device' not used" in m]
    assert w["errors"] == [] and w["log"] == ["calc_batch"] * 3 and len(said) == 1 and "not uint8 RGB" in said[0], w
    assert walks["config"].startswith("ConfigurationError") and "payload='device'" in walks["config"]


def test_a_record_that_does_not_fit_fails_its_study_alone(walks):
    for tag in ("bad_thr", "bad_prc"):
        w = walks["walks"][tag]
        assert len(w["errors"]) == 1 and w["errors"][0][0] == "s1.hdf5" and w["errors"][0][1].startswith("OpticalFlowError"), w["errors"]
        assert "deflater's record of 'flow'" in w["errors"][0][1]
        assert w["files"] == ["s0.hdf5", "s2.hdf5"] and walks["same"][tag]


def test_a_dead_worker_switches_to_threads_and_leaves_no_block(walks):
    w = walks["walks"]["died"]
    assert w["errors"] == [] and walks["same"]["died"] and w["log"] == ["study_chunks"] * 3
    assert any("continue in threads" in m for m in w["warnings"]), w["warnings"]
    assert {h["pool"] for h in w["handed"]} == {"process", "thread"}     # mid-walk: both kinds of writer were used
    assert walks["shm_left"] == [], "shared-memory blocks left behind"


class _Model:
    """a model with the float16 study calls, held_deflate and (chunks=True) study_chunks, in numpy: zeros, and records of no chunks"""
    device_unit_scale = device_payload = device_wase = True

    def __init__(self, chunks):
        self.device_study_chunks, self.log = chunks, []

    def calc_batch(self, frames):
        self.log.append("calc_batch")
        return np.zeros((len(frames) - 1,) + frames.shape[1:3] + (2,), np.float32)

    def calc_study_payload(self, rgb, scale=1.0, pad_last=True, echo=True, hold=False):
        self.log.append("calc_study_payload" + ("+hold" if hold else ""))
        return np.zeros(rgb.shape[:3] + (2,), np.float16), np.zeros(rgb.shape[:3], np.float16)

    def held_deflate(self, what, chunks):
        self.log.append("held_deflate:" + what)
        return {"blob": np.zeros(3, np.uint8), "chunks": chunks}

    def study_chunks(self, rgb, scale, flow_chunks, echo_chunks=None, chain=False):
        self.log.append("study_chunks")
        return {"flow": {"blob": np.zeros(3, np.uint8), "chunks": flow_chunks}, "echo": {"blob": np.zeros(3, np.uint8), "chunks": echo_chunks}}


@pytest.mark.parametrize("route,shape,kw,log", [
    ("host", (5, 48, 56), dict(payload="host"), ["calc_batch"]),
    ("device", (5, 48, 56), dict(payload="device"), ["calc_study_payload"]),
    ("hold", (9, 240, 256), dict(payload="device", deflate="device"), ["calc_study_payload+hold", "held_deflate:flow", "held_deflate:echo"]),
    ("chunks", (9, 240, 256), dict(payload="device", deflate="device"), ["study_chunks"])])
def test_the_hook_gets_the_hand_over_record_alone(monkeypatch, route, shape, kw, log):
    """On every route _defer_save is called once, with exactly one positional argument: the hand-over record.  flow and echo in it are
    arrays where the host compresses them, and Described beside their two records where the device did (9 x 240 x 256: both past
    create_gzip9's min_parallel_bytes)."""
    from tee_optical_flow_amd import hdf5_out, pipeline
    monkeypatch.setattr(hdf5_out, "auto_chunks", lambda shape, dtype: (1,) + tuple(shape[1:]))
    calls = []
    model = _Model(chunks=route == "chunks")
    rgb = np.full(shape + (3,), 9, np.uint8)
    flow = pipeline.process_video(None, "unwritten.hdf5", None, verbose=False, mode="otsu", no_saliency=True, nparr=rgb, flow_model=model,
                                  mask_dict={"otsu": np.zeros(shape + (1,), bool)}, _defer_save=lambda *a, **k: calls.append((a, k)), **kw)
    assert model.log == log
    (args, kwargs), = calls
    assert len(args) == 1 and not kwargs and type(args[0]) is pipeline._HandOver, calls
    out = args[0]
    assert out.save_path == "unwritten.hdf5" and out.nparr is rgb and list(out.mask_dict) == ["otsu"] and out.deflater is None and out.flow is flow
    if route in ("hold", "chunks"):
        assert sorted(out.records) == ["echo", "flow"] and out.records["flow"]["chunks"] == (1,) + shape[1:] + (2,)
        assert isinstance(out.flow, hdf5_out.Described) and (out.flow.shape, out.flow.dtype) == (shape + (2,), np.float16)
        assert isinstance(out.echo, hdf5_out.Described) and (out.echo.shape, out.echo.dtype) == (shape, np.float16)
    else:
        assert out.records == {} and out.flow.shape == shape + (2,) and out.flow.dtype == (np.float16 if route == "device" else np.float32)
        assert (out.echo is None) if route == "host" else (out.echo.shape == shape and out.echo.dtype == np.float16)


def test_process_folder_takes_deflate():
    """(fails without the feature: process_folder(deflate=...) is a TypeError)"""
    import inspect
    from tee_optical_flow_amd.exceptions import ConfigurationError
    from tee_optical_flow_amd.pipeline import process_folder
    assert inspect.signature(process_folder).parameters["deflate"].default == "host"
    with pytest.raises(ConfigurationError, match="deflate"):
        process_folder("unused", "unused", None, payload="device", deflate="bogus")
    with pytest.raises(ConfigurationError, match="needs payload='device'"):
        process_folder("unused", "unused", None, deflate="device")
