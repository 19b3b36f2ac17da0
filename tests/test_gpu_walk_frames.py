"""process_video / process_folder(frames="device") on the real engine: .npz studies of every `photometric` value, with and without
flipLR, through both walks -- what reaches the HDF5 writer (captured in its place: h5py is not in this interpreter) and what
process_video returns must be the same arrays, the host side converting with the twin.  The CPU twin of this file
(tests/test_walk_frames_cpu.py) compares the written files."""
import os

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import hdf5_out, pipeline

pytestmark = pytest.mark.gpu
KINDS = ["RGB", "YBR_FULL", "YBR_FULL_422", "MONOCHROME2", None]


def _stored(seed, photometric, n=5, h=40, w=56):
    from tee_optical_flow_amd.synth import speckle_sequence
    rng = np.random.default_rng(seed)
    g = speckle_sequence(seed, n, h, w)
    if photometric == "MONOCHROME2":
        return g
    if photometric in ("RGB", None):
        return np.stack([g, np.roll(g, 3, axis=2), rng.integers(0, 256, g.shape, dtype=np.uint8)], -1)
    return np.stack([g, rng.integers(64, 192, g.shape, dtype=np.uint8), rng.integers(64, 192, g.shape, dtype=np.uint8)], -1)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    src = tmp_path_factory.mktemp("frames_walk_in")
    for k, ph in enumerate(KINDS):
        extra = {} if ph is None else {"photometric": ph}
        np.savez(src / f"s{k}.npz", nparr=_stored(300 + k, ph), pixel_spacing=0.05, frame_rate=40.0, patient_id=f"P{k}", **extra)
    return str(src)


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0, max_batch=3)
    yield e
    e.close()


def _same(a, b, what):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            _same(a[k], b[k], f"{what}/{k}")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("payload", ["host", "device"])
def test_process_video(eng, folder, flip, payload):
    for k, ph in enumerate(KINDS):
        path = os.path.join(folder, f"s{k}.npz")
        up = eng.counter("frames_upload_bytes")
        dev = pipeline.process_video(path, None, mode="otsu", flipLR=flip, no_saliency=True, flow_model=eng, payload=payload, frames="device")
        assert eng.counter("frames_upload_bytes") - up == np.load(path)["nparr"].nbytes, ph          # once, as stored
        host = pipeline.process_video(path, None, mode="otsu", flipLR=flip, no_saliency=True, flow_model=eng, payload=payload, frames="host")
        _same(dev, host, f"{ph} flip={flip} payload={payload}")
        assert np.abs(np.asarray(dev, np.float32)).max() > 0


@pytest.mark.parametrize("kw", [dict(payload="host"), dict(payload="device", flipLR=True), dict(payload="device", studies_in_flight=1)],
                         ids=["host-payload", "device-payload-flip", "one-in-flight"])
def test_process_folder(eng, folder, tmp_path, monkeypatch, kw):
    written = {}

    def capture(save_path, flow, nparr, mask_dict, metadata, waveforms, patient_id, heart_rate, config, mode, no_saliency, include_waveforms,
                save_mask_subset=None, *, echo=None, nframes=None, deflate=None):
        from tee_optical_flow_amd.frames import rgb2gray
        written[os.path.basename(save_path)] = {"flow": np.asarray(flow, np.float16), "masks": {k: np.array(v) for k, v in mask_dict.items()},
                                                "echo": np.array(echo) if echo is not None else rgb2gray(nparr).astype(np.float16),
                                                "nframes": int(nframes) if nframes is not None else nparr.shape[0], "patient": patient_id}
    monkeypatch.setattr(hdf5_out, "save_optical_flow_to_hdf5", capture)
    got = {}
    for frames in ("host", "device"):
        written.clear()
        errs = pipeline.process_folder(folder, str(tmp_path / frames), None, nchunks=1, chunk_index=0, mode="otsu", otsu_masks="device", verbose=False,
                                       extensions=("npz",), workers="thread", flow_model=eng, frames=frames, **kw)
        assert errs == [] and len(written) == len(KINDS)
        got[frames] = dict(written)
    _same(got["device"], got["host"], "process_folder")
