"""DICOM RLE Lossless without a GPU: the Python twin (frames.rle_decode_frame) against the independent decoder of tests/rle_cases.py and
the known answers, the encoder, the encapsulated format, dicom_rle_frames on stub datasets, the core and the planar ingest under the
sanitizers (tests/csrc/verify_rle.cpp: a stand-alone program with exact-size buffers), and the walk's side with stand-in models: an RLE
.npz study must give the files its decoded `nparr` gives, byte for byte.  h5py lives only in the image's second interpreter, so the walks
run there."""
import json
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd import pipeline as P
from tee_optical_flow_amd.exceptions import DICOMReadError

from tests import rle_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_H5 = "/opt/conda/bin/python3.9"


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    for seg, want in RC.KNOWN:
        assert RC.reference_segment(seg) == want
        plane, full = F._rle_segment(seg, len(want))
        assert full and bytes(plane) == want
        if want:
            got, status = F.rle_decode_frame(RC.make_frame([seg]), 1, len(want), 1)
            assert status == 0 and got.tobytes() == want
            assert F.rle_decode_frame(RC.make_frame([seg]), 1, len(want) + 1, 1)[1] == 3      # one byte more is a byte short


def test_twin_agrees_with_the_independent_decoder_on_the_whole_corpus():
    want, seen = RC.expected(), {0: 0, 1: 0, 2: 0, 3: 0}
    for c in RC.corpus():
        arr, status = want[c.name]
        got, got_status = F.rle_decode_frame(c.buf, c.H, c.W, c.samples)
        assert got_status == status, (c.name, got_status, status)
        assert got.shape == ((c.H, c.W) if c.samples == 1 else (c.H, c.W, c.samples)) and got.dtype == np.uint8
        assert np.array_equal(got, arr) if status == 0 else not got.any(), c.name
        seen[status] += 1
    assert all(seen.values()), seen                                        # the corpus has every status
    assert len(RC.corpus()) == len(want) and len(want) > RC.T              # no two cases share a name


def test_the_corpus_says_what_its_names_promise():
    want = RC.expected()
    status = lambda name: want[name][1]
    assert all(status(n) == 1 for n in want if n.startswith(("bad_short_frame", "bad_count")))
    assert all(status(n) == 2 for n in want if n.startswith(("bad_offset_", "bad_offsets_")))
    assert all(status(n) == 0 for n in want if n.startswith(("enc_", "stage_noops_", "hand_gaps_", "hand_first_offset_")))
    for n in ("literal_cut_short", "run_without_value", "only_noops", "one_byte_short", "middle_plane_short", "last_plane_short"):
        assert status("hand_" + n) == 3, n
    for n in ("run_crosses_rows", "literal_crosses_rows", "noops_between", "odd_then_pad", "garbage_after", "garbage_is_a_cut_literal",
              "garbage_is_a_lone_run", "overlong_run_is_clipped", "overlong_literal_is_clipped", "literal_cut_but_enough", "three_planes"):
        assert status("hand_" + n) == 0, n
    cuts = [status(n) for n in want if n.startswith("cut_after_")]
    assert cuts[0] == 2 and 3 in cuts and cuts[-1] == 0                    # no segment byte left; short; only the pad missing
    assert np.array_equal(want["stage_noops_0"][0], want[f"stage_noops_{RC.T + 1}"][0])


def _tokens_stay_in_rows(seg, H, W):
    """a conformant segment: every literal and run lies in one row, and the plane ends with the stream or its one pad byte"""
    pos, made = 0, 0
    while made < H * W:
        c = seg[pos]
        cnt = c + 1 if c < 128 else 257 - c
        assert c != 128 and made // W == (made + cnt - 1) // W, (pos, made, cnt)
        pos += 1 + (cnt if c < 128 else 1)
        made += cnt
    return made == H * W and len(seg) - pos == (pos & 1) and not any(seg[pos:])


def test_encode_then_decode_is_the_identity_and_the_encoder_conforms():
    for c, frame in RC.encoded():
        got, status = F.rle_decode_frame(c.buf, c.H, c.W, c.samples)
        assert status == 0 and np.array_equal(got, frame), c.name
        head = struct.unpack_from("<16I", c.buf, 0)
        assert head[0] == c.samples and head[1] == 64 and not any(head[1 + c.samples:]), c.name
        ends = list(head[2:1 + c.samples]) + [len(c.buf)]
        for k in range(c.samples):
            seg = c.buf[head[1 + k]:ends[k]]
            assert len(seg) % 2 == 0 and _tokens_stay_in_rows(seg, c.H, c.W), (c.name, k)
    const = F.rle_encode_frame(np.full((2, 300), 9, np.uint8))             # 300 = 128 + 128 + 44 a row
    assert const[64:] == bytes([0x81, 9, 0x81, 9, 257 - 44, 9]) * 2
    with pytest.raises(ValueError):
        F.rle_encode_frame(np.zeros((2, 3), np.uint16))
    with pytest.raises(ValueError):
        F.rle_decode_frame(b"", 0, 3, 1)


def test_rle_record_lays_the_frames_end_to_end():
    blob, off, ln = F.rle_record([b"abc", b"", b"defgh"])
    assert blob.tobytes() == b"abcdefgh" and off.tolist() == [0, 3, 3] and ln.tolist() == [3, 0, 5]
    assert blob.dtype == np.uint8 and off.dtype == np.uint64 and ln.dtype == np.uint32


# ---- the encapsulated format ------------------------------------------------------------------------------------------------------------
def _item(data):
    return b"\xfe\xff\x00\xe0" + struct.pack("<I", len(data)) + data


END = b"\xfe\xff\xdd\xe0\x00\x00\x00\x00"


def test_encapsulated_frames():
    a, b, c, d = b"aaaa", b"bbbbbb", b"cc", b"dddddddd"
    assert F.encapsulated_frames(_item(b"") + _item(a) + _item(b) + END, 2) == [a, b]                       # an empty offset table
    table = struct.pack("<2I", 0, 8 + len(a))
    assert F.encapsulated_frames(_item(table) + _item(a) + _item(b) + END, 2) == [a, b]                     # a filled one, a fragment a frame
    table = struct.pack("<2I", 0, 16 + len(a) + len(b))
    assert F.encapsulated_frames(_item(table) + _item(a) + _item(b) + _item(c) + _item(d) + END, 2) == [a + b, c + d]   # two fragments a frame
    table = struct.pack("<2I", 0, 8 + len(a))
    assert F.encapsulated_frames(_item(table) + _item(a) + _item(b) + _item(c) + END, 2) == [a, b + c]      # ... or as the table says
    assert F.encapsulated_frames(_item(b"") + _item(a) + END + b"trailing", 1) == [a]
    for bad, n in ((_item(b"") + _item(a) + _item(b), 2),                                                   # no delimiter
                   (_item(b"") + _item(a) + _item(b) + _item(c) + END, 2),                                  # 3 fragments, 2 frames, no table
                   (_item(struct.pack("<2I", 0, 5)) + _item(a) + _item(b) + _item(c) + END, 2),             # a table that names no fragment
                   (_item(struct.pack("<I", 0)) + _item(a) + _item(b) + _item(c) + END, 2),                 # a table of one entry for 2 frames
                   (_item(b"") + b"\xfe\xff\x00\xe0" + struct.pack("<I", 99) + a + END, 1),                 # an item that passes the end
                   (_item(b"") + b"\xe0\x7f\x10\x00" + struct.pack("<I", 4) + a + END, 1),                  # not an item
                   (_item(b"abc") + _item(a) + _item(b) + _item(c) + END, 2), (END, 1), (b"", 1), (_item(b"") + _item(a) + END, 0)):
        with pytest.raises(ValueError):
            F.encapsulated_frames(bad, n)


# ---- dicom_rle_frames ---------------------------------------------------------------------------------------------------------------------
def _dataset(frames, samples, uid=F.RLE_TRANSFER_SYNTAX, bits=8, photometric="YBR_FULL", **more):
    enc = [F.rle_encode_frame(f) for f in frames]
    return SimpleNamespace(file_meta=SimpleNamespace(TransferSyntaxUID=uid), PixelData=_item(b"") + b"".join(_item(e) for e in enc) + END,
                           Rows=frames.shape[1], Columns=frames.shape[2], SamplesPerPixel=samples, BitsAllocated=bits,
                           PhotometricInterpretation=photometric, **more)


def test_dicom_rle_frames_on_stub_datasets():
    frames, (blob, off, ln) = RC.study("sector", 3, 37, 53, 3)
    got = P.dicom_rle_frames(_dataset(frames, 3, NumberOfFrames="3"))      # (NumberOfFrames is an IS: a string)
    assert isinstance(got, P.RleFrames) and got.shape == (3, 37, 53) and got.samples == 3 and got.photometric == "YBR_FULL"
    assert np.array_equal(got.blob, blob) and np.array_equal(got.off, off) and np.array_equal(got.len, ln)
    assert np.array_equal(got.decode(), frames) and P._rle_form(got, "YBR_FULL") == ("YBR_FULL", None) and P._rle_form(got, None) == ("RGB", None)
    grey, _ = RC.study("speckle", 1, 3, 5, 1)
    one = P.dicom_rle_frames(_dataset(grey, 1, photometric="MONOCHROME2"))   # no NumberOfFrames: one frame
    assert one.shape == (1, 3, 5) and one.samples == 1 and np.array_equal(one.decode(), grey)
    assert P._rle_form(one, None)[0] is None                               # (a grey stack of one frame stays grey)
    # refused: 16-bit samples, another transfer syntax, no file_meta -- read through pixel_array as ever
    assert P.dicom_rle_frames(_dataset(frames, 3, bits=16, NumberOfFrames=3)) is None
    assert "BitsAllocated = 16" in P._rle_refusal(_dataset(frames, 3, bits=16))
    assert P.dicom_rle_frames(_dataset(frames, 3, uid="1.2.840.10008.1.2.1", NumberOfFrames=3)) is None
    assert P.dicom_rle_frames(_dataset(frames, 3, uid="1.2.840.10008.1.2.4.50", NumberOfFrames=3)) is None
    assert P.dicom_rle_frames(SimpleNamespace(Rows=1, Columns=1)) is None
    with pytest.raises(ValueError):                                        # three fragments for two frames and no offset table
        P.dicom_rle_frames(_dataset(frames, 3, NumberOfFrames=2))
    bad = P.RleFrames(blob[:-40].copy(), off, np.array([ln[0], ln[1], ln[2] - 40], np.uint32), (3, 37, 53), 3)
    with pytest.raises(DICOMReadError, match="frame 2 did not decode: status 3"):
        bad.decode()


def test_npz_study_may_carry_rle_in_nparrs_place(tmp_path):
    frames, (blob, off, ln) = RC.study("sector", 4, 40, 64, 3)
    path = str(tmp_path / "s.npz")
    np.savez(path, rle_blob=blob, rle_off=off, rle_len=ln, rows=40, cols=64, samples=3, photometric="YBR_FULL", pixel_spacing=0.05, frame_rate=40.0)
    stored = P.read_study_stored(path)
    assert isinstance(stored[0], P.RleFrames) and stored[1] == "YBR_FULL" and stored[0].shape == (4, 40, 64) and stored[2]["frame_rate"] == 40.0
    assert np.array_equal(stored[0].blob, blob)
    arr, md, pid, hr = P.read_study(path)                                  # frames="host": the twin decodes, then converts
    assert np.array_equal(arr, F.ybr_full_to_rgb(frames)) and md["pixel_spacing"] == 0.05
    np.savez(path, rle_blob=blob, rle_off=off, rle_len=ln, rows=40, cols=64)
    with pytest.raises(DICOMReadError, match="samples"):
        P.read_study_stored(path)
    np.savez(path, rle_blob=blob[:100], rle_off=off, rle_len=ln, rows=40, cols=64, samples=3)
    with pytest.raises(DICOMReadError, match="inside rle_blob"):
        P.read_study(path)


def test_the_blob_travels_between_the_walks_processes_as_one_shared_array(tmp_path, monkeypatch):
    frames, (blob, off, ln) = RC.study("speckle", 3, 40, 64, 3)
    path = str(tmp_path / "s.npz")
    np.savez(path, rle_blob=blob, rle_off=off, rle_len=ln, rows=40, cols=64, samples=3)
    monkeypatch.setattr(P, "_SHM_MIN", 1024)
    before = dict(P._shm_stats)
    prepared = P._prepare_study_shm(P.read_study, path, "otsu", False, None, False, True, "device")
    assert isinstance(prepared[0], P.RleFrames) and P._is_shm(prepared[0].blob) and prepared[0].blob[2] == (blob.size,)
    study = P._Study("s.npz", str(tmp_path / "s.hdf5")).take(prepared, mapped=True)
    try:
        assert len(study.descs) == 1 and P._shm_stats["created"] == before["created"] + 1 and P._shm_stats["mapped"] == before["mapped"] + 1
        assert np.array_equal(study.nparr.blob, blob) and np.array_equal(study.nparr.decode(), frames)
    finally:
        study.release()
    # a study nobody mapped gives its block up by name
    prepared = P._prepare_study_shm(P.read_study, path, "otsu", False, None, False, True, "device")
    P._Study("s.npz", "x").take(prepared, mapped=False).release()
    from multiprocessing import shared_memory
    with pytest.raises(FileNotFoundError):
        shared_memory.SharedMemory(name=prepared[0].blob[1])


# ---- the library's side that needs no GPU ------------------------------------------------------------------------------------------------
def test_library_declares_the_rle_calls():
    from tee_optical_flow_amd.dense_flow import DenseFlow
    assert {"tf_rle_decode", "tf_hold_frames_rle", "tf_rle_stage_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.tf_rle_stage_bytes() == _lib.RLE_STAGE_BYTES == RC.T and RC.T % 16 == 0
    blob, off, ln = F.rle_record([F.rle_encode_frame(np.zeros((1, 1), np.uint8))])
    out, status = np.full(4, 7, np.uint8), np.full(1, -7, np.int32)
    assert L.tf_rle_decode(None, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, 1, 1, 1, out.ctypes.data, status.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_hold_frames_rle(None, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, 1, 1, 1, 1, 0, status.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert (out == 7).all() and status[0] == -7 and L.tf_abi_version() == 2
    for name in ("rle_decode", "hold_frames_rle"):
        assert callable(getattr(DenseFlow, name))


# ---- the core under the sanitizers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verify_rle(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rle") / "verify_rle"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_rle.cpp"), "-o", str(exe)])
    return str(exe)


def test_core_decodes_the_whole_corpus_under_the_sanitizers(verify_rle, tmp_path):
    path = tmp_path / "corpus.bin"
    RC.write_corpus(path)
    r = subprocess.run([verify_rle, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.strip() == f"{len(RC.corpus())} cases ok"


@pytest.mark.parametrize("shape", [(4, 1, 1), (3, 1, 2), (3, 1, 129), (2, 3, 5), (3, 37, 53), (2, 40, 64)], ids=lambda s: "x".join(map(str, s)))
def test_planar_ingest_stays_inside_exact_size_buffers(verify_rle, tmp_path, shape):
    N, H, W = shape
    src = np.random.default_rng(N * 1000 + H * 10 + W).integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(src.transpose(0, 3, 1, 2)).tofile(fin)            # [N][3][H * W]
    for form in ("RGB", "YBR_FULL"):
        for flip in (False, True):
            r = subprocess.run([verify_rle, "planar", str(fin), str(fout), str(_lib.FRAMES_FORMS[form]), str(int(flip)), str(N), str(H), str(W)],
                               capture_output=True, text=True)
            assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
            assert np.array_equal(np.fromfile(fout, np.uint8).reshape(N, H, W, 3), F.ingest_host(src, form, flip)), (form, flip)


# ---- the walks, with stand-in models -------------------------------------------------------------------------------------------------------
DRIVER = r"""
import sys, json, os, logging, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tee_optical_flow_amd import pipeline, masks as masks_mod
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.dense_flow import HeldFrames
from tee_optical_flow_amd.pipeline import process_folder, process_video
from tests.payload_cases import same_file
from tests.frames_cases import NumpyFrames
from tests import rle_cases as RC

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

class RleHolder(Holder):                  # ... and hold_frames_rle: the compressed bytes cross the bus, the twin stands for the device
    def hold_frames_rle(self, record, H, W, samples, form="RGB", flip=False):
        blob, off, ln = record
        self.log.append(("hold_frames_rle", form, bool(flip), int(np.asarray(blob).size)))
        arr = pipeline.RleFrames(blob, off, ln, (len(off), H, W), samples).decode()
        up = self.uploads
        tok = NumpyFrames.hold_frames(self, arr, form, flip)
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

if __name__ == "__main__":
    tmp = TMP
    kinds = [("sector", 3, None), ("sector", 3, "YBR_FULL"), ("speckle", 1, "MONOCHROME2"), ("ramps", 3, "RGB")]
    dirs = {"arr": os.path.join(tmp, "in_arr"), "rle": os.path.join(tmp, "in_rle")}
    for d in dirs.values(): os.makedirs(d)
    sizes = []
    for k, (fam, samples, ph) in enumerate(kinds):                      # 5 frames of 40 x 64, decoded and as stored
        frames, (blob, off, ln) = RC.study(fam, 5, 40, 64, samples, seed=k)
        extra = dict(pixel_spacing=0.05, frame_rate=40.0, patient_id=f"P{k}", heart_rate=70, **({} if ph is None else {"photometric": ph}))
        np.savez(os.path.join(dirs["arr"], f"s{k}.npz"), nparr=frames, **extra)
        np.savez(os.path.join(dirs["rle"], f"s{k}.npz"), rle_blob=blob, rle_off=off, rle_len=ln, rows=40, cols=64, samples=samples, **extra)
        sizes.append(int(blob.size))
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
        out["same"]["host" + f] = same_files(want, walk("rle_host" + f, "rle", Plain(), frames="host", flipLR=flip))
        out["same"]["device" + f] = same_files(want, walk("rle_dev" + f, "rle", RleHolder(), frames="device", flipLR=flip))
    want = os.path.join(tmp, "arr_host")
    out["same"]["no_rle_model"] = same_files(want, walk("fb_no_rle", "rle", Holder(), frames="device"))      # hold_frames, but no hold_frames_rle
    out["same"]["no_hold_model"] = same_files(want, walk("fb_plain", "rle", Plain(), frames="device"))
    for k in range(len(kinds)):
        a, b, c = (os.path.join(tmp, f"pv_{t}_{k}.hdf5") for t in "abc")
        m = RleHolder()
        fa = process_video(os.path.join(dirs["arr"], f"s{k}.npz"), a, mode="otsu", no_saliency=True, flow_model=Plain(), frames="host", flipLR=True)
        fb = process_video(os.path.join(dirs["rle"], f"s{k}.npz"), b, mode="otsu", no_saliency=True, flow_model=Plain(), frames="host", flipLR=True)
        fc = process_video(os.path.join(dirs["rle"], f"s{k}.npz"), c, mode="otsu", no_saliency=True, flow_model=m, frames="device", flipLR=True)
        out["video"][k] = [same_file(a, b), same_file(a, c), bool(np.array_equal(fa, fb) and np.array_equal(fa, fc)), m.log[0], m.uploads]
    print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    tmp = tmp_path_factory.mktemp("rle_walk")
    script = tmp / "walks.py"
    script.write_text(DRIVER.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp))))
    r = subprocess.run([PY_H5, str(script)], capture_output=True, text=True, timeout=600, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


FORMS = ["RGB", "YBR_FULL", "GRAY", "RGB"]                                   # s0 .. s3: no key, YBR_FULL, MONOCHROME2, RGB


def test_rle_studies_write_the_decoded_studies_files(walks):
    assert all(not w["errors"] for w in walks["walks"].values()), {k: w["errors"] for k, w in walks["walks"].items() if w["errors"]}
    assert len(walks["same"]) == 6 and all(walks["same"].values()), walks["same"]
    for k, (host, dev, flows, first, uploads) in walks["video"].items():
        assert host and dev and flows, (k, walks["video"][k])
        assert first == ["hold_frames_rle", FORMS[int(k)], True, walks["sizes"][int(k)]] and uploads == walks["sizes"][int(k)], (k, first, uploads)


def test_the_device_walk_holds_each_study_from_its_compressed_bytes(walks):
    for tag, flip in (("rle_dev", False), ("rle_dev_flip", True)):
        w = walks["walks"][tag]
        holds = [x for x in w["log"] if isinstance(x, list)]
        assert holds == [["hold_frames_rle", form, flip, size] for form, size in zip(FORMS, walks["sizes"])], (tag, holds)
        assert w["uploads"] == sum(walks["sizes"]) and not w["warnings"] and w["left"] == 0, (tag, w)
    for tag in ("rle_host", "arr_host"):
        assert not any(isinstance(x, list) for x in walks["walks"][tag]["log"]) and not walks["walks"][tag]["warnings"]


def test_rle_fallbacks_say_why_once_per_walk(walks):
    w = walks["walks"]["fb_no_rle"]                                         # the twin decodes, the decoded array is held as ever
    assert len(w["warnings"]) == 1 and "the host decodes it instead" in w["warnings"][0] and "has no hold_frames_rle" in w["warnings"][0]
    assert [x[:2] for x in w["log"] if isinstance(x, list)] == [["hold_frames", form] for form in FORMS]
    assert w["uploads"] == 5 * 40 * 64 * (3 + 3 + 1 + 3)
    w = walks["walks"]["fb_plain"]
    assert len(w["warnings"]) == 2 and any("has no hold_frames_rle" in x for x in w["warnings"]) and any("has no hold_frames" in x and "frames='device' not used" in x for x in w["warnings"])
