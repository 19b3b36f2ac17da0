"""Inflate without a GPU: the decoder's core (csrc/teeflow_inflate_core.h, the text the device kernel runs) on one lane, in a
stand-alone program built with the address and undefined-behaviour sanitizers, over the whole corpus of tests/inflate_cases.py --
zlib's bytes where zlib decodes a stream, a status where zlib raises, no sanitizer report anywhere; and the chunk records of a study
file: analysis.unchunk_host against direct slicing, HeldStudy.from_chunks' bookkeeping on a numpy engine, and, in the interpreter that
has h5py, study_chunks of a file the writer made."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A

from tests import inflate_cases as IC
from tests.numpy_engine import NumpyEngine

ROOT, PY_H5 = IC.ROOT, IC.PY_H5


# ---- 1. the core under the sanitizers -----------------------------------------------------------------------------------------------
def test_corpus_has_every_case_the_decoder_must_meet():
    """a check of the corpus itself, not of the decoder: it holds the sizes, families, settings and faults the other tests rely on
    (it needs nothing of the library, so it also passes where the decoder does not exist)"""
    cs, vs = IC.cases(), IC.verdicts()
    kinds = [k for k, _ in vs]
    assert kinds.count(IC.GOOD) > 300 and kinds.count(IC.BAD) > 40 and kinds.count(IC.SHORT) > 100
    names = {c.name for c in cs}
    for fam in IC.FAMILIES:
        for n in IC.SIZES:
            assert f"{fam}-{n}-L9" in names
    by = dict(zip((c.name for c in cs), kinds))
    assert by["bytes-after-trailer"] == IC.GOOD and by["flushes"] == IC.GOOD and by["f16noise-73728-L0-huffman-m1-w9"] == IC.GOOD
    for bad in ("block-type-3", "stored-len-nlen", "match-before-start", "match-one-before-start", "fdict", "cm-not-8"):
        assert by[bad] == IC.BAD, bad
    assert by["one-byte-longer"] == IC.SHORT and by["one-byte-shorter"] == IC.SHORT and by["prefix-dynamic-0"] == IC.SHORT
    # the good streams hold every block type: stored (00), fixed (01) and dynamic (10) first blocks
    first = {(c.stream[2] >> 1) & 3 for c, k in zip(cs, kinds) if k == IC.GOOD}
    assert first == {0, 1, 2}
    # and codes of every length the format has: the deepest literal/length code and the deepest distance code of the good streams
    # have 15 bits, the limit, far behind the decoder's one-step tables (without the four streams below they have 13 and 12)
    from tests import deflate_cases as DC
    deep = [0, 0]
    for name in ("fibdist-L9", "fibdist-bl-L9", "lloverflow-16-L9", "lloverflow-17-L9"):
        assert by[name] == IC.GOOD, name
        d = DC.blocks(next(c.stream for c in cs if c.name == name))[1]
        deep = [max(deep[0], d[0]), max(deep[1], d[2])]
    assert deep == [15, 15]


def test_core_decodes_the_corpus_under_the_sanitizers(tmp_path):
    exe = tmp_path / "verify_inflate"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_inflate.cpp"), "-o", str(exe)])
    cs, vs = IC.cases(), IC.verdicts()
    with open(tmp_path / "corpus.bin", "wb") as f:
        f.write(struct.pack("<I", len(cs)))
        for c in cs:
            f.write(struct.pack("<II", len(c.stream), c.out_bytes))
            f.write(c.stream)
    r = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), str(tmp_path / "result.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    buf = open(tmp_path / "result.bin", "rb").read()
    at, wrong = 0, []
    for c, (kind, want) in zip(cs, vs):
        status, produced = struct.unpack_from("<iI", buf, at)
        got = buf[at + 8:at + 8 + c.out_bytes]
        at += 8 + c.out_bytes
        assert 0 <= status <= 8 and produced <= c.out_bytes, c.name
        assert got[produced:] == b"\xEE" * (c.out_bytes - produced), f"{c.name}: wrote behind what it produced"
        for msg in (IC.check(c, kind, want, status, got), IC.check_prefix(c, kind, want, got, produced)):
            if msg:
                wrong.append(msg)
    assert at == len(buf)
    assert not wrong, (len(wrong), wrong[:10])


# ---- 2. chunk records ------------------------------------------------------------------------------------------------------------------
_record = IC.chunked


CHUNKINGS = [((5, 37, 53, 2), (2, 16, 16, 1), np.float16), ((5, 37, 53), (3, 10, 27), np.float16), ((4, 6, 8, 2), (4, 6, 8, 2), np.bool_),
             ((5, 37, 53, 1), (5, 19, 53, 1), np.uint8), ((3, 7), (2, 4), np.uint32)]


@pytest.mark.parametrize("shape,chunks,dtype", CHUNKINGS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_unchunk_host_equals_direct_slicing(shape, chunks, dtype):
    rng = np.random.default_rng(sum(shape))
    arr = (rng.random(shape) < 0.4) if dtype == np.bool_ else (rng.normal(0, 40, shape)).astype(dtype)
    rec, want = _record(arr, chunks)
    got = A.unchunk_host(rec)
    assert got.dtype == arr.dtype and got.shape == arr.shape and np.array_equal(got.view(np.uint8), arr.view(np.uint8))
    n = len(rec["len"])
    rec2, want2 = _record(arr, chunks, unfiltered={0}, missing={n - 1} if n > 1 else ())
    assert np.array_equal(A.unchunk_host(rec2, workers=1).view(np.uint8), want2.view(np.uint8))
    if n > 1:
        assert not want2[tuple(slice(s - 1, s) for s in shape)].any() and len(rec2["len"]) == n - 1
    bad = dict(rec, blob=rec["blob"].copy())
    bad["blob"][int(rec["off"][0]) + int(rec["len"][0]) // 2] ^= 0x55
    with pytest.raises((zlib.error, ValueError)):
        A.unchunk_host(bad)


class ChunkEngine(NumpyEngine):
    """NumpyEngine with the three chunk methods, on unchunk_host"""

    def inflate(self, streams, out_bytes):
        out, status = np.zeros((len(streams), out_bytes), np.uint8), np.zeros(len(streams), np.int32)
        for i, s in enumerate(streams):
            d = zlib.decompressobj()
            try:
                got = d.decompress(bytes(s))
            except zlib.error:
                status[i] = 1
                continue
            out[i, :min(len(got), out_bytes)] = np.frombuffer(got[:out_bytes], np.uint8)
            status[i] = 0 if d.eof and len(got) == out_bytes else 7
        return out, status

    def hold_study_chunks(self, flow_chunks, echo_chunks=None):
        self.calls.append("hold_study_chunks")
        flow, echo = A.unchunk_host(flow_chunks), None if echo_chunks is None else A.unchunk_host(echo_chunks)   # raises before anything changes
        NumpyEngine.hold_study(self, flow, echo)
        self.calls.pop()
        return self.held

    def hold_mask_chunks(self, label, chunks):
        self.calls.append("hold_mask_chunks")
        NumpyEngine.hold_mask(self, label, A.unchunk_host(chunks))
        self.calls.pop()


def _study_record(N=5, H=37, W=53, labels=("rv", "av"), echo=True):
    rng = np.random.default_rng(N * H + W)
    arrays = {"flow": rng.normal(0, 2, (N, H, W, 2)).astype(np.float16)}
    if echo:
        arrays["echo"] = rng.integers(0, 256, (N, H, W)).astype(np.float16)
    for k, lab in enumerate(labels):
        arrays[lab] = rng.random((N, H, W, 1 + k % 2)) < 0.5
    ch = {"flow": (2, 16, 16, 1), "echo": (3, 10, 27)}
    rec = {"filename": "study", "attrs": {"frame_rate": 50.0, "units_converted": True, "nframes": N, "mode": "RVIO_2class", "labels": list(labels)},
           "datasets": {k: _record(a, ch.get(k, (2, 16, 16, 1)))[0] for k, a in arrays.items()}}
    return rec, arrays


@pytest.mark.parametrize("way", ["host", "device"])
def test_from_chunks_bookkeeping_on_the_numpy_engine(way):
    rec, arrays = _study_record()
    e = ChunkEngine()
    hs = A.HeldStudy.from_chunks(e, rec, inflate=way)
    want = ["hold_study", "hold_mask", "hold_mask"] if way == "host" else ["hold_study_chunks", "hold_mask_chunks", "hold_mask_chunks"]
    assert e.calls == want
    assert hs.nframes == 3 and hs.frame_rate == 50.0 and hs.mode == "RVIO_2class" and hs.filename == "study"
    assert hs.accepted_labels == ["rv", "av"] and hs.shape == (5, 37, 53) and hs.n_echo == 5
    assert e.held.masks == {"rv": (5, 1), "av": (5, 2)}
    assert np.array_equal(e.flow.view(np.uint16), arrays["flow"].view(np.uint16)) and np.array_equal(e.echo, arrays["echo"])
    for k in ("rv", "av"):
        assert np.array_equal(e.masks[k], arrays[k])
    # the analysis functions read it as they read any held study
    ref = A.FlowStudy(arrays["flow"], {k: arrays[k] for k in ("rv", "av")}, 50.0, nframes=3, echo=arrays["echo"])
    assert np.array_equal(A.area_series(hs, "rv", engine=e), A.area_series(ref, "rv", engine=NumpyEngine()))
    # units_converted False: the frame rate is 1, as FlowStudy.from_hdf5 has it; no echo: none held
    rec2, _ = _study_record(echo=False, labels=("rv",))
    rec2["attrs"]["units_converted"] = False
    hs2 = A.HeldStudy.from_chunks(e, rec2, inflate=way)
    assert hs2.frame_rate == 1 and hs2.n_echo == 0 and hs2.generation != hs.generation and hs2.accepted_labels == ["rv"]
    with pytest.raises(RuntimeError, match="stale"):
        A.area_series(hs, "rv", engine=e)
    with pytest.raises(ValueError, match="inflate must be"):
        A.HeldStudy.from_chunks(e, rec, inflate="h5py")
    with pytest.raises(ValueError, match="inflate must be"):
        A.HeldStudy.from_hdf5(e, "nowhere.hdf5", inflate="gpu")


def test_a_chunk_that_does_not_inflate_leaves_the_held_study(caplog):
    rec, arrays = _study_record()
    e = ChunkEngine()
    hs = A.HeldStudy.from_chunks(e, rec)
    bad, _ = _study_record(N=6)
    blob = bad["datasets"]["flow"]["blob"].copy()
    blob[int(bad["datasets"]["flow"]["off"][3]) + 9] ^= 0xFF
    bad["datasets"]["flow"]["blob"] = blob
    with pytest.raises((zlib.error, ValueError)):
        A.HeldStudy.from_chunks(e, bad)
    assert e.held.generation == hs.generation and e.held.N == 5 and sorted(e.held.masks) == ["av", "rv"]
    assert np.array_equal(e.flow.view(np.uint16), arrays["flow"].view(np.uint16))


def test_save_chunks_round_trip_is_plain_data(tmp_path):
    rec, arrays = _study_record()
    A.save_chunks(rec, str(tmp_path / "c.npz"))
    back = A.load_chunks(str(tmp_path / "c.npz"))
    assert back["filename"] == rec["filename"] and back["attrs"] == rec["attrs"] and list(back["datasets"]) == list(rec["datasets"])
    for name, ds in rec["datasets"].items():
        b = back["datasets"][name]
        assert b["shape"] == ds["shape"] and b["chunks"] == ds["chunks"] and b["dtype"] == ds["dtype"]
        for k in ("coord", "filter_mask", "off", "len", "blob"):
            assert b[k].dtype == ds[k].dtype and np.array_equal(b[k], ds[k]), (name, k)
        assert np.array_equal(A.unchunk_host(b).view(np.uint8), arrays[name].view(np.uint8))


def test_python_refusals_come_before_the_library():
    from tee_optical_flow_amd import DenseFlow
    from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError
    rec, _ = _study_record()
    flow = rec["datasets"]["flow"]
    for broken, text in ((dict(flow, dtype="float32"), "float16"), (dict(flow, shape=(5, 37, 53)), "4-D"),
                         (dict(flow, len=flow["len"][:-1]), "disagree"), (dict(flow, blob=flow["blob"][:-1]), "behind the blob")):
        with pytest.raises(OpticalFlowCalculationError, match=text):
            DenseFlow._chunked(broken, "flow", 4, (np.float16,))
    c, keep = DenseFlow._chunked(flow, "flow", 4, (np.float16,))
    assert (c.n, c.ndim, c.elem_bytes, c.chunk_bytes, list(c.shape), list(c.chunk)) == (len(flow["len"]), 4, 2, 1024, [5, 37, 53, 2], [2, 16, 16, 1])


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    """(the refusals that need a handle to carry their message are in tests/test_gpu_inflate.py and tests/test_gpu_held_chunks.py)"""
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd import DenseFlow
    L = _lib.load()
    rec, _ = _study_record()
    one = np.zeros(1, np.uint8)
    off, ln, st = np.zeros(2, np.uint64), np.full(2, 4, np.uint32), np.full(2, -5, np.int32)
    out = np.full((2, 8), 7, np.uint8)
    assert L.tf_inflate(None, one.ctypes.data, off.ctypes.data, ln.ctypes.data, None, 2, 8, out.ctypes.data, st.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert (out == 7).all() and (st == -5).all()
    flow, keep = DenseFlow._chunked(rec["datasets"]["flow"], "flow", 4, (np.float16,))
    mask, keep2 = DenseFlow._chunked(rec["datasets"]["rv"], "mask", 4, (np.bool_,))
    assert L.tf_hold_study_chunks(None, C.byref(flow), None) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_hold_mask_chunks(None, 0, C.byref(mask)) == _lib.TF_ERR_INVALID_ARG
    del keep, keep2


# ---- 3. a file the writer made, in the interpreter that has h5py -----------------------------------------------------------------
H5_DRIVER = r"""
import sys, json, os, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.hdf5_out import save_optical_flow_to_hdf5
from tee_optical_flow_amd.config import default_optical_flow_config

rng = np.random.default_rng(11)
N, H, W = 7, 150, 170
flow = np.cumsum(rng.normal(0, 0.1, (N, H, W, 2)), axis=2).astype(np.float32)
nparr = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
masks = {"rv": rng.random((N, H, W, 2)) < 0.5, "bkgd": np.ones((N, H, W, 2), bool)}
meta = {"frame_rate": 40.0, "pixel_spacing": 0.05, "R_wave_data_present": False, "R_times": None}
path = os.path.join(TMP, "study.hdf5")
save_optical_flow_to_hdf5(path, flow, nparr, masks, meta, {}, "P", 60, default_optical_flow_config(), "RVIO_2class", False, False)
rec = A.study_chunks(path)
A.save_chunks(rec, os.path.join(TMP, "study_chunks.npz"))
back = A.load_chunks(os.path.join(TMP, "study_chunks.npz"))
out = {"names": list(back["datasets"]), "labels": back["attrs"]["labels"], "filename": back["filename"], "equal": {}, "chunks": {}, "gpu_libs": []}
with h5py.File(path, "r") as f:
    for k, ds in back["datasets"].items():
        got = A.unchunk_host(ds)
        out["equal"][k] = bool(got.dtype == f[k].dtype and np.array_equal(got.view(np.uint8), f[k][()].view(np.uint8)))
        out["chunks"][k] = [len(ds["len"]), list(ds["chunks"]), list(f[k].chunks)]
    a = f["flow"].attrs
    out["attrs"] = [bool(back["attrs"]["frame_rate"] == a["frame_rate"]), bool(back["attrs"]["nframes"] == a["nframes"]), back["attrs"]["mode"] == a["mode"],
                    bool(back["attrs"]["units_converted"] == a["units_converted"])]
    # a dataset that is not plain gzip chunks is refused with a reason
    with h5py.File(os.path.join(TMP, "other.hdf5"), "w") as g:
        for k in ("flow", "echo", "rv", "bkgd"):
            g.create_dataset(k, data=f[k][()], **({"compression": "gzip", "shuffle": True} if k == "rv" else {} if k == "echo" else {"compression": "gzip"}))
        for k, v in a.items():
            g["flow"].attrs[k] = v
for drop, key in (("echo", "contiguous"), (None, "shuffle")):
    p = os.path.join(TMP, "other.hdf5")
    if drop is None:
        with h5py.File(p, "a") as g:
            del g["echo"]
    try:
        A.study_chunks(p)
        out[key] = "accepted"
    except A.ChunksUnavailable as e:
        out[key] = str(e)
# from_hdf5's three ways on an engine that keeps the arrays: the same held bytes; and the fall-back to h5py, with its one logged reason
import logging
from tests.numpy_engine import NumpyEngine
class Eng(NumpyEngine):
    def hold_study_chunks(self, flow_chunks, echo_chunks=None):
        self.calls.append("hold_study_chunks")
        return NumpyEngine.hold_study(self, A.unchunk_host(flow_chunks), None if echo_chunks is None else A.unchunk_host(echo_chunks))
    def hold_mask_chunks(self, label, chunks):
        self.calls.append("hold_mask_chunks")
        NumpyEngine.hold_mask(self, label, A.unchunk_host(chunks))
class Keep(logging.Handler):
    def __init__(self): logging.Handler.__init__(self); self.msgs = []
    def emit(self, r): self.msgs.append(r.getMessage())
keep = Keep()
logging.getLogger("tee_optical_flow_amd.analysis").addHandler(keep)
held = {}
for way in A.INFLATE_WAYS:
    e = Eng()
    hs = A.HeldStudy.from_hdf5(e, path, inflate=way)
    held[way] = (e, hs)
ref = held["h5py"][0]
out["ways"] = {w: [bool(np.array_equal(e.flow.view(np.uint16), ref.flow.view(np.uint16)) and np.array_equal(e.echo, ref.echo)
                        and all(np.array_equal(e.masks[k], ref.masks[k]) for k in ("rv", "bkgd"))),
                   hs.nframes, hs.frame_rate, hs.filename, "hold_study_chunks" in e.calls] for w, (e, hs) in held.items()}
out["logged_before"] = list(keep.msgs)
e = Eng()
A.HeldStudy.from_hdf5(e, os.path.join(TMP, "other.hdf5"), inflate="device")
out["fallback"] = [bool(np.array_equal(e.flow.view(np.uint16), ref.flow.view(np.uint16))), "hold_study_chunks" in e.calls, list(keep.msgs)]
with open("/proc/self/maps") as m:
    out["gpu_libs"] = sorted({ln.split("/")[-1].strip() for ln in m if "libamdhip" in ln or "libteeflow" in ln or "libhsa" in ln})
print(json.dumps(out))
"""


def test_study_chunks_of_a_written_file(tmp_path):
    import json
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    script = H5_DRIVER.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp_path)))
    r = subprocess.run([PY_H5, "-c", script], capture_output=True, text=True, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    g = json.loads(r.stdout.strip().splitlines()[-1])
    assert g["names"] == ["flow", "echo", "rv", "bkgd"] and g["labels"] == ["rv", "bkgd"] and g["filename"] == "study."
    assert g["equal"] == {"flow": True, "echo": True, "rv": True, "bkgd": True}
    assert all(g["attrs"])
    for k, (n, rec_chunks, file_chunks) in g["chunks"].items():
        assert rec_chunks == file_chunks and n > 1, k
    assert "contiguous" in g["contiguous"] and "filter pipeline" in g["shuffle"]
    assert g["ways"] == {"h5py": [True, 5, 40.0, "study.", False], "host": [True, 5, 40.0, "study.", False], "device": [True, 5, 40.0, "study.", True]}
    assert g["logged_before"] == []
    same, chunked, logged = g["fallback"]
    assert same and not chunked and len(logged) == 1 and "read through h5py instead of inflate='device'" in logged[0] and "filter pipeline" in logged[0]
    assert g["gpu_libs"] == []                                # the child has mapped no GPU library
