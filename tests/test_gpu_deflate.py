"""Deflate on the device (tf_deflate, tf_deflate_array, tf_held_deflate; DenseFlow.deflate, deflate_array, held_deflate) against zlib
level 9, byte for byte: the whole corpus of tests/deflate_cases.py against the recorded digests of zlib's streams (which
tests/test_deflate_cpu.py holds the running zlib to), the chunking of arrays against tests/inflate_cases.chunked, the round trip
through the device's own inflate, the held study's arrays read where they are, and every refusal.  A call has one chunk size, so the
corpus goes up grouped by size.  Calls of more chunks than one batch of the scratch holds ("deflate_batches" counts the batches), and
the corpus' sweeps of 1,500 seeded chunks against their recorded digests."""
import time
import zlib

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests import deflate_cases as DC
from tests import inflate_cases as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0, max_batch=3)
    yield e
    e.close()


def _streams(blob, off, ln):
    return [blob[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)]


def _same_record(got, want, what):
    assert tuple(got["shape"]) == tuple(want["shape"]) and tuple(got["chunks"]) == tuple(want["chunks"]) and got["dtype"] == want["dtype"], what
    for k in ("coord", "off", "len", "blob", "filter_mask"):
        assert np.array_equal(np.asarray(got[k]).reshape(np.asarray(want[k]).shape), want[k]), (what, k)


def test_the_whole_corpus_against_zlibs_digests(eng):
    groups = {}
    for c in DC.cases():
        groups.setdefault(len(c.raw), []).append(c)
    want, wrong, seen = DC.digests(), [], 0
    c0 = [eng.counter(k) for k in ("deflate_match_us", "deflate_emit_us")]
    for size, cs in sorted(groups.items()):
        blob, off, ln = eng.deflate([c.raw for c in cs])
        assert off.dtype == np.uint64 and ln.dtype == np.uint32 and blob.dtype == np.uint8
        assert list(off) == list(np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)])) and blob.size == int(ln.sum())
        for c, s in zip(cs, _streams(blob, off, ln)):
            seen += 1
            if DC.digest(s) != want[c.name]:
                wrong.append((c.name, len(s), want[c.name][0]))
    assert seen == len(want) and not wrong, (len(wrong), wrong[:10])
    assert eng.counter("deflate_match_us") > c0[0] and eng.counter("deflate_emit_us") > c0[1]


# (the last four: chunks of more than 2,048 elements, where k_chunk's grid has a second row and a thread's stride is rows x 256:
# 16,384 elements, ragged in three dimensions; 6,000 and 4,224; 180,000, where the grid stays at its 64 rows)
CHUNKINGS = [((5, 37, 53, 2), (2, 16, 16, 1), np.float16), ((5, 37, 53), (3, 10, 27), np.float16), ((4, 6, 8, 2), (4, 6, 8, 2), np.bool_),
             ((3, 7), (2, 4), np.uint32), ((1000,), (333,), np.uint8),
             ((3, 70, 90, 2), (2, 64, 64, 2), np.float16), ((5, 50, 60), (2, 50, 60), np.bool_), ((3, 40, 70), (2, 33, 64), np.uint32),
             ((4, 300, 300), (2, 300, 300), np.uint8)]


def _array(shape, dtype):
    rng = np.random.default_rng(sum(shape))
    return (rng.random(shape) < 0.4) if dtype == np.bool_ else rng.normal(0, 40, shape).astype(dtype)


@pytest.mark.parametrize("shape,chunks,dtype", CHUNKINGS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_deflate_array_equals_the_chunks_zlib_makes(eng, shape, chunks, dtype):
    arr = _array(shape, dtype)
    want, _ = IC.chunked(arr, chunks, level=9)
    c0 = eng.counter("chunk_kernel_us")
    _same_record(eng.deflate_array(arr, chunks), want, "deflate_array")
    assert eng.counter("chunk_kernel_us") > c0


def _running_sum(off, ln):
    return off.dtype == np.uint64 and list(off) == list(np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]))


def test_many_packed_chunks_go_through_several_batches(eng):
    """3,000 chunks of 16 bytes: more than one batch of deflate_run's scratch holds (1,363 today, so three batches), which the
    counter shows rather than the constants: the later batches read their coordinates, lengths and offsets from c0 on, carry the
    blob's total on, and write the scratch again"""
    t0 = time.perf_counter()
    chunks = DC.sweep(16, 3000)
    b0 = eng.counter("deflate_batches")
    blob, off, ln = eng.deflate(chunks)
    batches = eng.counter("deflate_batches") - b0
    print(f"3000 packed chunks of 16 B: {batches} batches")
    assert batches >= 2
    assert ln.shape == off.shape == (3000,) and _running_sum(off, ln) and blob.size == int(ln.sum())
    wrong = [i for i, (c, s) in enumerate(zip(chunks, _streams(blob, off, ln))) if s != zlib.compress(c, 9)]
    assert not wrong, (len(wrong), wrong[:10])
    print(f"3000 packed chunks of 16 B: {time.perf_counter() - t0:.2f} s")


def test_many_array_chunks_go_through_several_batches(eng):
    """1,960 chunks of 32 bytes of an array in host memory and of the held study: k_chunk from the batch's first coordinate on"""
    t0 = time.perf_counter()
    arr, chunks = _array((7, 37, 53, 2), np.float16), (1, 4, 4, 1)
    want, _ = IC.chunked(arr, chunks, level=9)
    assert len(want["len"]) == 1960
    b0 = eng.counter("deflate_batches")
    _same_record(eng.deflate_array(arr, chunks), want, "deflate_array")
    b1 = eng.counter("deflate_batches")
    eng.hold_study(arr)
    up = eng.counter("tail_upload_bytes")
    held = eng.held_deflate("flow", chunks)
    b2 = eng.counter("deflate_batches")
    print(f"1960 array chunks of 32 B: {b1 - b0} batches from host memory, {b2 - b1} from the held study")
    assert eng.counter("tail_upload_bytes") == up
    _same_record(held, want, "held_deflate")
    assert b1 - b0 >= 2 and b2 - b1 >= 2
    eng.release_study()
    print(f"1960 array chunks of 32 B: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("size", DC.SWEEP_SIZES)
def test_sweep_against_zlibs_digest(eng, size):
    """1,500 seeded chunks of one size in one call, against the one recorded digest of zlib's streams of them"""
    t0 = time.perf_counter()
    chunks = DC.sweep(size)
    b0 = eng.counter("deflate_batches")
    blob, off, ln = eng.deflate(chunks)
    batches = eng.counter("deflate_batches") - b0
    print(f"sweep of {len(chunks)} chunks of {size} B: {batches} batches")
    assert _running_sum(off, ln) and blob.size == int(ln.sum())
    streams = _streams(blob, off, ln)
    if DC.sweep_digest(streams) != DC.sweep_digests()[size]:
        pytest.fail(f"sweep {size}: (first differing chunk, its family, bytes made, zlib's bytes) = {DC.first_difference(chunks, streams)}")
    assert batches >= (2 if size == 512 else 1)               # (512: about 1,323 chunks to a batch today)
    print(f"sweep of {len(chunks)} chunks of {size} B: {time.perf_counter() - t0:.2f} s")


def test_round_trip_through_the_devices_inflate(eng):
    cs = [c for c in DC.cases() if len(c.raw) == 73728]
    assert len(cs) >= 8
    blob, off, ln = eng.deflate(np.frombuffer(b"".join(c.raw for c in cs), np.uint8).reshape(len(cs), 73728))
    out, status = eng.inflate(_streams(blob, off, ln), 73728)
    assert not status.any() and all(out[i].tobytes() == c.raw for i, c in enumerate(cs))
    # the device's own streams with codes of 15 bits, distance and literal/length: behind the decoder's one-step tables
    by = {c.name: c.raw for c in DC.cases()}
    for name in ("fibdist", "lloverflow-16", "lloverflow-17"):
        blob, off, ln = eng.deflate([by[name]])
        out, status = eng.inflate(_streams(blob, off, ln), len(by[name]))
        assert list(status) == [0] and out[0].tobytes() == by[name], name
    # and a record goes back into a held study as the file's own chunks do
    flow = _array((5, 37, 53, 2), np.float16)
    eng.hold_study_chunks(eng.deflate_array(flow, (2, 16, 16, 1)))
    again = eng.held_deflate("flow", (5, 37, 53, 2))
    assert zlib.decompress(again["blob"].tobytes()) == flow.tobytes()
    eng.release_study()


def _held_equals_array(eng, arrays, chunkings):
    for what, arr in arrays.items():
        up = eng.counter("tail_upload_bytes")
        got = eng.held_deflate(what, chunkings[what])
        assert eng.counter("tail_upload_bytes") == up, what
        _same_record(got, eng.deflate_array(arr, chunkings[what]), what)
        _same_record(got, IC.chunked(arr, chunkings[what], level=9)[0], what)


def test_held_deflate_reads_the_held_study_where_it_is(eng):
    from tee_optical_flow_amd.synth import speckle_sequence
    rng = np.random.default_rng(5)
    N, H, W = 5, 37, 53
    flow, echo = _array((N, H, W, 2), np.float16), rng.integers(0, 256, (N, H, W)).astype(np.float16)
    mask = rng.random((N, H, W, 2)) < 0.5
    chunkings = {"flow": (2, 16, 16, 1), "echo": (3, 10, 27), "rv": (2, 19, 53, 1)}
    eng.hold_study(flow, echo)
    eng.hold_mask("rv", mask)
    _held_equals_array(eng, {"flow": flow, "echo": echo, "rv": mask}, chunkings)
    # after a study call that leaves its payload held
    rgb = np.ascontiguousarray(np.repeat(speckle_sequence(6, N + 1, H, W)[..., None], 3, axis=3))
    flow2, echo2 = eng.calc_study_payload(rgb, hold=True)
    eng.hold_mask("rv", mask[:flow2.shape[0]])
    _held_equals_array(eng, {"flow": flow2, "echo": echo2, "rv": mask[:flow2.shape[0]]}, chunkings)
    eng.release_study()
    with pytest.raises(OpticalFlowCalculationError, match="no study is held"):
        eng.held_deflate("flow", (2, 16, 16, 1))


def test_refusals_come_before_any_gpu_work(eng):
    L, h = eng._L, eng._h
    raw = np.zeros((2, 64), np.uint8)
    cap = 2 * eng.deflate_bound(64)
    blob, off, ln, st = np.full(cap, 7, np.uint8), np.full(2, 9, np.uint64), np.full(2, 9, np.uint32), np.full(2, -5, np.int32)
    coord = np.full((2, 4), -3, np.int64)
    names = ("tail_upload_bytes", "deflate_match_us", "deflate_emit_us", "chunk_kernel_us")
    c0 = [eng.counter(k) for k in names]
    good = dict(chunks=raw.ctypes.data, n=2, cb=64, blob=blob.ctypes.data, cap=cap, off=off.ctypes.data, len=ln.ctypes.data, st=st.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_deflate(h, a["chunks"], a["n"], a["cb"], a["blob"], a["cap"], a["off"], a["len"], a["st"])
    for bad, text in ((dict(chunks=None), "null chunks"), (dict(n=-1), "n = -1"), (dict(cb=(16 << 20) + 1), "at most"), (dict(blob=None), "null blob"),
                      (dict(off=None), "null blob"), (dict(len=None), "null blob"), (dict(st=None), "null blob"), (dict(cap=cap - 1), "blob_cap")):
        assert call(**bad) == _lib.TF_ERR_INVALID_ARG, bad
        assert text in L.tf_last_error(h).decode(), (bad, L.tf_last_error(h))
    assert call(n=0) == _lib.TF_OK
    arr = np.zeros((4, 6, 8, 2), np.uint8)
    sh, ch = np.array(arr.shape, np.int64), np.array((4, 6, 8, 1), np.int64)
    agood = dict(arr=arr.ctypes.data, ndim=4, sh=sh.ctypes.data, ch=ch.ctypes.data, eb=1, n=2, blob=blob.ctypes.data, cap=1 << 20, off=off.ctypes.data,
                 len=ln.ctypes.data, coord=coord.ctypes.data, st=st.ctypes.data)

    def acall(**kw):
        a = {**agood, **kw}
        return L.tf_deflate_array(h, a["arr"], a["ndim"], a["sh"], a["ch"], a["eb"], a["n"], a["blob"], a["cap"], a["off"], a["len"], a["coord"], a["st"])
    zero = np.array((4, 0, 8, 1), np.int64)
    for bad, text in ((dict(arr=None), "null array"), (dict(ndim=0), "dimensions"), (dict(ndim=5), "dimensions"), (dict(eb=3), "byte elements"),
                      (dict(sh=None), "null shape"), (dict(ch=None), "null shape"), (dict(ch=zero.ctypes.data), "dimension 1"), (dict(n=3), "has 2 chunks"),
                      (dict(coord=None), "null blob"), (dict(cap=10), "blob_cap")):
        assert acall(**bad) == _lib.TF_ERR_INVALID_ARG, bad
        assert text in L.tf_last_error(h).decode(), (bad, L.tf_last_error(h))

    def hcall(what=0, slot=0, n=2):
        return L.tf_held_deflate(h, what, slot, ch.ctypes.data, n, blob.ctypes.data, 1 << 20, off.ctypes.data, ln.ctypes.data, coord.ctypes.data, st.ctypes.data)
    assert hcall() == _lib.TF_ERR_INVALID_ARG and "no study is held" in L.tf_last_error(h).decode()
    eng.hold_study(np.zeros((4, 6, 8, 2), np.float16))
    c0[0] = eng.counter("tail_upload_bytes")
    for kw, text in ((dict(what=3), "none of flow"), (dict(what=1), "no echo"), (dict(what=2, slot=0), "is empty"), (dict(what=2, slot=12), "out of range"),
                     (dict(n=5), "has 2 chunks")):
        assert hcall(**kw) == _lib.TF_ERR_INVALID_ARG, kw
        assert text in L.tf_last_error(h).decode(), (kw, L.tf_last_error(h))
    assert (blob == 7).all() and (off == 9).all() and (ln == 9).all() and (st == -5).all() and (coord == -3).all()
    assert [eng.counter(k) for k in names] == c0
    eng.release_study()
    for bad, text in (((np.zeros((2, 3), np.float32),), "uint8"), (([b"ab", b"abc"],), "one size")):
        with pytest.raises(OpticalFlowCalculationError, match=text):
            eng.deflate(*bad)
    with pytest.raises(OpticalFlowCalculationError, match="1-, 2- or 4-byte"):
        eng.deflate_array(np.zeros((2, 2)), (1, 1))
    with pytest.raises(OpticalFlowCalculationError, match="chunk extents"):
        eng.deflate_array(np.zeros((2, 2), np.uint8), (1,))
    # the call that follows the refusals works, and counts what it uploads
    blob2, off2, ln2 = eng.deflate([b"hello hello hello", b"HELLO HELLO HELLO"])
    assert _streams(blob2, off2, ln2) == [zlib.compress(b"hello hello hello", 9), zlib.compress(b"HELLO HELLO HELLO", 9)]
    assert eng.counter("tail_upload_bytes") - c0[0] == 34


VIDEO_SCRIPT = r"""
import sys, json, os, logging, zlib, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tests.payload_cases import same_file
import tee_optical_flow_amd as T
from tee_optical_flow_amd import hdf5_out
from tee_optical_flow_amd.pipeline import process_video
from tee_optical_flow_amd.synth import speckle_sequence

class Keep(logging.Handler):
    def __init__(self): logging.Handler.__init__(self); self.msgs = []
    def emit(self, r): self.msgs.append(r.getMessage())
keep = Keep()
logging.getLogger("tee_optical_flow_amd.pipeline").addHandler(keep)
count = [0]
real = zlib.compress
def counting(*a, **k):
    count[0] += 1
    return real(*a, **k)
hdf5_out.zlib.compress = counting
# (21 frames: echo, flow and mask each pass 1 MiB, from where create_gzip9 hands whole chunks to HDF5 and asks the deflater)
rgb = np.ascontiguousarray(np.repeat(speckle_sequence(31, 21, 150, 170)[..., None], 3, axis=3))
md = {"pixel_spacing": 0.04, "frame_rate": 50.0, "R_wave_data_present": False, "R_times": None}
eng = T.DenseFlow(device_id=0)
out = {"host_compress": {}, "counters": {}}
kw = dict(nparr=rgb, metadata=md, patient_id="SYN", heart_rate=60, mode="otsu", no_saliency=True, verbose=False, flow_model=eng, payload="device")
for way in ("host", "device"):
    c0 = [eng.counter(k) for k in ("deflate_match_us", "chunk_kernel_us")]
    count[0] = 0
    flow = process_video(None, os.path.join(TMP, way + ".hdf5"), deflate=way, **kw)
    out["host_compress"][way] = count[0]
    out["counters"][way] = [eng.counter(k) - c for k, c in zip(("deflate_match_us", "chunk_kernel_us"), c0)]
    out["flow_" + way] = [str(flow.dtype), list(flow.shape)]
out["same"] = same_file(os.path.join(TMP, "host.hdf5"), os.path.join(TMP, "device.hdf5"))
with h5py.File(os.path.join(TMP, "device.hdf5"), "r") as f, h5py.File(os.path.join(TMP, "host.hdf5"), "r") as g:
    out["names"] = sorted(f.keys())
    out["chunks"] = {k: int(f[k].id.get_num_chunks()) for k in f.keys()}
    out["chunk_bytes_equal"] = {k: bool(f[k].id.get_num_chunks() == g[k].id.get_num_chunks() and all(
        f[k].id.read_direct_chunk(g[k].id.get_chunk_info(i).chunk_offset) == g[k].id.read_direct_chunk(g[k].id.get_chunk_info(i).chunk_offset)
        for i in range(g[k].id.get_num_chunks()))) for k in g.keys()}
out["logged"] = list(keep.msgs)
# a model of the call's own is closed before the file is written: the chunks are compressed while it still holds the study
process_video(None, os.path.join(TMP, "own.hdf5"), deflate="device", **{**kw, "flow_model": None})
out["same_own"] = same_file(os.path.join(TMP, "host.hdf5"), os.path.join(TMP, "own.hdf5"))
# gray frames: payload="device" does not serve, so neither does deflate="device": the host's file, one logged reason
gray = dict(kw, nparr=rgb[..., 0].astype(np.float32), mask_dict={"otsu": np.asarray(eng.otsu_masks(rgb, 64))})
for way in ("host", "device"):
    process_video(None, os.path.join(TMP, "gray_" + way + ".hdf5"), deflate=way, **gray)
out["same_gray"] = same_file(os.path.join(TMP, "gray_host.hdf5"), os.path.join(TMP, "gray_device.hdf5"))
out["logged_gray"] = [m for m in keep.msgs if "deflate='device' not used" in m]
eng.close()
print(json.dumps(out))
"""


def test_process_video_device_deflate_writes_the_hosts_file(tmp_path):
    """21 frames of 150 x 170, Otsu masks, on the real engine: deflate="device" against deflate="host", the files byte for byte (all
    but HDF5's own time stamps: tests/payload_cases.py)."""
    import json
    import os
    import subprocess
    if not os.path.exists(IC.PY_H5):
        pytest.skip("no interpreter with h5py")
    env = {**os.environ, "PYTHONDONTWRITEBYTECODE": "1"}
    sys_stdcpp = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"       # conda ships an older libstdc++ than libamdhip64 needs
    if os.path.exists(sys_stdcpp):                                # (in front of whatever the environment preloads already)
        env["LD_PRELOAD"] = ":".join([sys_stdcpp] + ([env["LD_PRELOAD"]] if env.get("LD_PRELOAD") else []))
    script = tmp_path / "video.py"
    script.write_text(VIDEO_SCRIPT.replace("ROOT", repr(IC.ROOT)).replace("TMP", repr(str(tmp_path))))
    r = subprocess.run([IC.PY_H5, str(script)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    g = json.loads(r.stdout.strip().splitlines()[-1])
    assert g["names"] == ["echo", "flow", "otsu"] and min(g["chunks"].values()) > 1, g
    assert g["chunk_bytes_equal"] == {"echo": True, "flow": True, "otsu": True}, g
    assert g["same"] and g["same_own"], g
    assert g["flow_host"] == g["flow_device"] == ["float16", [21, 150, 170, 2]]
    # flow and echo came from the device, read where they are held; the host compressed the mask's chunks and nothing else
    assert g["host_compress"]["host"] == sum(g["chunks"].values()) and g["host_compress"]["device"] == g["chunks"]["otsu"]
    assert g["counters"]["host"] == [0, 0] and min(g["counters"]["device"]) > 0
    assert g["logged"] == []
    assert g["same_gray"] and len(g["logged_gray"]) == 1 and "payload='device' does not serve" in g["logged_gray"][0]
