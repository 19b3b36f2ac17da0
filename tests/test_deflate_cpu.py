"""Deflate without a GPU: the recorded digests against the running zlib, the corpus against what it claims to hold, the compressor's
core (csrc/teeflow_deflate_core.h, the text the device kernels run) in a stand-alone program built with the address and
undefined-behaviour sanitizers over the whole corpus of tests/deflate_cases.py and its sweeps, the chunk bookkeeping and the writer's deflater hook
on a zlib-backed engine, and the refusals that need no device."""
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_cases as DC
from tests import inflate_cases as IC
from tests.numpy_engine import NumpyEngine

ROOT, PY_H5 = IC.ROOT, IC.PY_H5


# ---- 1. the yardstick -------------------------------------------------------------------------------------------------------------------
def test_the_running_zlib_reproduces_the_recorded_digests():
    """a machine whose zlib writes other level-9 streams than 1.2.11 fails here, not in the kernel's test"""
    want = DC.digests()
    assert sorted(want) == sorted(c.name for c in DC.cases())
    wrong = [c.name for c in DC.cases() if DC.digest(zlib.compress(c.raw, 9)) != want[c.name]]
    assert not wrong, (zlib.ZLIB_RUNTIME_VERSION, wrong[:10])
    assert sorted(DC.sweep_digests()) == DC.SWEEP_SIZES
    for n in DC.SWEEP_SIZES:
        assert len(DC.sweep(n)) == DC.SWEEP_COUNT and {len(c) for c in DC.sweep(n)} == {n}
        assert DC.sweep_digest([zlib.compress(c, 9) for c in DC.sweep(n)]) == DC.sweep_digests()[n], (zlib.ZLIB_RUNTIME_VERSION, n)


def test_corpus_has_every_case_the_compressor_must_meet():
    """a check of the corpus itself: zlib's streams over it hold stored, fixed and dynamic blocks, blocks of exactly 16,383 symbols,
    multi-block streams, and the boundary cases change zlib's output where they are meant to"""
    by = {c.name: c.raw for c in DC.cases()}
    for fam in IC.FAMILIES:
        for n in DC.SIZES:
            assert len(by[f"{fam}-{n}"]) == n
    assert set(IC.SIZES) <= set(DC.SIZES) and all(len(by[f"tiny-{n}"]) < 100 for n in (5, 19, 64, 99))

    def z(name):
        return zlib.compress(by[name], 9)
    kinds = {name: DC.blocks(z(name)) for name in ("zeros-0", "tiny-19", "tiny-99", "random-259", "f16noise-32505", "counter-16396", "counter-16397",
                                                   "counter-16398", "counter-16399", "counter-40000", "fibdist", "fibdist-bl", "lloverflow-16",
                                                   "lloverflow-17", "prefix-slide-73728", "random-140000")}
    for name, (bl, _) in kinds.items():
        assert sum(b[2] for b in bl) == len(by[name]), name
    ks = {name: [b[:2] for b in bl] for name, (bl, _) in kinds.items()}
    assert ks["zeros-0"] == [(1, 0)] and ks["tiny-19"] == [(1, 19)] and ks["tiny-99"][0][0] == 1                # fixed
    assert ks["random-259"] == [(0, 259)]                                                                       # stored
    assert [k for k, _ in ks["f16noise-32505"]] == [2, 2]                                                       # dynamic
    assert ks["counter-16396"] == [(2, 16382)] and ks["counter-16397"] == [(2, 16383)]
    assert ks["counter-16398"] == [(2, 16383), (1, 1)] and ks["counter-16399"] == [(2, 16383), (1, 2)]
    assert ks["counter-40000"][:2] == [(2, 16383), (2, 16383)] and len(ks["counter-40000"]) == 3
    assert len(ks["random-140000"]) > 5 and {k for k, _ in ks["random-140000"]} == {0}                          # stored blocks behind two slides
    # a full block over the random prefix, then one that begins below 32,768 and is flushed at the end, behind the slide at 65,275
    first, second = kinds["prefix-slide-73728"][0]
    assert first[:2] == (2, 16383) and 16000 < first[2] < 32768 and second[0] == 2 and first[2] + second[2] == 73728
    # the trees that must be repaired: their Huffman depth, from the frequencies zlib's own stream shows, passes the limit, and the
    # stream's codes sit at it
    last = kinds["fibdist"][0][-1]
    assert DC.huffman_depth(last[4]) > 15
    last = kinds["fibdist-bl"][0][-1]
    assert DC.huffman_depth(last[5]) > 7 and kinds["fibdist-bl"][1][1] == 7
    # ... the literal/length tree's: a last block of matches alone, short of a full one, whose deepest code has the limit's 15 bits
    for name, depth in (("lloverflow-16", 16), ("lloverflow-17", 17)):
        last = kinds[name][0][-1]
        assert last[0] == 2 and DC.huffman_depth(last[3]) >= depth and last[6][0] == 15 and last[1] < 16383, (name, DC.huffman_depth(last[3]), last[6], last[1])
        assert sum(last[3][:256]) == 0 and [b[0] for b in kinds[name][0][:-1]].count(1) == 0, name
    # different three-byte strings of one hash inside the 64 positions that the device links in one step, in nearly every step
    for n in DC.COLLIDE:
        raw = by[f"collide-{n}"]
        assert len(raw) == n and len({b & 31 for b in raw}) == DC.COLLIDE[n] and len({b >> 5 for b in raw}) == 8
        assert DC.colliding_steps(raw) >= 1 and DC.colliding_steps(raw) > n // 64 // 2, (n, DC.colliding_steps(raw))
        assert len(zlib.compress(raw, 9)) < 0.7 * n                                                             # real matches
    assert DC.colliding_steps(by["seven-73728"]) == 0 == DC.colliding_steps(by["slide0-65400-65274"])         # what the corpus had
    # the window's first position as a chain's head: not a match where the input ends behind it, a match where it goes on
    for n, p in DC.SLIDE0:
        raw = by[f"slide0-{n}-{p}"]
        assert len(raw) == n and raw.count(bytes([31, 31, 30])) == 2 and raw[p - 32506:p - 32506 + 24] == raw[p:p + 24] and (p - 32506) % 32768 == 0
    assert [n - p < 262 for n, p in DC.SLIDE0] == [True, True, True, True, False, False]
    # the boundaries move zlib's output: a 3-byte match 4,096 back is taken, 4,097 back dropped; a chain's head 32,506 back is admitted,
    # 32,507 is not; the long match is found as candidate 4,095 and 1,023 and missed one later
    assert len(z("far3-4096")) != len(z("far3-4097")) and len(z("dist-32506")) < len(z("dist-32507"))
    assert len(z("chain-4095-short")) < len(z("chain-4096-short")) and len(z("chain-1023-long")) < len(z("chain-1024-long"))
    assert len(z("chain-1023-short")) == len(z("chain-1022-short")) and len(z("chain-4094-short")) == len(z("chain-4095-short"))


# ---- 2. the core under the sanitizers --------------------------------------------------------------------------------------------------
def test_core_reproduces_zlib_over_the_corpus_under_the_sanitizers(tmp_path):
    exe = tmp_path / "verify_deflate"
    subprocess.check_call(["g++", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_deflate.cpp"), "-o", str(exe)])
    corpus, want = DC.cases(), DC.digests()
    # the corpus, then the sweeps' chunks, which are judged by their size's one digest
    cs = list(corpus) + [DC.Case((n, i), c) for n in DC.SWEEP_SIZES for i, c in enumerate(DC.sweep(n))]
    swept = {n: [None] * DC.SWEEP_COUNT for n in DC.SWEEP_SIZES}
    # the search walks up to 4,096 candidates for every byte: the corpus goes through the program in four parts side by side
    order = sorted(range(len(cs)), key=lambda i: -len(cs[i].raw))
    parts = [order[k::4] for k in range(4)]
    procs = []
    for k, part in enumerate(parts):
        with open(tmp_path / f"corpus{k}.bin", "wb") as f:
            f.write(struct.pack("<I", len(part)))
            for i in part:
                f.write(struct.pack("<I", len(cs[i].raw)))
                f.write(cs[i].raw)
        procs.append(subprocess.Popen([str(exe), str(tmp_path / f"corpus{k}.bin"), str(tmp_path / f"result{k}.bin")], stderr=subprocess.PIPE, text=True))
    wrong, seen = [], 0
    for k, (part, p) in enumerate(zip(parts, procs)):
        _, err = p.communicate()
        assert p.returncode == 0 and err == "", err[-3000:]
        buf, at = open(tmp_path / f"result{k}.bin", "rb").read(), 0
        for i in part:
            status, n, clean = struct.unpack_from("<iII", buf, at)
            got = buf[at + 12:at + 12 + n]
            at += 12 + n
            seen += 1
            bound = len(cs[i].raw) + (len(cs[i].raw) >> 12) + (len(cs[i].raw) >> 14) + (len(cs[i].raw) >> 25) + 13
            assert status == 0 and n <= bound and clean == 1, (cs[i].name, status, n, clean)
            if i >= len(corpus):
                swept[cs[i].name[0]][cs[i].name[1]] = got
            elif DC.digest(got) != want[cs[i].name]:
                wrong.append((cs[i].name, n, want[cs[i].name][0]))
        assert at == len(buf)
    assert seen == len(cs) and not wrong, (len(wrong), wrong[:10])
    for n, streams in swept.items():
        if DC.sweep_digest(streams) != DC.sweep_digests()[n]:
            wrong.append((n, DC.first_difference(DC.sweep(n), streams)))
    assert not wrong, f"sweeps (size, (first differing chunk, its family, bytes made, zlib's bytes)): {wrong}"


# ---- 3. chunk bookkeeping and the writer's hook, on a zlib-backed engine ---------------------------------------------------------------
class ZlibEngine(NumpyEngine):
    """NumpyEngine with DenseFlow's three deflate methods, the streams made by zlib: the engine the glue is tested on"""

    @staticmethod
    def _streams(chunks):
        from tee_optical_flow_amd import DenseFlow
        chunks = [bytes(c) for c in chunks]
        if len({len(c) for c in chunks}) > 1:
            raise ValueError("one size per call")
        streams = [zlib.compress(c, 9) for c in chunks]
        ln = np.array([len(s) for s in streams], np.uint32)
        off = np.zeros(len(streams), np.uint64)
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        assert all(n <= DenseFlow.deflate_bound(len(c)) for n, c in zip(ln, chunks))
        return np.frombuffer(b"".join(streams), np.uint8), off, ln

    def deflate(self, chunks):
        self.calls.append("deflate")
        return self._streams(chunks)

    def deflate_array(self, arr, chunks, _call="deflate_array"):
        from tee_optical_flow_amd import DenseFlow
        self.calls.append(_call)
        arr = np.ascontiguousarray(arr)
        shape, chunks, n = DenseFlow._chunk_grid(arr.shape, chunks, _call)
        coord, raw = [], []
        at = [0] * len(shape)
        for _ in range(n):                                       # the library's walk: the last dimension moves first
            full = np.zeros(chunks, arr.dtype)
            sl = tuple(slice(o, min(o + c, s)) for o, c, s in zip(at, chunks, shape))
            full[tuple(slice(0, s.stop - s.start) for s in sl)] = arr[sl]
            coord.append(list(at))
            raw.append(full.tobytes())
            for d in range(len(shape) - 1, -1, -1):
                at[d] += chunks[d]
                if at[d] < shape[d]:
                    break
                at[d] = 0
        blob, off, ln = self._streams(raw)
        return DenseFlow._deflated_record(shape, arr.dtype, chunks, blob, off, ln, np.array(coord, np.int64).reshape(n, len(shape)))

    def held_deflate(self, what, chunks):
        arr = self.flow if what == "flow" else self.echo if what == "echo" else self.masks[what]
        if arr is None:
            raise ValueError(f"no {what} is held")
        return self.deflate_array(arr, chunks, _call="held_deflate")


CHUNKINGS = [((5, 37, 53, 2), (2, 16, 16, 1), np.float16), ((5, 37, 53), (3, 10, 27), np.float16), ((4, 6, 8, 2), (4, 6, 8, 2), np.bool_)]


@pytest.mark.parametrize("shape,chunks,dtype", CHUNKINGS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_deflate_array_bookkeeping_equals_the_chunks_of_a_file(shape, chunks, dtype):
    from tee_optical_flow_amd import analysis as A
    rng = np.random.default_rng(sum(shape))
    arr = (rng.random(shape) < 0.4) if dtype == np.bool_ else rng.normal(0, 40, shape).astype(dtype)
    want, _ = IC.chunked(arr, chunks, level=9)
    e = ZlibEngine()
    got = e.deflate_array(arr, chunks)
    assert e.calls == ["deflate_array"]
    assert tuple(got["shape"]) == tuple(want["shape"]) and tuple(got["chunks"]) == tuple(want["chunks"]) and got["dtype"] == want["dtype"]
    for k in ("coord", "off", "len", "blob", "filter_mask"):
        assert np.array_equal(np.asarray(got[k]).reshape(np.asarray(want[k]).shape), want[k]), k
    assert np.array_equal(A.unchunk_host(got).view(np.uint8), arr.view(np.uint8))
    if dtype == np.float16 and len(shape) == 4:
        e.hold_study(arr)
        held = e.held_deflate("flow", chunks)
        assert np.array_equal(held["blob"], want["blob"]) and e.calls[-1] == "held_deflate"


def test_device_deflater_takes_flow_and_echo_from_the_held_study(monkeypatch):
    from tee_optical_flow_amd import hdf5_out, pipeline
    rng = np.random.default_rng(3)
    flow, echo = rng.normal(0, 2, (5, 37, 53, 2)).astype(np.float16), rng.integers(0, 256, (5, 37, 53)).astype(np.float16)
    mask = rng.random((5, 37, 53, 2)) < 0.5
    chunkings = {4: (2, 16, 16, 1), 3: (3, 10, 27)}
    monkeypatch.setattr(hdf5_out, "auto_chunks", lambda shape, dtype: chunkings[len(shape)])
    e = ZlibEngine()
    e.hold_study(flow, echo)
    e.calls.clear()
    d = pipeline._device_deflater(e, flow, echo)
    assert e.calls == ["held_deflate", "held_deflate"]
    for name, arr in (("flow", flow), ("echo", echo)):
        rec = d(name, arr, chunkings[arr.ndim])
        assert np.array_equal(rec["blob"], IC.chunked(arr, chunkings[arr.ndim], level=9)[0]["blob"]), name
    # what it has no record of (the masks, the waveforms), or a record of another layout, stays with the host
    assert d("rv", mask, chunkings[4]) is None and d("ecg", np.zeros(100, np.float16), (100,)) is None
    assert d("flow", flow, (1, 16, 16, 1)) is None and d("flow", flow.astype(np.float32), chunkings[4]) is None
    e.calls.clear()
    assert pipeline._device_deflater(e, flow, None)("echo", echo, chunkings[3]) is None and e.calls == ["held_deflate"]


# ---- 4. refusals that need no device ---------------------------------------------------------------------------------------------------
def test_python_refusals():
    from tee_optical_flow_amd import DenseFlow, pipeline
    from tee_optical_flow_amd.exceptions import ConfigurationError, OpticalFlowCalculationError
    for shape, chunks in (((2, 3), (1,)), ((2, 3), (0, 1)), ((), ()), ((1, 2, 3, 4, 5), (1, 1, 1, 1, 1))):
        with pytest.raises(OpticalFlowCalculationError, match="chunk extents"):
            DenseFlow._chunk_grid(shape, chunks, "deflate_array")
    assert DenseFlow._chunk_grid((5, 37, 53, 2), (2, 16, 16, 1), "x") == ((5, 37, 53, 2), (2, 16, 16, 1), 3 * 3 * 4 * 2)
    assert [DenseFlow.deflate_bound(n) for n in (0, 1, 73728, 1 << 25)] == [13, 14, 73728 + 18 + 4 + 13, (1 << 25) + 8192 + 2048 + 1 + 13]
    with pytest.raises(ConfigurationError, match="deflate must be"):
        pipeline._check_deflate("gpu", "device")
    with pytest.raises(ConfigurationError, match="needs payload='device'"):
        pipeline._check_deflate("device", "host")
    pipeline._check_deflate("host", "host")
    pipeline._check_deflate("device", "device")
    with pytest.raises(ConfigurationError, match="needs payload='device'"):
        pipeline.process_video(None, None, nparr=np.zeros((3, 8, 8, 3), np.uint8), mode="otsu", deflate="device")


def test_entry_points_refuse_a_null_handle_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    raw = np.zeros((2, 8), np.uint8)
    blob, off, ln, st = np.full(64, 7, np.uint8), np.full(2, 9, np.uint64), np.full(2, 9, np.uint32), np.full(2, -5, np.int32)
    coord, sh, ch = np.full((2, 2), -3, np.int64), np.array([2, 8], np.int64), np.array([1, 8], np.int64)
    assert L.tf_deflate(None, raw.ctypes.data, 2, 8, blob.ctypes.data, 64, off.ctypes.data, ln.ctypes.data, st.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_deflate_array(None, raw.ctypes.data, 2, sh.ctypes.data, ch.ctypes.data, 1, 2, blob.ctypes.data, 64, off.ctypes.data, ln.ctypes.data,
                              coord.ctypes.data, st.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_held_deflate(None, _lib.HELD_FLOW, 0, ch.ctypes.data, 2, blob.ctypes.data, 64, off.ctypes.data, ln.ctypes.data, coord.ctypes.data,
                             st.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert (blob == 7).all() and (off == 9).all() and (ln == 9).all() and (st == -5).all() and (coord == -3).all()
    assert {"tf_deflate", "tf_deflate_array", "tf_held_deflate"} <= set(_lib.EXPORTED_SYMBOLS)


# ---- 5. a file written through the hook, in the interpreter that has h5py -------------------------------------------------------------
H5_DRIVER = r"""
import sys, json, os, zlib, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tee_optical_flow_amd import hdf5_out
from tests.test_deflate_cpu import ZlibEngine

rng = np.random.default_rng(11)
N, H, W = 7, 150, 170
arrays = {"flow": np.cumsum(rng.normal(0, 0.1, (N, H, W, 2)), axis=2).astype(np.float16), "echo": rng.integers(0, 256, (N, H, W)).astype(np.float16),
          "rv": rng.random((N, H, W, 2)) < 0.5, "small": np.arange(40, dtype=np.float16)}
e = ZlibEngine()
asked = []
def deflater(name, data, chunks):
    asked.append(name)
    return None if name == "small" else e.deflate_array(data, chunks)
real = zlib.compress
for path, hook in ((os.path.join(TMP, "host.hdf5"), None), (os.path.join(TMP, "hook.hdf5"), deflater)):
    with h5py.File(path, "w") as f:
        for k, a in arrays.items():
            hdf5_out.create_gzip9(f, k, a, min_parallel_bytes=0, deflater=hook)
out = {"asked": list(asked), "same": {}, "auto": list(hdf5_out.auto_chunks(arrays["flow"].shape, np.float16))}
with h5py.File(os.path.join(TMP, "host.hdf5"), "r") as a, h5py.File(os.path.join(TMP, "hook.hdf5"), "r") as b:
    out["flow_chunks"] = list(a["flow"].chunks)
    for k in arrays:
        x, y = a[k], b[k]
        same = x.chunks == y.chunks and x.dtype == y.dtype and x.shape == y.shape and x.compression == y.compression == "gzip"
        same = same and x.compression_opts == y.compression_opts == 9 and x.id.get_create_plist().get_nfilters() == y.id.get_create_plist().get_nfilters() == 1
        same = same and x.id.get_num_chunks() == y.id.get_num_chunks() and np.array_equal(x[()].view(np.uint8), y[()].view(np.uint8))
        same = same and np.array_equal(y[()].view(np.uint8), arrays[k].view(np.uint8))
        for i in range(x.id.get_num_chunks()):
            at = x.id.get_chunk_info(i).chunk_offset
            same = same and x.id.read_direct_chunk(at) == y.id.read_direct_chunk(at)
        out["same"][k] = bool(same)
# while a deflater serves, the host compresses nothing
count = [0]
def counting(*a, **k):
    count[0] += 1
    return real(*a, **k)
rec = e.deflate_array(arrays["flow"], tuple(out["flow_chunks"]))
hdf5_out.zlib.compress = counting
with h5py.File(os.path.join(TMP, "again.hdf5"), "w") as f:
    hdf5_out.create_gzip9(f, "flow", arrays["flow"], min_parallel_bytes=0, deflater=lambda n, d, c: rec)
out["host_compress_calls"] = count[0]
# under min_parallel_bytes (1 MiB by default) HDF5's own filter writes the dataset whoever compresses the larger ones
hdf5_out.zlib.compress = real
asked.clear()
with h5py.File(os.path.join(TMP, "default.hdf5"), "w") as f:
    hdf5_out.create_gzip9(f, "flow", arrays["flow"], deflater=deflater)
    big = np.tile(arrays["flow"], (2, 1, 1, 1))
    hdf5_out.create_gzip9(f, "big", big, deflater=deflater)
    out["default"] = [list(asked), arrays["flow"].nbytes < (1 << 20) <= big.nbytes, bool(np.array_equal(f["flow"][()].view(np.uint8), arrays["flow"].view(np.uint8)))]
try:
    with h5py.File(os.path.join(TMP, "bad.hdf5"), "w") as f:
        hdf5_out.create_gzip9(f, "flow", arrays["flow"], min_parallel_bytes=0, deflater=lambda n, d, c: dict(rec, chunks=(1, 1, 1, 1)))
    out["bad"] = "accepted"
except Exception as ex:
    out["bad"] = f"{type(ex).__name__}: {ex}"
print(json.dumps(out))
"""


def test_a_file_written_through_the_deflater_is_the_hosts_file(tmp_path):
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    script = H5_DRIVER.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp_path)))
    r = subprocess.run([PY_H5, "-c", script], capture_output=True, text=True, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    g = json.loads(r.stdout.strip().splitlines()[-1])
    assert g["asked"] == ["flow", "echo", "rv", "small"]
    assert g["same"] == {"flow": True, "echo": True, "rv": True, "small": True}
    assert g["auto"] == g["flow_chunks"] and g["host_compress_calls"] == 0
    assert g["default"] == [["big"], True, True]
    assert g["bad"].startswith("OpticalFlowError") and "in chunks of" in g["bad"]
