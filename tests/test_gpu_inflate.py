"""Inflate on the device (tf_inflate, DenseFlow.inflate; kernel k_inflate, one wave per stream) over the corpus of
tests/inflate_cases.py, which the CPU program of tests/test_inflate_cpu.py runs under the sanitizers first.  The yardstick is zlib:
a stream zlib decodes must come out as zlib's bytes with status 0, a stream zlib raises on must have a status, and a stream that ends
early or has another size than asked for must have one too.  A call has one out_bytes for all its streams, so the corpus goes up
grouped by output size, every group in one call; further calls of 1, 3, 4, 5 and 257 streams sit around the waves of a block, the
blocks of a CU and the CUs.  Every call's output is pre-filled with a pattern: a slot holds what its stream decoded and the pattern
behind it, whatever its neighbours did."""
import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests import inflate_cases as IC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0, max_batch=3)
    yield e
    e.close()


def _groups():
    """{out_bytes: [index into cases()]}"""
    g = {}
    for i, c in enumerate(IC.cases()):
        g.setdefault(c.out_bytes, []).append(i)
    return g


def _pattern(n, out_bytes):
    return np.tile(((np.arange(out_bytes) * 7 + 3) & 255).astype(np.uint8), (n, 1))


def _check_call(e, idx, what):
    """one inflate call over cases()[idx] (one out_bytes): every slot against zlib's verdict; returns the statuses"""
    cs, vs = IC.cases(), IC.verdicts()
    out_bytes = cs[idx[0]].out_bytes
    assert all(cs[i].out_bytes == out_bytes for i in idx)
    out = _pattern(len(idx), out_bytes)
    pat = out[0].tobytes() if len(idx) else b""
    got, status = e.inflate([cs[i].stream for i in idx], out_bytes, out=out)
    assert got is out and status.shape == (len(idx),) and status.dtype == np.int32
    wrong = []
    for k, i in enumerate(idx):
        kind, want = vs[i]
        assert 0 <= status[k] <= 8, (what, cs[i].name, status[k])
        slot = out[k].tobytes()
        # a stream that is not good: what zlib decoded of it as far as the slot was written, then the pattern, nothing else
        for msg in (IC.check(cs[i], kind, want, int(status[k]), slot), IC.check_prefix(cs[i], kind, want, slot, IC.written(slot, pat))):
            if msg:
                wrong.append(msg)
    assert not wrong, (what, len(wrong), wrong[:10])
    return status


def test_the_whole_corpus_group_by_group(eng):
    seen = 0
    for out_bytes, idx in sorted(_groups().items()):
        _check_call(eng, idx, f"out_bytes {out_bytes}")
        seen += len(idx)
    assert seen == len(IC.cases())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_calls_of_a_few_and_of_many_streams(eng, n):
    g = _groups()
    for out_bytes in (259, 32769):                            # the header and trailer faults; the long good streams and their settings
        idx = g[out_bytes]
        take = [idx[(k * 5 + n) % len(idx)] for k in range(n)]   # good and bad ones side by side
        _check_call(eng, take, f"{n} streams of {out_bytes}")


def test_a_mixed_call_reports_the_first_bad_stream_and_keeps_the_good_ones(eng):
    cs, vs = IC.cases(), IC.verdicts()
    idx = _groups()[259]
    kinds = [vs[i][0] for i in idx]
    assert IC.GOOD in kinds and IC.BAD in kinds
    out, status = _pattern(len(idx), 259), np.zeros(len(idx), np.int32)
    streams = [cs[i].stream for i in idx]
    lens = np.array([len(s) for s in streams], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.uint64)
    blob = np.frombuffer(b"".join(streams), np.uint8)
    rc = eng._L.tf_inflate(eng._h, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, None, len(idx), 259, out.ctypes.data, status.ctypes.data)
    first = int(np.flatnonzero(status)[0])
    msg = eng._L.tf_last_error(eng._h).decode()
    assert rc == _lib.TF_ERR_INVALID_ARG and f"stream {first} did not inflate: status {status[first]}" in msg, msg
    for k, i in enumerate(idx):
        if kinds[k] == IC.GOOD:
            assert status[k] == 0 and out[k].tobytes() == vs[i][1]
    # raw streams are copied as they are, and must have the slot's size
    plain = IC.data("random", 259)
    streams = [plain, IC.deflate(plain, 9), plain[:100], IC.deflate(plain, 0)]
    lens = np.array([len(s) for s in streams], np.uint32)
    offs = (np.concatenate([[0], np.cumsum(lens[:-1])]) + 5).astype(np.uint64)         # (the blob's first 5 bytes belong to no stream)
    blob = np.frombuffer(b"\xAA" * 5 + b"".join(streams), np.uint8)
    raw = np.array([1, 0, 1, 0], np.uint8)
    out2, status2 = _pattern(4, 259), np.zeros(4, np.int32)
    c0 = eng.counter("tail_upload_bytes")
    rc = eng._L.tf_inflate(eng._h, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, raw.ctypes.data, 4, 259, out2.ctypes.data, status2.ctypes.data)
    assert rc == _lib.TF_ERR_INVALID_ARG and list(status2) == [0, 0, 7, 0]
    assert eng.counter("tail_upload_bytes") - c0 == int(lens.sum())
    assert all(out2[k].tobytes() == plain for k in (0, 1, 3)) and np.array_equal(out2[2], _pattern(1, 259)[0])


def test_junk_in_front_of_the_streams_changes_nothing_at_any_alignment(eng):
    """Four streams of the 259-byte group, good and bad side by side, behind g junk bytes, g = 0 .. 15: the span's first byte sits at
    every offset mod 16 of the blob, and the call gives the bits and statuses of g = 0 and uploads the streams' span, not the junk."""
    cs, vs = IC.cases(), IC.verdicts()
    idx = _groups()[259]
    take = [idx[(k * 5 + 4) % len(idx)] for k in range(4)]
    kinds = [vs[i][0] for i in take]
    assert IC.GOOD in kinds and IC.BAD in kinds
    streams = [cs[i].stream for i in take]
    lens = np.array([len(s) for s in streams], np.uint32)
    first = None
    for g in range(16):
        offs = (np.concatenate([[0], np.cumsum(lens[:-1])]) + g).astype(np.uint64)
        blob = np.frombuffer(b"\xC3" * g + b"".join(streams), np.uint8)
        out, status = _pattern(4, 259), np.zeros(4, np.int32)
        c0 = eng.counter("tail_upload_bytes")
        rc = eng._L.tf_inflate(eng._h, blob.ctypes.data, offs.ctypes.data, lens.ctypes.data, None, 4, 259, out.ctypes.data, status.ctypes.data)
        assert rc == _lib.TF_ERR_INVALID_ARG and status.any(), (g, rc, status)          # (the verdict on the bad ones)
        assert eng.counter("tail_upload_bytes") - c0 == int(lens.sum()), g
        if first is None:
            first = out.copy(), status.copy()
            for k, i in enumerate(take):
                assert IC.check(cs[i], vs[i][0], vs[i][1], int(status[k]), out[k].tobytes()) is None, cs[i].name
        assert np.array_equal(out, first[0]) and np.array_equal(status, first[1]), g


def test_python_form_returns_zeros_behind_a_failed_stream(eng):
    cs, vs = IC.cases(), IC.verdicts()
    idx = _groups()[4099]
    out, status = eng.inflate([cs[i].stream for i in idx], 4099)
    assert out.shape == (len(idx), 4099) and out.dtype == np.uint8 and status.dtype == np.int32
    assert [int(s) != 0 for s in status] == [vs[i][0] != IC.GOOD for i in idx]
    out0, st0 = eng.inflate([], 10)
    assert out0.shape == (0, 10) and st0.shape == (0,)
    out1, st1 = eng.inflate([cs[i].stream for i in _groups()[0]], 0)
    assert out1.shape[1] == 0 and [int(s) != 0 for s in st1] == [vs[i][0] != IC.GOOD for i in _groups()[0]]


def test_refusals_come_before_any_gpu_work(eng):
    L, h = eng._L, eng._h
    one = np.zeros(64, np.uint8)
    off, ln, st = np.zeros(2, np.uint64), np.full(2, 4, np.uint32), np.full(2, -5, np.int32)
    out = np.full((2, 8), 7, np.uint8)
    c0 = [eng.counter(k) for k in ("tail_upload_bytes", "inflate_kernel_us")]
    good = dict(blob=one.ctypes.data, off=off.ctypes.data, len=ln.ctypes.data, n=2, out_bytes=8, out=out.ctypes.data, st=st.ctypes.data)

    def call(**kw):
        a = {**good, **kw}
        return L.tf_inflate(h, a["blob"], a["off"], a["len"], None, a["n"], a["out_bytes"], a["out"], a["st"])
    huge = np.array([0, 1 << 31], np.uint32)
    far = np.array([0, 1 << 63], np.uint64)
    for bad, text in ((dict(blob=None), "null blob"), (dict(off=None), "null blob"), (dict(len=None), "null blob"), (dict(n=-1), "n = -1"),
                      (dict(out=None), "null out_host"), (dict(st=None), "null out_host"), (dict(out_bytes=(1 << 30) + 1), "output bytes per stream"),
                      (dict(len=huge.ctypes.data), "stream 1 has"), (dict(off=far.ctypes.data), "stream 1 starts")):
        assert call(**bad) == _lib.TF_ERR_INVALID_ARG, bad
        assert text in L.tf_last_error(h).decode(), (bad, L.tf_last_error(h))
    assert call(n=0) == _lib.TF_OK
    assert (out == 7).all() and (st == -5).all()
    assert [eng.counter(k) for k in ("tail_upload_bytes", "inflate_kernel_us")] == c0
    with pytest.raises(OpticalFlowCalculationError, match="out must be"):
        eng.inflate([b"x"], 4, out=np.zeros((2, 4), np.uint8))
    with pytest.raises(OpticalFlowCalculationError, match="out_bytes"):
        eng.inflate([b"x"], -1)
    # the call that follows the refusals works, and counts what it uploads and runs
    idx = _groups()[258]
    _check_call(eng, idx, "after the refusals")
    assert eng.counter("tail_upload_bytes") - c0[0] == sum(len(IC.cases()[i].stream) for i in idx)
    assert eng.counter("inflate_kernel_us") > c0[1]


def test_a_second_engine_and_a_call_beside_a_job_in_flight(eng):
    from tee_optical_flow_amd.synth import speckle_sequence
    idx = _groups()[73728][:40]
    ref = _check_call(eng, idx, "first engine")
    other = T.DenseFlow(device_id=0)
    try:
        assert np.array_equal(_check_call(other, idx, "second engine"), ref)
    finally:
        other.close()
    rgb = np.ascontiguousarray(np.repeat(speckle_sequence(5, 6, 40, 52)[..., None], 3, axis=3))
    sync = eng.calc_study_payload(rgb)
    t = eng.submit_study_payload(rgb)
    got = _check_call(eng, idx, "with a job in flight")
    flow, echo = eng.wait(t)
    assert np.array_equal(got, ref) and np.array_equal(flow, sync[0]) and np.array_equal(echo, sync[1])
