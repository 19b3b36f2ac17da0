"""A study solved into the held payload with nothing downloaded (tf_calc_seq_rgb_held; DenseFlow.calc_study_held, study_chunks).  The
yardstick is the float16 route, calc_study_payload(hold=True): what it returns and holds is what the new call must hold, bit for bit,
and the chunks study_chunks returns must be zlib.compress(chunk, 9) of those arrays cut on the host.  The held arrays are read back
through held_deflate and the host's zlib.decompress, never through a call of the new route alone.  Small frames: 7 of the odd 37 x 53
(every second flow of the payload starts on an odd 4-byte word) in sub-batches of 3 pairs, so a study crosses sub-batches on the lanes;
4 of 80 x 96 for DeepFlow; once 21 of 150 x 170.  Chunk shapes are passed explicitly (no h5py here)."""
import itertools
import zlib

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests.tvl1_forms import iter_form

pytestmark = pytest.mark.gpu

N, H, W = 7, 37, 53
SCALE = 0.04 * 50
FLOW_CHUNKS, ECHO_CHUNKS = (2, 10, 14, 1), (2, 19, 27)          # neither divides the study: clipped edge chunks on every axis
SPACING = 1 / 50.0


def _frames(n, h, w, seed=0):
    from tee_optical_flow_amd.synth import speckle_sequence
    return np.ascontiguousarray(np.repeat(speckle_sequence(seed + n * 1000 + h + w, n, h, w)[..., None], 3, axis=3))


def _mask(n, h, w):
    yy, xx = np.mgrid[:h, :w]
    m = np.stack([((yy - h / 2 - f / 3) / (0.35 * h)) ** 2 + ((xx - w / 2 + f / 3) / (0.4 * w)) ** 2 < 1 for f in range(n)])
    return np.ascontiguousarray(m[..., None])


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0, max_batch=3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def chained():
    e = T.DenseFlow(device_id=0, max_batch=3)
    e.setUseInitialFlow(True)
    yield e
    e.close()


def _cut(arr, chunks):
    """{chunk offset: the whole chunk's bytes, zero beyond the edge}, as HDF5 stores the array"""
    out = {}
    for off in itertools.product(*[range(0, s, c) for s, c in zip(arr.shape, chunks)]):
        full = np.zeros(chunks, arr.dtype)
        blk = arr[tuple(slice(o, min(o + c, s)) for o, c, s in zip(off, chunks, arr.shape))]
        full[tuple(slice(0, n) for n in blk.shape)] = blk
        out[off] = full.tobytes()
    return out


def _streams(rec):
    blob = np.asarray(rec["blob"], np.uint8)
    coord = np.asarray(rec["coord"]).reshape(-1, len(rec["shape"]))
    return {tuple(int(v) for v in at): blob[int(o):int(o) + int(n)].tobytes() for at, o, n in zip(coord, rec["off"], rec["len"])}


def _inflate(rec):
    """the array a record describes, through the host's zlib"""
    shape, chunks, dt = tuple(rec["shape"]), tuple(rec["chunks"]), np.dtype(rec["dtype"])
    pad = np.zeros([-(-s // c) * c for s, c in zip(shape, chunks)], dt)
    for at, stream in _streams(rec).items():
        pad[tuple(slice(o, o + c) for o, c in zip(at, chunks))] = np.frombuffer(zlib.decompress(stream), dt).reshape(chunks)
    return np.ascontiguousarray(pad[tuple(slice(0, s) for s in shape)])


def _held_arrays(e, echo=True):
    h = e.held
    flow = _inflate(e.held_deflate("flow", (h.N, h.H, h.W, 2)))
    return flow, _inflate(e.held_deflate("echo", (h.n_echo, h.H, h.W))) if echo else None


def _bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), (what, int((a.view(np.uint16) != b.view(np.uint16)).sum()))


def _check_held_equals_f16_route(e, rgb, scale, chain=False):
    n, h, w = rgb.shape[:3]
    flow, echo = e.calc_study_payload(rgb, scale=scale, hold=True, chain=chain)
    iters, stats = e.last_iters().copy(), dict(e.last_stats)
    ref_flow, ref_echo = _held_arrays(e)
    _bits(ref_flow, np.asarray(flow), "the yardstick: what hold=True holds is what it returns")
    _bits(ref_echo, np.asarray(echo), "the yardstick's echo")
    e.release_study()
    units, down = e.counter("queue_units_done"), e.counter("study_download_bytes")
    assert e.calc_study_held(rgb, scale=scale, chain=chain) is None
    assert e.counter("study_download_bytes") == down, "calc_study_held copied flow or echo to the host"
    held = e.held
    assert (held.N, held.H, held.W, held.n_echo, held.masks) == (n, h, w, n, {})
    got_flow, got_echo = _held_arrays(e)
    _bits(got_flow, ref_flow, "held flow")
    _bits(got_echo, ref_echo, "held echo")
    assert np.array_equal(got_flow[n - 1], got_flow[n - 2])
    assert np.array_equal(e.last_iters(), iters), "iteration counts"
    for k in ("n_pairs", "nscales_used", "warps", "inner_iters_total", "outer_iters_total"):
        assert e.last_stats[k] == stats[k], k
    return e.counter("queue_units_done") - units


# ---- 1. the held payload is the float16 route's ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "strips2", "tiles"])
def test_held_payload_equals_the_float16_route(eng, form):
    rgb = _frames(N, H, W)
    if form == "default":
        units = _check_held_equals_f16_route(eng, rgb, SCALE)
        assert units >= 2, "the study did not cross sub-batches on the lanes"
    else:
        with iter_form(eng, form):
            _check_held_equals_f16_route(eng, rgb, SCALE)


@pytest.mark.parametrize("form", ["default", "tiles"])
def test_held_payload_equals_the_float16_route_chained(chained, form):
    rgb = _frames(N, H, W, seed=3)
    steps = chained.counter("chain_steps")
    if form == "default":
        _check_held_equals_f16_route(chained, rgb, SCALE, chain=True)
    else:
        with iter_form(chained, form):
            _check_held_equals_f16_route(chained, rgb, SCALE, chain=True)
    assert chained.counter("chain_steps") - steps == 2 * (N - 1)          # both routes ran as chains


def test_held_payload_equals_the_float16_route_deepflow():
    e = T.createOptFlow_DeepFlow(max_batch=3)
    try:
        rgb = _frames(4, 80, 96)
        flow, echo = e.calc_study_payload(rgb, scale=SCALE, hold=True)
        e.release_study()
        down = e.counter("study_download_bytes")
        e.calc_study_held(rgb, scale=SCALE)
        assert e.counter("study_download_bytes") == down
        got_flow, got_echo = _held_arrays(e)
        _bits(got_flow, np.asarray(flow), "DeepFlow held flow")
        _bits(got_echo, np.asarray(echo), "DeepFlow held echo")
        assert e.last_stats["n_pairs"] == 3
    finally:
        e.close()


# ---- 2. study_chunks: every chunk is zlib's ----------------------------------------------------------------------------------------
def _check_chunks(e, rgb, scale, flow_chunks, echo_chunks):
    flow, echo = (np.asarray(a) for a in e.calc_study_payload(rgb, scale=scale))
    e.release_study()
    down = e.counter("study_download_bytes")
    recs = e.study_chunks(rgb, scale, flow_chunks, echo_chunks)
    assert e.counter("study_download_bytes") == down, "study_chunks copied flow or echo to the host"
    assert sorted(recs) == ["echo", "flow"]
    for name, arr, chunks in (("flow", flow, flow_chunks), ("echo", echo, echo_chunks)):
        rec = recs[name]
        assert sorted(rec) == sorted(A.chunks_record(arr.shape, arr.dtype, chunks, [])), "analysis.chunks_record's layout"
        assert tuple(rec["shape"]) == arr.shape and tuple(rec["chunks"]) == chunks and np.dtype(rec["dtype"]) == np.float16
        assert not np.asarray(rec["filter_mask"]).any()
        want, got = _cut(arr, chunks), _streams(rec)
        assert sorted(got) == sorted(want), f"{name}: chunk offsets"
        assert int(np.asarray(rec["len"], np.uint64).sum()) == np.asarray(rec["blob"]).size
        bad = [at for at in want if got[at] != zlib.compress(want[at], 9)]
        assert not bad, f"{name}: {len(bad)} of {len(want)} chunks are not zlib.compress(chunk, 9), first at {bad[0]}"
    return recs


def test_study_chunks_equal_zlib(eng):
    _check_chunks(eng, _frames(N, H, W, seed=1), SCALE, FLOW_CHUNKS, ECHO_CHUNKS)
    assert (eng.held.N, eng.held.n_echo) == (N, N)             # the study stays held


def test_study_chunks_equal_zlib_21_frames_of_150x170(eng):
    _check_chunks(eng, _frames(21, 150, 170), SCALE, (3, 38, 43, 1), (3, 38, 43))


def test_study_chunks_without_echo(eng):
    rgb = _frames(N, H, W, seed=2)
    flow, _ = eng.calc_study_payload(rgb, scale=SCALE, echo=False)
    recs = eng.study_chunks(rgb, SCALE, FLOW_CHUNKS)
    assert recs["echo"] is None and eng.held.n_echo == 0
    want, got = _cut(np.asarray(flow), FLOW_CHUNKS), _streams(recs["flow"])
    assert all(got[at] == zlib.compress(want[at], 9) for at in want) and len(got) == len(want)
    with pytest.raises(OpticalFlowCalculationError, match="the held study has no echo"):
        eng.held_deflate("echo", ECHO_CHUNKS)
    eng.calc_study_held(rgb, scale=SCALE, echo=False)
    assert eng.held.n_echo == 0
    with pytest.raises(OpticalFlowCalculationError, match="the held study has no echo"):
        eng.held_deflate("echo", ECHO_CHUNKS)


# ---- 3. the download counter -------------------------------------------------------------------------------------------------------
def test_download_counter(eng):
    rgb = _frames(N, H, W)
    c = eng.counter("study_download_bytes")
    assert c >= 0
    eng.calc_study_held(rgb, scale=SCALE)
    eng.study_chunks(rgb, SCALE, FLOW_CHUNKS, ECHO_CHUNKS)
    eng.study_chunks(rgb, SCALE, FLOW_CHUNKS)
    assert eng.counter("study_download_bytes") == c
    # the library copies what it solves: N - 1 flows and N echo frames (pad_last=False returns exactly those; the repeat is the host's)
    flow, echo = eng.calc_study_payload(rgb, scale=SCALE, pad_last=False)
    assert flow.shape[0] == N - 1
    assert eng.counter("study_download_bytes") - c == flow.nbytes + echo.nbytes
    c = eng.counter("study_download_bytes")
    flow, echo = eng.calc_study_payload(rgb, scale=SCALE, pad_last=False, echo=False, hold=True)
    assert echo is None and eng.counter("study_download_bytes") - c == flow.nbytes
    c = eng.counter("study_download_bytes")
    flow32 = eng.calc_study(rgb, scale=SCALE)
    assert eng.counter("study_download_bytes") - c == flow32.nbytes


def _leaves(x):
    if isinstance(x, dict):
        return [v for k in sorted(x) for v in _leaves(x[k])]
    if isinstance(x, (tuple, list)):
        return [v for y in x for v in _leaves(y)]
    return [x]


# ---- 4. a held tail call reads the same bits on both routes ------------------------------------------------------------------------
def test_held_tail_call_gives_the_same_bits_on_both_routes(eng):
    rgb, mask = _frames(N, H, W, seed=4), _mask(N, H, W)
    cent = np.full((N, 2), 17.5)

    def tail():
        eng.hold_mask("rv", mask)
        out = []
        for param in (0, 2):
            mm, nz, rad, lon = eng.held_radlong_project_param("rv", param, SPACING, True, N, cent, return_arrays=True)
            st = A._radlong_stats_resident(eng, N, mm, nz, 1, 99, 40)            # tf_radlong_hist and tf_radlong_select on the planes
            out += [mm, nz, rad, lon] + [np.asarray(v) for k in ("radial", "longitudinal") for v in _leaves(st[k])]
        return out

    eng.calc_study_payload(rgb, scale=SCALE, hold=True)
    ref = tail()
    eng.release_study()
    eng.calc_study_held(rgb, scale=SCALE)
    got = tail()
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), i


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _refused(e, rc, text, code=_lib.TF_ERR_INVALID_ARG):
    msg = e._L.tf_last_error(e._h).decode()
    assert rc == code and text in msg, (rc, msg)


def test_refusals_come_first_and_spend_the_flags(eng, chained):
    rgb = _frames(N, H, W)
    eng.calc_study_held(rgb, scale=SCALE)
    gen, ref = eng.held.generation, _held_arrays(eng)
    up = eng.counter("tail_upload_bytes")
    L = eng._L
    # refused for their arguments: nothing is uploaded, the study held before survives
    _refused(eng, L.tf_calc_seq_rgb_held(eng._h, rgb.ctypes.data, 1, H, W, 1.0, 1, None), "at least 2 frames")
    _refused(eng, L.tf_calc_seq_rgb_held(eng._h, None, N, H, W, 1.0, 1, None), "null image/flow pointer")
    _refused(eng, L.tf_calc_seq_rgb_held(eng._h, rgb.ctypes.data, N, 0, W, 1.0, 1, None), "bad sizes")
    _refused(eng, L.tf_calc_seq_rgb_held(eng._h, rgb.ctypes.data, N, 4097, 4097, 1.0, 1, None), "2^24 pixels", _lib.TF_ERR_UNSUPPORTED)
    assert L.tf_calc_seq_rgb_held(None, rgb.ctypes.data, N, H, W, 1.0, 1, None) == _lib.TF_ERR_INVALID_ARG
    with pytest.raises(OpticalFlowCalculationError, match=r"nparr must be \[N>=2,H,W,3\]"):
        eng.calc_study_held(rgb[:1])
    with pytest.raises(OpticalFlowCalculationError, match=r"nparr must be \[N>=2,H,W,3\]"):
        eng.calc_study_held(rgb[..., :1])
    with pytest.raises(OpticalFlowCalculationError, match=r"nparr must be \[N>=2,H,W,3\]"):
        eng.study_chunks(rgb[..., :1], SCALE, FLOW_CHUNKS, ECHO_CHUNKS)
    assert eng.held.generation == gen and eng.counter("tail_upload_bytes") == up and eng.counter("queue_outstanding") == 0
    for a, b in zip(_held_arrays(eng), ref):
        _bits(a, b, "the held study after the refusals")
    # a refused call spends an armed hold_next: the float16 call after it holds nothing new
    eng.hold_next()
    _refused(eng, L.tf_calc_seq_rgb_held(eng._h, rgb.ctypes.data, 1, H, W, 1.0, 1, None), "at least 2 frames")
    eng.calc_study_payload(rgb, scale=SCALE)
    assert eng.held.generation == gen
    # ... and so does one that succeeds
    eng.hold_next()
    eng.calc_study_held(rgb, scale=SCALE)
    gen = eng.held.generation
    eng.calc_study_payload(rgb, scale=SCALE)
    assert eng.held.generation == gen
    # useInitialFlow without a chain: the solve calls' refusal, before any work; an armed chain flag is spent by the refused call
    chained.calc_study_held(rgb, scale=SCALE, chain=True)
    cgen, steps = chained.held.generation, chained.counter("chain_steps")
    with pytest.raises(OpticalFlowCalculationError, match="useInitialFlow is set") as ei:
        chained.calc_study_held(rgb, scale=SCALE)
    assert ei.value.code == _lib.TF_ERR_UNSUPPORTED
    chained.chain_next()
    _refused(chained, L.tf_calc_seq_rgb_held(chained._h, rgb.ctypes.data, 1, H, W, 1.0, 1, None), "at least 2 frames")
    with pytest.raises(OpticalFlowCalculationError, match="useInitialFlow is set"):
        chained.calc_study_held(rgb, scale=SCALE)
    assert chained.held.generation == cgen and chained.counter("chain_steps") == steps
    # a chain without useInitialFlow: tf_chain_next's refusal, nothing else armed or solved
    with pytest.raises(OpticalFlowCalculationError, match="useInitialFlow is clear"):
        eng.calc_study_held(rgb, scale=SCALE, chain=True)
    assert eng.held.generation == gen
    # tf_hold_next + tf_submit_* stays refused
    eng.hold_next()
    with pytest.raises(OpticalFlowCalculationError, match="held"):
        eng.submit_study_payload(rgb)
    assert eng.held.generation == gen and eng.counter("queue_outstanding") == 0


def test_study_chunks_beside_a_submitted_job(eng):
    """The synchronous study calls may be made while a submitted job is in flight (they queue behind it): so may this one."""
    rgb, other = _frames(N, H, W, seed=5), _frames(6, 33, 47, seed=9)
    ref_other = [np.asarray(a).copy() for a in eng.calc_study_payload(other, scale=0.7)]
    flow, echo = (np.asarray(a).copy() for a in eng.calc_study_payload(rgb, scale=SCALE))
    t = eng.submit_study_payload(other, scale=0.7)
    recs = eng.study_chunks(rgb, SCALE, FLOW_CHUNKS, ECHO_CHUNKS)
    got_other = eng.wait(t)
    for a, b in zip(got_other, ref_other):
        _bits(np.asarray(a), b, "the submitted job's results")
    _bits(_inflate(recs["flow"]), flow, "flow beside a job")
    _bits(_inflate(recs["echo"]), echo, "echo beside a job")
    want, got = _cut(flow, FLOW_CHUNKS), _streams(recs["flow"])
    assert all(got[at] == zlib.compress(want[at], 9) for at in want)
    assert eng.counter("queue_outstanding") == 0
