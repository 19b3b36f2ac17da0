"""The study file's float16 payload from the device (reference calculate_optical_flow.py:400-404 casts `flow` and `echo` at write time):
the output kernels' float32 -> float16 rounding, the `echo` kernel's single float64 -> float16 rounding, the float16 study calls of both
solvers against the float32 calls of the same engine, and process_folder(payload="device") against payload="host", file against file."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY_H5 = "/opt/conda/bin/python3.9"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _half(a32):
    with np.errstate(over="ignore"):
        return np.asarray(a32, np.float32).astype(np.float16)


def _round_on_device(engine, x, scale):
    from tee_optical_flow_amd import _lib
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.size, np.uint16)
    _lib.check(_lib.load().tf_dbg_f16_round(engine._h, x.ctypes.data, x.size, C.c_float(scale), out.ctypes.data), engine._h, "tf_dbg_f16_round")
    return out


# ---- 1. the rounding of the output kernels ----------------------------------------------------------------------------------------
def test_rounding_of_every_half_its_midpoints_and_their_neighbours(engine):
    """scale = 1: every finite float16 of both signs, the exact midpoint to its successor (a float32), and nextafter of that midpoint
    in each direction, against numpy's astype, as bits."""
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)           # +0 .. 65504
    succ = np.append(h[1:], np.float32(65536.0))                                            # 65504's successor would be 2^16
    mid = (h.astype(np.float64) + succ.astype(np.float64)) / 2
    assert np.array_equal(mid, mid.astype(np.float32).astype(np.float64))                   # representable, as claimed
    mid = mid.astype(np.float32)
    pos = np.concatenate([h, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(0))])
    x = np.concatenate([pos, -pos])
    got = _round_on_device(engine, x, 1.0)
    exp = _bits(_half(x * np.float32(1)))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(exp[i])) for i in bad[:8]]


def test_rounding_named_cases(engine):
    f32 = np.float32
    cases = [(2.0 ** -25, 0x0000), (2.0 ** -25 * (1 + 2.0 ** -23), 0x0001), (3 * 2.0 ** -25, 0x0002), (-2.0 ** -25, 0x8000),
             (6.1e-5, 0x03FF), (65504.0, 0x7BFF), (65519.99, 0x7BFF), (65520.0, 0x7C00), (np.inf, 0x7C00), (-np.inf, 0xFC00),
             (-65520.0, 0xFC00), (1e-40, 0x0000), (-1e-40, 0x8000), (0.0, 0x0000), (-0.0, 0x8000)]
    x = np.array([c[0] for c in cases], f32)
    assert x[1] > x[0] and 0 < abs(x[11]) < np.finfo(f32).tiny                              # the inputs are what their names say
    want = np.array([c[1] for c in cases], np.uint16)
    assert np.array_equal(_bits(_half(x * f32(1))), want)                                   # numpy agrees with the issue's table
    got = _round_on_device(engine, x, 1.0)
    assert np.array_equal(got, want), [(float(a), hex(g), hex(w)) for a, g, w in zip(x, got, want) if g != w]
    nan = np.array([np.nan, -np.nan, np.float32(np.nan)], f32)
    nan = np.concatenate([nan, np.array([0x7F800001, 0xFFC12345], np.uint32).view(f32)])    # a signalling and a payload NaN
    assert np.isnan(_round_on_device(engine, nan, 1.0).view(np.float16)).all()


def test_rounding_multiplies_in_float32_then_converts(engine):
    """scale = float32(0.1) on 10^5 seeded values in +-70000: two roundings, numpy's order; a fused multiply-and-convert rounds once."""
    rng = np.random.default_rng(12)
    x = rng.uniform(-70000, 70000, 100000).astype(np.float32)
    s = np.float32(0.1)
    exp = _bits(_half(x * s))
    fused = _bits((x.astype(np.float64) * np.float64(s)).astype(np.float16))               # the exact product, rounded once
    assert (fused != exp).any()                                                            # precondition: the two orders differ here
    got = _round_on_device(engine, x, float(s))
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(exp[i])) for i in bad[:8]]


# ---- 2. echo ----------------------------------------------------------------------------------------------------------------------
def test_echo_of_the_whole_rgb_cube(engine):
    from tee_optical_flow_amd.frames import rgb2gray
    r = np.arange(256, dtype=np.uint8)
    cube = np.stack(np.broadcast_arrays(r[:, None, None], r[None, :, None], r[None, None, :]), -1)   # frame R, row G, column B
    cube = np.ascontiguousarray(cube)
    luma = rgb2gray(cube)
    exp = luma.astype(np.float16)
    via32 = luma.astype(np.float32).astype(np.float16)
    assert int((_bits(via32) != _bits(exp)).sum()) >= 1000                                  # precondition: rounding through float32 would show
    got = engine.echo_frames(cube)
    assert got.dtype == np.float16 and got.shape == (256, 256, 256)
    bad = np.argwhere(_bits(got) != _bits(exp))
    assert bad.size == 0, (len(bad), bad[:8].tolist())


def test_echo_of_a_gray_study_and_of_an_odd_frame(engine):
    from tee_optical_flow_amd.frames import rgb2gray
    from tee_optical_flow_amd.pipeline import _prep_frames
    from tee_optical_flow_amd.synth import speckle_sequence
    gray = speckle_sequence(3, 4, 48, 56)
    rgb = np.ascontiguousarray(_prep_frames(gray, False))
    assert rgb.shape == (4, 48, 56, 3)
    assert np.array_equal(_bits(engine.echo_frames(rgb)), _bits(rgb2gray(rgb).astype(np.float16)))
    odd = np.random.default_rng(5).integers(0, 256, (1, 37, 53, 3), dtype=np.uint8)         # 1961 pixels: a tail of one
    assert np.array_equal(_bits(engine.echo_frames(odd)), _bits(rgb2gray(odd).astype(np.float16)))
    odd3 = np.random.default_rng(6).integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)        # 5883 pixels: a tail of three
    assert np.array_equal(_bits(engine.echo_frames(odd3)), _bits(rgb2gray(odd3).astype(np.float16)))


# ---- 3. flows ---------------------------------------------------------------------------------------------------------------------
SCALES = (1.0, 1e-4, 3e4)


def _study(seed, N, H, W):
    from tee_optical_flow_amd.synth import speckle_sequence
    return np.ascontiguousarray(np.repeat(speckle_sequence(seed, N, H, W)[..., None], 3, axis=3))


@pytest.fixture(scope="module")
def studies():
    """(TVL1 41 x 67, DeepFlow 55 x 123 -- the smallest odd-width size test_gpu_deepflow.py solves), 11 frames each; made once"""
    return {"TVL1": _study(31, 11, 41, 67), "deepflow": _study(32, 11, 55, 123)}


def _engine(algo, **kw):
    import tee_optical_flow_amd as T
    return T.DenseFlow(device_id=0, max_batch=4, **({"algo": "deepflow"} if algo == "deepflow" else {}), **kw)


def _check_payload_call(eng, rgb, scale, pad_last, preconditions=False):
    """calc_study_payload against the float32 call of the same engine, then astype: bits, iteration counts, the echo"""
    from tee_optical_flow_amd.frames import rgb2gray
    ref = eng.calc_study(rgb, scale=scale, pad_last=pad_last)
    it = eng.last_iters().copy() if eng.algo == "TVL1" else None                            # (DeepFlow has no iteration counts)
    exp = _half(ref)
    if preconditions and scale == 3e4:
        assert np.isinf(exp).any()                                                          # precondition: this scale overflows float16
    if preconditions and scale == 1e-4:
        sub = (exp != 0) & (np.abs(exp) < np.finfo(np.float16).tiny)
        assert sub.any()                                                                    # precondition: ... and this one gives subnormal halves
    f16, e16 = eng.calc_study_payload(rgb, scale=scale, pad_last=pad_last)
    assert f16.dtype == np.float16 and f16.shape == ref.shape
    bad = np.argwhere(_bits(f16) != _bits(exp))
    assert bad.size == 0, (len(bad), bad[:6].tolist())
    assert it is None or np.array_equal(eng.last_iters(), it)
    assert e16.dtype == np.float16 and np.array_equal(_bits(e16), _bits(rgb2gray(rgb).astype(np.float16)))
    return exp


@pytest.mark.parametrize("lanes", [0, None])
@pytest.mark.parametrize("algo", ["TVL1", "deepflow"])
def test_float16_flows_equal_the_float32_call_rounded(studies, algo, lanes):
    """max_batch = 4.  N = 11: 10 pairs in 3 sub-batches -- both staging halves are used again and the third waits for the first's
    copy-out; with the default lanes the units land in their own slices of the destination.  N = 4: one sub-batch (with lanes: the
    contiguous split).  N = 2: one pair.  Every scale: 1, 1e-4 (float16 subnormals), 3e4 (overflow to inf)."""
    eng = _engine(algo)
    try:
        if lanes is not None:
            eng.set_tuning("queue_lanes", lanes)
        for N in (11, 4, 2):
            for k, scale in enumerate(SCALES):
                _check_payload_call(eng, studies[algo][:N], scale, pad_last=bool((N + k) & 1), preconditions=N == 11)
        if lanes is None:
            assert eng.counter("queue_units_done") > 0                                      # the lanes really took the larger calls
        f16, e16 = eng.calc_study_payload(studies[algo][:4], echo=False)
        assert e16 is None and f16.shape == (4,) + studies[algo].shape[1:3] + (2,)          # pad_last is the default
    finally:
        eng.close()


def test_an_aborted_coresident_sub_batch_is_repeated_into_the_same_float16_half():
    """DeepFlow, the handle alone (queue_lanes = 0), co-resident SOR with block 0 muted: the first sub-batch's launch gives up, the
    sub-batch is solved again (tiled) into the staging half it had, and its copy-out is made again."""
    rgb = _study(33, 7, 97, 131)                                                            # 128 x 32 regions: 4 x 2 of them, 6 pairs = 4 + 2
    eng = _engine("deepflow")
    try:
        eng.set_tuning("queue_lanes", 0)
        eng.set_tuning("sor_coop", 3)
        eng.set_tuning("coop_test_mute", 1)
        f16, _ = eng.calc_study_payload(rgb, scale=0.5, pad_last=False, echo=False)
        assert eng.counter("coop_aborts") == 1                                              # precondition: the repeat happened in the float16 call
        eng.set_tuning("coop_test_mute", 0)
        exp = _half(eng.calc_study(rgb, scale=0.5, pad_last=False))
        assert np.array_equal(_bits(f16), _bits(exp))
    finally:
        eng.close()


def test_float16_flows_on_the_cuda_class_variant(studies):
    eng = _engine("TVL1", variant="cuda")
    try:
        _check_payload_call(eng, studies["TVL1"], 2.0, pad_last=True)
    finally:
        eng.close()


def test_two_payload_jobs_in_flight_collected_in_reverse_order(studies):
    from tee_optical_flow_amd.frames import rgb2gray
    eng = _engine("TVL1")
    try:
        a, b = studies["TVL1"], np.ascontiguousarray(studies["TVL1"][::-1][:6])
        ref = {}
        for name, rgb, scale in (("a", a, 2.0), ("b", b, 1e-4)):
            ref[name] = (_half(eng.calc_study(rgb, scale=scale, pad_last=True)), eng.last_iters().copy())
        ta = eng.submit_study_payload(a, scale=2.0, pad_last=True)
        tb = eng.submit_study_payload(b, scale=1e-4, pad_last=True, echo=True)
        fb, eb = eng.wait(tb)
        itb = eng.last_iters().copy()
        fa, ea = eng.wait(ta)
        assert np.array_equal(_bits(fa), _bits(ref["a"][0])) and np.array_equal(eng.last_iters(), ref["a"][1])
        assert np.array_equal(_bits(fb), _bits(ref["b"][0])) and np.array_equal(itb, ref["b"][1])
        assert np.array_equal(_bits(ea), _bits(rgb2gray(a).astype(np.float16))) and np.array_equal(_bits(eb), _bits(rgb2gray(b).astype(np.float16)))
    finally:
        eng.close()


@pytest.mark.parametrize("map_dtype", ["f32", "u8"])
def test_saliency_payload_for_both_map_types(map_dtype):
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.frames import rgb2gray
    rng = np.random.default_rng(8)
    rgb = _study(34, 6, 41, 67)
    rgb[..., 1] = np.roll(rgb[..., 1], 2, axis=2)
    rgb[..., 2] = rng.integers(0, 256, rgb.shape[:3], dtype=np.uint8)                       # R != G != B: the echo is not the gray diagonal's
    eng = _engine("TVL1")
    try:
        ref = eng.calc_study_saliency(rgb, scale=2.0, pad_last=True, map_dtype=map_dtype)
        it = eng.last_iters().copy()
        f16, e16 = eng.calc_study_saliency_payload(rgb, scale=2.0, pad_last=True, map_dtype=map_dtype)
        assert np.array_equal(_bits(f16), _bits(_half(ref))) and np.array_equal(eng.last_iters(), it)
        assert np.array_equal(_bits(e16), _bits(rgb2gray(rgb).astype(np.float16)))
        # the echo needs RGB frames
        g1 = np.ascontiguousarray(rgb[..., :1])
        out, e = np.empty((5, 41, 67, 2), np.float16), np.empty((6, 41, 67), np.float16)
        rc = eng._L.tf_calc_seq_saliency_f16(eng._h, g1.ctypes.data, 6, 41, 67, 1, 1, C.c_float(1.0), out.ctypes.data, e.ctypes.data, None)
        assert rc == _lib.TF_ERR_INVALID_ARG
    finally:
        eng.close()


@pytest.mark.parametrize("algo", ["TVL1", "deepflow"])
def test_pageable_destination_takes_the_in_order_copy(studies, algo):
    """The raw C call with plain numpy destinations (pageable memory): the in-order copy-out path, 3 sub-batches through one staging buffer."""
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.frames import rgb2gray
    rgb = studies[algo]
    N, H, W, _ = rgb.shape
    eng = _engine(algo)
    try:
        exp = _half(eng.calc_study(rgb, scale=2.0))
        exp_echo = _bits(rgb2gray(rgb).astype(np.float16))
        for lanes in (0, None):
            if lanes is not None:
                eng.set_tuning("queue_lanes", lanes)
            out = np.full((N - 1, H, W, 2), 0x7E00, np.uint16)                              # NaN bits: nothing may stay unwritten
            echo = np.full((N, H, W), 0x7E00, np.uint16)
            st = _lib.TfStats()
            _lib.check(eng._L.tf_calc_seq_rgb_f16(eng._h, rgb.ctypes.data, N, H, W, C.c_float(2.0), out.ctypes.data, echo.ctypes.data, C.byref(st)),
                       eng._h, "tf_calc_seq_rgb_f16")
            assert st.n_pairs == N - 1 and np.array_equal(out, _bits(exp))
            assert np.array_equal(echo, exp_echo)
            eng.set_tuning("queue_lanes", -1)
    finally:
        eng.close()


# ---- 4. files ---------------------------------------------------------------------------------------------------------------------
SCRIPT = r"""
import sys, json, os, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tests.payload_cases import same_file
from tee_optical_flow_amd import dense_flow
from tee_optical_flow_amd.pipeline import process_folder
from tee_optical_flow_amd.synth import speckle_sequence

calls = {}
def count(name):
    real = getattr(dense_flow.DenseFlow, name)
    def wrapped(self, *a, **k):
        calls[name] = calls.get(name, 0) + 1
        return real(self, *a, **k)
    setattr(dense_flow.DenseFlow, name, wrapped)
for name in ("calc_study", "submit_study", "calc_study_payload", "submit_study_payload"):
    count(name)

if __name__ == "__main__":
    workers, in_flight = sys.argv[1], int(sys.argv[2])
    src = os.path.join(TMP, "in")
    os.makedirs(src)
    for k in range(3):
        g = speckle_sequence(200 + k, 6, 128, 160)
        np.savez(os.path.join(src, f"st{k}.npz"), nparr=np.repeat(g[..., None], 3, axis=3), pixel_spacing=0.04, frame_rate=50.0, patient_id=f"SYN{k}", heart_rate=60)
    kw = dict(nchunks=1, chunk_index=0, mode="otsu", verbose=False, extensions=("npz",), OF_algo="TVL1", workers=workers, n_readers=2, n_writers=2,
              studies_in_flight=in_flight)
    out = {}
    for payload in ("host", "device"):
        calls.clear()
        out["errors_" + payload] = process_folder(src, os.path.join(TMP, payload), None, payload=payload, **kw)
        out["calls_" + payload] = dict(calls)
    names = sorted(os.listdir(os.path.join(TMP, "host")))
    out["files"] = names
    out["same"] = names == sorted(os.listdir(os.path.join(TMP, "device"))) and \
        all(same_file(os.path.join(TMP, "host", n), os.path.join(TMP, "device", n)) for n in names)
    with h5py.File(os.path.join(TMP, "device", "st0.hdf5"), "r") as f:
        out["moving"] = bool((np.abs(f["flow"][...].astype(np.float32)).reshape(6, -1).max(axis=1) > 0.5).all())
    print(json.dumps(out, default=str))
"""


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("workers", ["process", "thread"])
def test_process_folder_device_payload_writes_the_host_payloads_files(tmp_path, workers, in_flight):
    """A 3-study folder, Otsu masks, 6 frames of 128 x 160 (as test_gpu_study.py builds it), on the real engine: payload="device" against
    payload="host", the files byte for byte (all but HDF5's own time stamps: tests/payload_cases.py)."""
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    env = {**os.environ, "PYTHONDONTWRITEBYTECODE": "1"}
    sys_stdcpp = "/usr/lib/x86_64-linux-gnu/libstdc++.so.6"       # conda ships an older libstdc++ than libamdhip64 needs
    if os.path.exists(sys_stdcpp):                                # (in front of whatever the environment preloads already)
        env["LD_PRELOAD"] = ":".join([sys_stdcpp] + ([env["LD_PRELOAD"]] if env.get("LD_PRELOAD") else []))
    script = tmp_path / "walk.py"
    script.write_text(SCRIPT.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp_path))))
    r = subprocess.run([PY_H5, str(script), workers, str(in_flight)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    g = json.loads(r.stdout.strip().splitlines()[-1])
    assert g["errors_host"] == [] and g["errors_device"] == []
    assert g["files"] == ["st0.hdf5", "st1.hdf5", "st2.hdf5"] and g["same"] and g["moving"]
    f32_call, f16_call = ("submit_study", "submit_study_payload") if in_flight > 1 else ("calc_study", "calc_study_payload")
    assert g["calls_host"] == {f32_call: 3} and g["calls_device"] == {f16_call: 3}
