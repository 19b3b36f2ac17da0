"""A study held from the gzip chunks of its file (tf_hold_study_chunks, tf_hold_mask_chunks; DenseFlow.hold_study_chunks &
hold_mask_chunks; HeldStudy.from_chunks / from_hdf5(inflate="device")): the device inflates and assembles the chunks, and every held
tail call must then give the bits it gives after hold_study / hold_mask of the same arrays -- the comparisons of
tests/test_gpu_held_study.py (its _tail and _same_tail, imported: one statement of what "the whole tail" is), np.array_equal and no
tolerance.  The records are made here with zlib level 9 in the chunk shapes of the issue: (2,16,16,1) on 37 x 53 frames, where every
dimension has an edge chunk, and one chunk per frame stack on 64 x 64; one chunk is stored unfiltered and one is not stored at all."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests.inflate_cases import PY_H5, ROOT, chunked as _record
from tests.test_gpu_held_study import _masks, _same, _same_tail, _tail

pytestmark = pytest.mark.gpu

STUDIES = [((5, 37, 53), (2, 16, 16)), ((9, 64, 64), (9, 64, 64))]


@pytest.fixture(scope="module")
def eng():
    e = T.DenseFlow(device_id=0, max_batch=3)
    yield e
    e.close()


def _study(shape, chunk, Cm, special=True):
    """arrays and records of one study: ({'flow', 'echo', 'rv', 'av'} as the records say they are, {name: record})"""
    N, H, W = shape
    rng = np.random.default_rng(N * H * W + Cm)
    amp = np.concatenate([[0.5], rng.uniform(1, 6, N - 1)])[:, None, None, None]
    arrays = {"flow": (np.cumsum(rng.normal(0, 0.3, (N, H, W, 2)), axis=2) * amp).astype(np.float16),
              "echo": rng.integers(1, 256, (N, H, W)).astype(np.float16), **_masks(N, H, W, Cm)}
    recs, want = {}, {}
    for k, a in arrays.items():
        ch = chunk if a.ndim == 3 else chunk + (1,)
        n = int(np.prod([-(-s // c) for s, c in zip(a.shape, ch)]))
        recs[k], want[k] = _record(a, ch, unfiltered={1 % n} if special else (), missing={n - 1} if special and n > 2 else ())
    return want, recs


def _hold_arrays(e, a):
    e.hold_study(a["flow"], a["echo"])
    for k in ("rv", "av"):
        e.hold_mask(k, a[k])


def _hold_chunks(e, r):
    e.hold_study_chunks(r["flow"], r["echo"])
    for k in ("rv", "av"):
        e.hold_mask_chunks(k, r[k])


@pytest.mark.parametrize("Cm", [1, 2])
@pytest.mark.parametrize("shape,chunk", STUDIES, ids=["37x53", "64x64"])
def test_every_held_call_after_the_chunks_equals_the_call_after_the_arrays(eng, shape, chunk, Cm):
    arrays, recs = _study(shape, chunk, Cm)
    N = shape[0]
    assert any(int(m) & 1 for m in recs["flow"]["filter_mask"])                         # the unfiltered chunk
    if chunk == (2, 16, 16):                                                            # ... and, where there are more than two, the missing one
        assert len(recs["flow"]["len"]) == 3 * 3 * 4 * 2 - 1 and not arrays["flow"][-1, -1, -1, 1].any()
    _hold_arrays(eng, arrays)
    ref = {(n, g): _tail(eng, n, g, True) for n in (N - 2, N) for g in (False, True)}
    g0 = eng.held.generation
    c0 = eng.counter("tail_upload_bytes")
    _hold_chunks(eng, recs)
    assert eng.counter("tail_upload_bytes") - c0 == sum(int(r["blob"].size) for r in recs.values())
    h = eng.held
    assert (h.N, h.H, h.W, h.n_echo) == shape + (N,) and h.generation > g0 and h.masks == {"rv": (N, Cm), "av": (N, Cm)}
    for key, want in ref.items():
        _same_tail(_tail(eng, key[0], key[1], True), want, f"{shape} C={Cm} n={key[0]} grad_f64={key[1]}")
    # ... and against the originals on the host arrays, which the reference fixtures pin
    _same_tail(_tail(eng, N - 2, True, True), _tail(eng, N - 2, True, False, arrays["flow"], arrays, arrays["echo"]), "against the originals")
    # without an echo; a mask held again replaces its slot
    eng.hold_study_chunks(recs["flow"])
    assert eng.held.n_echo == 0 and eng.held.masks == {}
    eng.hold_mask_chunks("rv", recs["rv"])
    eng.hold_mask_chunks("rv", recs["av"])
    eng.hold_mask("av", arrays["av"])
    _same(eng.held_first_region_areas("rv", N), eng.held_first_region_areas("av", N), "a replaced slot")


def test_a_corrupted_chunk_raises_and_changes_nothing(eng):
    shape, chunk = STUDIES[0]
    arrays, recs = _study(shape, chunk, 2)
    _hold_chunks(eng, recs)
    N = shape[0]
    ref = _tail(eng, N - 2, True, True)
    gen, masks = eng.held.generation, eng.held.masks
    other, orecs = _study((6, 37, 53), chunk, 2, special=False)
    for name in ("flow", "echo"):
        bad = {k: dict(v) for k, v in orecs.items()}
        blob = bad[name]["blob"].copy()
        blob[int(bad[name]["off"][7]) + int(bad[name]["len"][7]) // 2] ^= 0x10
        bad[name]["blob"] = blob
        with pytest.raises(OpticalFlowCalculationError, match=f"{name} chunk 7 did not inflate") as ei:
            eng.hold_study_chunks(bad["flow"], bad["echo"])
        assert ei.value.code == _lib.TF_ERR_INVALID_ARG
        assert eng.held.generation == gen and eng.held.masks == masks and eng.held.N == N
    bad = dict(recs["rv"], blob=recs["rv"]["blob"].copy())
    bad["blob"][int(bad["off"][2]) + 3] ^= 0xFF
    for label in ("rv", "fresh"):
        with pytest.raises(OpticalFlowCalculationError, match="mask chunk 2 did not inflate"):
            eng.hold_mask_chunks(label, bad)
    trunc = dict(recs["rv"], len=recs["rv"]["len"].copy())
    trunc["len"][0] -= 1
    with pytest.raises(OpticalFlowCalculationError, match=r"mask chunk 0 did not inflate: status 6 \(input truncated\)"):
        eng.hold_mask_chunks("rv", trunc)
    assert eng.held.generation == gen and eng.held.masks == masks
    _same_tail(_tail(eng, N - 2, True, True), ref, "after the failed calls")


def test_refusals_come_before_any_gpu_work(eng):
    shape, chunk = STUDIES[0]
    arrays, recs = _study(shape, chunk, 1)
    _hold_chunks(eng, recs)
    L, h = eng._L, eng._h
    gen = eng.held.generation
    c0 = [eng.counter(k) for k in ("tail_upload_bytes", "inflate_kernel_us", "unchunk_kernel_us")]
    flow, keep = T.DenseFlow._chunked(recs["flow"], "flow", 4, (np.float16,))
    echo, keep2 = T.DenseFlow._chunked(recs["echo"], "echo", 3, (np.float16,))
    mask, keep3 = T.DenseFlow._chunked(recs["rv"], "mask", 4, (np.bool_,))

    def study(f=flow, e=echo, shape=None, chunk=None, **kw):
        f2 = None if f is None else _lib.TfChunked.from_buffer_copy(f)
        for k, v in kw.items():
            setattr(f2, k, v)
        if shape:
            f2.shape[shape[0]] = shape[1]
        if chunk:
            f2.chunk[chunk[0]] = chunk[1]
        return L.tf_hold_study_chunks(h, None if f2 is None else C.byref(f2), None if e is None else C.byref(e))

    far = keep[4].copy()
    far[1, 1] = 37                               # a chunk that starts outside the array
    neg = keep[4].copy()
    neg[0, 0] = -2
    for bad, text in ((dict(f=None), "null flow"), (dict(n=-1), "n = -1"), (dict(blob=None), "null blob"), (dict(off=None), "null blob"),
                      (dict(len=None), "null blob"), (dict(coord=None), "null coord"), (dict(ndim=3), "dimensions"), (dict(elem_bytes=4), "byte elements"),
                      (dict(chunk_bytes=1023), "chunk_bytes 1023"), (dict(shape=(3, 3)), "last dimension"), (dict(shape=(0, 0)), "dimension 0"),
                      (dict(chunk=(1, 0)), "dimension 1"), (dict(chunk=(2, 17)), "chunk_bytes"), (dict(coord=far.ctypes.data), "outside [0, 37)"),
                      (dict(coord=neg.ctypes.data), "outside [0, 5)"), (dict(e=flow), "echo has 4 dimensions"), (dict(e=mask), "echo has 4 dimensions")):
        assert study(**bad) == _lib.TF_ERR_INVALID_ARG, bad
        assert text in L.tf_last_error(h).decode(), (bad, L.tf_last_error(h))
    e2 = _lib.TfChunked.from_buffer_copy(echo)
    e2.shape[2] = 54                             # echo frames of another size than the flow's
    assert L.tf_hold_study_chunks(h, C.byref(flow), C.byref(e2)) == _lib.TF_ERR_INVALID_ARG and b"echo frames are" in L.tf_last_error(h)
    for slot, m, text in ((-1, mask, "out of range"), (12, mask, "out of range"), (0, None, "null mask"), (0, flow, "2-byte elements"), (0, echo, "3 dimensions")):
        assert L.tf_hold_mask_chunks(h, slot, None if m is None else C.byref(m)) == _lib.TF_ERR_INVALID_ARG
        assert text in L.tf_last_error(h).decode(), (slot, L.tf_last_error(h))
    m2 = _lib.TfChunked.from_buffer_copy(mask)
    m2.shape[1] = 38
    assert L.tf_hold_mask_chunks(h, 0, C.byref(m2)) == _lib.TF_ERR_INVALID_ARG and b"the held study's frames" in L.tf_last_error(h)
    assert eng.held.generation == gen and [eng.counter(k) for k in ("tail_upload_bytes", "inflate_kernel_us", "unchunk_kernel_us")] == c0
    with pytest.raises(OpticalFlowCalculationError, match="float16"):
        eng.hold_study_chunks(recs["rv"])
    with pytest.raises(OpticalFlowCalculationError, match="the held study's frames"):
        eng.hold_mask_chunks("rv", _study((5, 36, 53), chunk, 1)[1]["rv"])
    eng.release_study()
    assert L.tf_hold_mask_chunks(h, 0, C.byref(mask)) == _lib.TF_ERR_INVALID_ARG and b"no study is held" in L.tf_last_error(h)
    with pytest.raises(OpticalFlowCalculationError, match="no study is held"):
        eng.hold_mask_chunks("rv", recs["rv"])
    del keep2, keep3


def _analysis(ds, e):
    out = [("av_centroids", np.asarray(A.av_centroids(ds.get_mask("av"), ds.nframes, engine=e)))]
    for param in A.PARAMS:
        st = A.calculate_3dhist_radlong(ds, param, nbins=60, engine=e)
        out += [(f"radlong/{param}/{k}", st[k]) for k in sorted(st)]
        out.append((f"3dhist/{param}", A.calculate_3dhist(ds, param, "rv", nbins=60, engine=e)))
        out.append((f"overlay/{param}", A.radlong_overlay(ds, param, engine=e, return_info=True)))
    out.append(("angle_mode", A.angle_mode_series(ds, "velocity", "rv", engine=e)))
    out.append(("area/rv", A.area_series(ds, "rv", engine=e)))
    return out


def test_from_chunks_gives_the_analysis_of_from_study(eng):
    shape, chunk = (14, 37, 53), (2, 16, 16)
    arrays, recs = _study(shape, chunk, 2, special=False)
    rec = {"filename": "held", "attrs": {"frame_rate": 50.0, "units_converted": True, "nframes": 14, "mode": "RVIO_2class", "labels": ["rv", "av"]},
           "datasets": recs}
    st = A.FlowStudy(arrays["flow"], {k: arrays[k] for k in ("rv", "av")}, 50.0, nframes=12, echo=arrays["echo"], filename="held")
    ref = _analysis(A.HeldStudy.from_study(eng, st), eng)
    for way in ("host", "device"):
        hs = A.HeldStudy.from_chunks(eng, rec, inflate=way)
        assert hs.nframes == 12 and hs.accepted_labels == ["rv", "av"] and hs.filename == "held"
        _same_tail(_analysis(hs, eng), ref, f"from_chunks inflate={way}")


H5_DRIVER = r"""
import sys, os, numpy as np
sys.path.insert(0, ROOT)
import h5py
from tee_optical_flow_amd import analysis as A
from tee_optical_flow_amd.hdf5_out import save_optical_flow_to_hdf5
from tee_optical_flow_amd.config import default_optical_flow_config
rng = np.random.default_rng(12)
N, H, W = 12, 150, 170
yy, xx = np.mgrid[:H, :W]
flow = np.cumsum(rng.normal(0, 0.1, (N, H, W, 2)), axis=2).astype(np.float32)
nparr = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
disc = np.stack([((yy - 70 - f) ** 2 + (xx - 80) ** 2 < 900 + 20 * f) for f in range(N)])
masks = {"rv": np.repeat(disc[..., None], 2, axis=3), "av": np.repeat((disc & (yy < 75))[..., None], 2, axis=3)}
meta = {"frame_rate": 40.0, "pixel_spacing": 0.05, "R_wave_data_present": False, "R_times": None}
path = os.path.join(TMP, "study.hdf5")
save_optical_flow_to_hdf5(path, flow, nparr, masks, meta, {}, "P", 60, default_optical_flow_config(), "RVIO_2class", False, False)
A.save_chunks(A.study_chunks(path), os.path.join(TMP, "chunks.npz"))
with h5py.File(path, "r") as f:
    np.savez(os.path.join(TMP, "arrays.npz"), **{k: f[k][()] for k in ("flow", "echo", "rv", "av")})
print("written")
"""


def test_a_real_study_file_read_by_another_interpreter(eng, tmp_path):
    if not os.path.exists(PY_H5):
        pytest.skip("no interpreter with h5py")
    script = H5_DRIVER.replace("ROOT", repr(ROOT)).replace("TMP", repr(str(tmp_path)))
    r = subprocess.run([PY_H5, "-c", script], capture_output=True, text=True, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    rec = A.load_chunks(str(tmp_path / "chunks.npz"))
    z = np.load(str(tmp_path / "arrays.npz"))
    assert rec["attrs"]["labels"] == ["rv", "av"] and len(rec["datasets"]["flow"]["len"]) > 1
    st = A.FlowStudy(z["flow"], {k: z[k] for k in ("rv", "av")}, 40.0, nframes=10, echo=z["echo"], filename=rec["filename"])
    ref = _analysis(A.HeldStudy.from_study(eng, st), eng)
    c0 = eng.counter("tail_upload_bytes")
    hs = A.HeldStudy.from_chunks(eng, rec, inflate="device")
    assert eng.counter("tail_upload_bytes") - c0 == sum(int(d["blob"].size) for k, d in rec["datasets"].items())
    assert hs.nframes == 10 and hs.frame_rate == 40.0
    _same_tail(_analysis(hs, eng), ref, "a written file, inflate=device")
