"""DualTVL1 with useInitialFlow on the device (include/teeflow.h, tf_calc_pairs_init / tf_calc_pairs_init_device): a solve started
from the caller's flow is bit-equal to the oracle's stages composed on the CPU (tests/tvl1_init_cases.composed) and meets the project's
criterion against the float64 solve; a zero seed is the plain solve; batches on the lanes, in place, device pointers, float32 frames,
an off-image seed, what one solve leaves behind for the next, and the refusals.  Each test prints its figures before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tvl1_init_cases as IC
from tests import tvl1_ref64_cases as K
from tests.tvl1_forms import iter_form

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_engine(**over):
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(**over)
    eng.setUseInitialFlow(True)
    assert eng.getUseInitialFlow() is True
    return eng


def run_case(oracle, cid, form):
    over, _, seeds, _ = IC.CASES[cid]
    I0s, I1s, inits = IC.case_inputs(cid)
    eng = seeded_engine(**over)
    try:
        with iter_form(eng, form):
            for b, seed in enumerate(seeds):
                keep = inits[b].copy()
                flow = eng.calc(I0s[b], I1s[b], inits[b])
                iters, levels = eng.last_iters()[0], eng.last_stats["nscales_used"]
                assert np.array_equal(inits[b], keep) and flow is not inits[b]
                cf, cit, cl = IC.composed_case(oracle, cid, b)
                sid = f"{cid}/seed{seed}/{form}"
                print(sid, "values that differ from composed:", int(np.sum(flow != cf)))
                assert levels == cl and np.array_equal(iters, cit), f"{sid}: {iters.tolist()}\n{cit.tolist()}"
                assert np.array_equal(flow, cf), f"{sid}: {np.sum(flow != cf)} values differ from composed, max {np.abs(flow - cf).max()}"
                missed = IC.criterion(sid, flow, iters, levels, IC.ref_case(cid, b))
                assert not missed, f"{sid}: {missed}"
    finally:
        eng.close()


@pytest.mark.parametrize("cid", list(IC.CASES))
def test_seeded_solve_is_composed_and_meets_the_criterion(oracle, cid):
    run_case(oracle, cid, "strips2")


@pytest.mark.parametrize("cid", IC.TILES_TOO)
def test_seeded_solve_on_tiles(oracle, cid):
    run_case(oracle, cid, "tiles")


@pytest.mark.parametrize("cid", ["short-3x2", "odd-37x53"])
def test_zero_seed_is_the_plain_solve(cid):
    import tee_optical_flow_amd as T
    I0s, I1s, inits = IC.case_inputs(cid)
    eng = T.DenseFlow(**IC.CASES[cid][0])
    try:
        plain = np.array(eng.calc(I0s[0], I1s[0], None))
        plain_it = eng.last_iters()
        eng.setUseInitialFlow(True)
        zero = eng.calc(I0s[0], I1s[0], np.zeros_like(inits[0]))
        assert np.array_equal(zero, plain) and np.array_equal(eng.last_iters(), plain_it)
        seeded = eng.calc(I0s[0], I1s[0], inits[0])
        assert not np.array_equal(seeded, plain), "the seed was not read"
    finally:
        eng.close()


def _batch():
    """five odd-37x53 pairs (seeds 3..7), each with an initial flow of its own"""
    from tee_optical_flow_amd.synth import speckle_pairs
    over, (H, W), _, amp = IC.CASES["odd-37x53"]
    seeds = [3, 4, 5, 6, 7]
    I0s, I1s = speckle_pairs(seeds, H, W)
    return over, np.ascontiguousarray(I0s), np.ascontiguousarray(I1s), np.stack([IC.initial_flow(s, H, W, amp) for s in seeds])


def test_batch_in_sub_batches_on_the_lanes_and_in_place(oracle):
    """max_batch = 2: three sub-batches taken by the lanes, every pair with its own slice of `init`; then the same call with init and
    flow_out the same host array, as cv2's in/out `flow`"""
    from tee_optical_flow_amd import _lib
    over, I0s, I1s, inits = _batch()
    B, H, W = I0s.shape
    eng = seeded_engine(max_batch=2, **over)
    try:
        keep = inits.copy()
        flows = np.array(eng.calc_pairs(I0s, I1s, init=inits))
        iters = eng.last_iters()
        assert eng.counter("queue_units_done") == 3, "the call did not go through the lane queue"
        assert np.array_equal(inits, keep)
        for b in range(B):
            one = eng.calc(I0s[b], I1s[b], inits[b])
            assert np.array_equal(flows[b], one) and np.array_equal(iters[b], eng.last_iters()[0]), f"pair {b}"
        cf, cit, _ = IC.composed(oracle, I0s[4], I1s[4], K.params(**over), inits[4])     # the last pair: a sub-batch of one, offset 4
        assert np.array_equal(flows[4], cf) and np.array_equal(iters[4], cit)
        buf = inits.copy()
        st = _lib.TfStats()
        _lib.check(eng._L.tf_calc_pairs_init(eng._h, I0s.ctypes.data, I1s.ctypes.data, 0, buf.ctypes.data, B, H, W, buf.ctypes.data, C.byref(st)),
                   eng._h, "tf_calc_pairs_init")
        assert np.array_equal(buf, flows), "in place differs from out of place"
    finally:
        eng.close()


DEVICE_FORM = r"""
import sys
import numpy as np, torch
sys.path.insert(0, ROOT)
import tee_optical_flow_amd as T
from tests.test_gpu_tvl1_init import _batch
over, I0s, I1s, inits = _batch()
B, H, W = I0s.shape
dev = torch.device("cuda", 0)
fr = torch.from_numpy(np.concatenate([I0s, I1s])).to(dev)
p0, p1 = fr.data_ptr(), fr.data_ptr() + B * H * W
dinit = torch.from_numpy(inits).to(dev)
out = torch.zeros((B, H, W, 2), dtype=torch.float32, device=dev)
torch.cuda.synchronize()
for mb in (2, 128):                                   # three sub-batches on the lanes; one sub-batch on the handle
    eng = T.DenseFlow(device_id=0, max_batch=mb, **over)
    try:
        eng.setUseInitialFlow(True)
        host = np.array(eng.calc_pairs(I0s, I1s, init=inits))
        host_it = eng.last_iters()
        eng.calc_pairs_device(p0, p1, B, H, W, out.data_ptr(), dinit_ptr=dinit.data_ptr())
        assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(eng.last_iters(), host_it), mb
        assert np.array_equal(dinit.cpu().numpy(), inits)
        eng.calc_pairs_device(p0, p1, B, H, W, out.data_ptr(), scale=2.0, dinit_ptr=dinit.data_ptr())     # the seed is not scaled
        assert np.array_equal(out.cpu().numpy(), host * np.float32(2)), mb
        io = dinit.clone()
        torch.cuda.synchronize()
        eng.calc_pairs_device(p0, p1, B, H, W, io.data_ptr(), dinit_ptr=io.data_ptr())
        assert np.array_equal(io.cpu().numpy(), host), f"in place, max_batch {mb}"
        try:
            eng.calc_pairs_device(p0, p1, B, H, W, out.data_ptr())
            raise SystemExit("no refusal without dinit_ptr")
        except T.OpticalFlowCalculationError as e:
            assert e.code == 2 and "tf_calc_pairs_init" in str(e), e
        eng.setUseInitialFlow(False)                  # flag off: the initial flow is not looked at
        plain = np.array(eng.calc_pairs(I0s, I1s))
        eng.calc_pairs_device(p0, p1, B, H, W, out.data_ptr(), dinit_ptr=dinit.data_ptr())
        assert np.array_equal(out.cpu().numpy(), plain) and not np.array_equal(plain, host)
    finally:
        eng.close()
print("device form ok")
"""


def test_device_pointer_form_equals_host_form():
    """tf_calc_pairs_init_device on torch tensors (a child process with torch imported first: the engine and torch must share one HIP
    runtime): equal to the host form, the seed unscaled, in place, refused without a seed, ignored with the flag off"""
    r = subprocess.run([sys.executable, "-c", DEVICE_FORM.replace("ROOT", repr(ROOT))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device form ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_float32_frames(oracle):
    over, _, seeds, _ = IC.CASES["one"]
    I0s, I1s, inits = IC.case_inputs("one")
    F0, F1 = IC.f32_frames(I0s, I1s, seeds[0])
    eng = seeded_engine(**over)
    try:
        for b in range(len(seeds)):
            flow = eng.calc(F0[b], F1[b], inits[b])
            cf, cit, cl = IC.composed(oracle, F0[b], F1[b], K.params(**over), inits[b])
            assert eng.last_stats["nscales_used"] == cl and np.array_equal(eng.last_iters()[0], cit)
            assert np.array_equal(flow, cf), f"pair {b}: {np.sum(flow != cf)} values differ"
            assert not np.array_equal(flow, IC.composed_case(oracle, "one", b)[0]), "the float frames equal the uint8 ones"
    finally:
        eng.close()


def test_seed_far_outside_the_image(oracle):
    """amp 500 on 72x88: the warp's integer part leaves the image (and the LDS tile) almost everywhere; composed only, the float64
    solve is not asked"""
    over, (H, W), seeds, _ = IC.CASES["one"]
    I0s, I1s, _ = IC.case_inputs("one")
    eng = seeded_engine(**over)
    try:
        for b, seed in enumerate(seeds):
            init = IC.initial_flow(seed, H, W, 500.0)
            flow = eng.calc(I0s[b], I1s[b], init)
            cf, cit, _ = IC.composed(oracle, I0s[b], I1s[b], K.params(**over), init)
            assert np.isfinite(flow).all()
            assert np.array_equal(eng.last_iters()[0], cit) and np.array_equal(flow, cf), f"pair {b}: {np.sum(flow != cf)} values differ"
    finally:
        eng.close()


def test_nothing_of_one_solve_leaks_into_the_next():
    """a 97x131 seeded solve, then on the same handle 37x53 from zero and 37x53 seeded: what fresh handles give (the 97x131 chain has
    written both u buffers over the smaller geometry's planes and padding)"""
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_pairs
    over = IC.CASES["odd-37x53"][0]
    big0, big1 = speckle_pairs([0], 97, 131)
    I0s, I1s, inits = IC.case_inputs("odd-37x53")
    used = seeded_engine(**over)
    try:
        used.calc(big0[0], big1[0], IC.initial_flow(0, 97, 131, 6.0))
        used.setUseInitialFlow(False)
        zero = np.array(used.calc(I0s[0], I1s[0], None))
        used.setUseInitialFlow(True)
        seeded = np.array(used.calc(I0s[0], I1s[0], inits[0]))
    finally:
        used.close()
    fresh = T.DenseFlow(**over)
    try:
        assert np.array_equal(zero, fresh.calc(I0s[0], I1s[0], None)), "zero start after a seeded solve"
    finally:
        fresh.close()
    fresh = seeded_engine(**over)
    try:
        assert np.array_equal(seeded, fresh.calc(I0s[0], I1s[0], inits[0])), "seeded solve after other solves"
    finally:
        fresh.close()


def test_refusals_and_state(oracle):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import _lib
    Err = T.OpticalFlowCalculationError
    I0s, I1s, inits = IC.case_inputs("one")
    H, W = I0s.shape[1:]
    eng = T.DenseFlow()
    try:
        assert eng.getUseInitialFlow() is False
        eng.setUseInitialFlow(True)
        with pytest.raises(Err, match="got None"):
            eng.calc(I0s[0], I1s[0], None)
        for bad in (inits[0][:, :, :1], inits[0][:-1], inits[0][None], np.zeros((W, H, 2), np.float32), "flow"):
            with pytest.raises(Err):
                eng.calc(I0s[0], I1s[0], bad)
        with pytest.raises(Err):
            eng.calc_pairs(I0s, I1s, init=inits[:1])
        assert np.array_equal(eng.calc(I0s[0], I1s[0], inits[0].astype(np.float64)), eng.calc(I0s[0], I1s[0], inits[0]))
        jobs = eng.counter("queue_jobs")
        rgb = np.repeat(I0s[..., None], 3, -1)
        for name, call in (("calc_batch", lambda: eng.calc_batch(I0s)), ("submit_pairs", lambda: eng.submit_pairs(I0s, I1s)),
                           ("calc_study", lambda: eng.calc_study(rgb)), ("calc_pairs", lambda: eng.calc_pairs(I0s, I1s)),
                           ("submit_batch", lambda: eng.submit_batch(I0s)), ("calc_study_payload", lambda: eng.calc_study_payload(rgb)),
                           ("calc_study_saliency", lambda: eng.calc_study_saliency(rgb))):
            if name == "calc_pairs":                 # the Python layer refuses a missing `init` itself; the library, a NULL one
                with pytest.raises(Err, match="got None"):
                    call()
                st = _lib.TfStats()
                rc = eng._L.tf_calc_pairs(eng._h, I0s.ctypes.data, I1s.ctypes.data, 2, H, W, np.empty((2, H, W, 2), np.float32).ctypes.data, C.byref(st))
                assert rc == _lib.TF_ERR_UNSUPPORTED and b"tf_calc_pairs_init" in eng._L.tf_last_error(eng._h)
                rc = eng._L.tf_calc_pairs_init(eng._h, I0s.ctypes.data, I1s.ctypes.data, 0, None, 2, H, W, np.empty((2, H, W, 2), np.float32).ctypes.data,
                                               C.byref(st))
                assert rc == _lib.TF_ERR_UNSUPPORTED
                continue
            with pytest.raises(Err, match="tf_calc_pairs_init") as e:
                call()
            assert e.value.code == _lib.TF_ERR_UNSUPPORTED, name
        assert eng.counter("queue_jobs") == jobs and not eng._jobs, "a refused call was queued"
        eng.setUseInitialFlow(False)
        assert np.array_equal(eng.calc(I0s[0], I1s[0], inits[0]), oracle.tvl1_calc(I0s[0], I1s[0])), "flag off: the flow is ignored"
        assert np.array_equal(eng.calc_pairs(I0s, I1s, init="anything")[1], oracle.tvl1_calc(I0s[1], I1s[1]))
        with pytest.raises(Err) as e:
            eng.setGamma(0.5)
        assert e.value.code == _lib.TF_ERR_UNSUPPORTED
        assert eng._L.tf_abi_version() == 2
    finally:
        eng.close()
    cuda = T.DenseFlow(variant="cuda")
    try:
        with pytest.raises(Err, match="TF_VARIANT_CUDA") as e:
            cuda.setUseInitialFlow(True)
        assert e.value.code == _lib.TF_ERR_UNSUPPORTED and cuda.getUseInitialFlow() is False
    finally:
        cuda.close()
    with pytest.raises(Err, match="TF_VARIANT_CUDA"):
        T.DenseFlow(variant="cuda", use_initial_flow=1)
    deep = T.createOptFlow_DeepFlow()
    try:
        with pytest.raises(Err):
            deep.setUseInitialFlow(True)
    finally:
        deep.close()
