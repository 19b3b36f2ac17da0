"""DualTVL1's chained sequence on the device (include/teeflow.h, tf_chain_next; DenseFlow's chain=True): one call equals the video idiom
`flow = calc(frames[k], frames[k+1], flow)` on the same handle and the oracle's stages composed on the CPU
(tests/tvl1_chain_cases.composed_chain), bit for bit and iteration count for iteration count; across sub-batches as one queue unit; under
scale, float16, WASE and hold, always seeded by the unscaled float32 flow; submitted chains side by side; device pointers; what one chain
leaves behind for the next; and the refusals.  Each test prints its figures before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tvl1_chain_cases as CC
from tests.tvl1_forms import iter_form

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain_engine(**over):
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(**over)
    eng.setUseInitialFlow(True)
    return eng


def loop(eng, fr):
    """the idiom the call replaces -> (flows [N-1, H, W, 2], iters [N-1, levels, warps, 2])"""
    flows, iters, flow = [], [], np.zeros(fr.shape[1:] + (2,), np.float32)
    for k in range(len(fr) - 1):
        flow = np.array(eng.calc(fr[k], fr[k + 1], flow))
        flows.append(flow)
        iters.append(eng.last_iters()[0])
    return np.stack(flows), np.stack(iters)


# ---- 1. chain against loop and composition -------------------------------------------------------------------------------------------
def run_case(oracle, cid, form):
    import tee_optical_flow_amd as T
    over, fr = CC.overrides(cid), CC.frames(cid)
    cf, cit, cl = CC.chain_case(oracle, cid)
    eng = chain_engine(**over)
    try:
        with iter_form(eng, form):
            steps = eng.counter("chain_steps")
            got = np.array(eng.calc_batch(fr, chain=True))
            iters, levels = eng.last_iters(), eng.last_stats["nscales_used"]
            assert eng.counter("chain_steps") - steps == len(fr) - 1
            lf, lit = loop(eng, fr)
        for k in range(len(got)):
            print(f"{cid}/{form} pair {k}: values that differ from the loop {int(np.sum(got[k] != lf[k]))}, from composed "
                  f"{int(np.sum(got[k] != cf[k]))}; inner iterations {int(iters[k, ..., 0].sum())}, composed {int(cit[k, ..., 0].sum())}")
        assert levels == cl and np.array_equal(iters, lit) and np.array_equal(iters, cit), f"{iters.tolist()}\n{cit.tolist()}"
        assert np.array_equal(got, lf), "the chain differs from the loop of calc(I0, I1, flow)"
        assert np.array_equal(got, cf), "the chain differs from the composed chain"
    finally:
        eng.close()
    plain = T.DenseFlow(**over)
    try:
        with iter_form(plain, form):
            unchained = plain.calc_batch(fr)
        assert np.array_equal(got[0], unchained[0]), "pair 0 is not the plain solve"
        assert not np.array_equal(got[1], unchained[1]), "the seed was not read"
    finally:
        plain.close()


@pytest.mark.parametrize("cid", list(CC.CASES))
def test_chain_is_the_loop_and_the_composed_chain(oracle, cid):
    run_case(oracle, cid, "strips2")


@pytest.mark.parametrize("cid", CC.TILES_TOO)
def test_chain_on_tiles(oracle, cid):
    run_case(oracle, cid, "tiles")


@pytest.mark.parametrize("form", ["strips2", "tiles"])
@pytest.mark.parametrize("cid", ["one", "odd"])
def test_chain_moves_a_flow_that_ends_in_the_other_buffer(oracle, cid, form):
    """Which u buffer a finished pair's flow lies in is the parity of its launches and medians.  With the cases' parameters no stage
    stops early and every stage advances it by an even number (150 or 300 launches + 10 medians), so the flow always ends where the
    seed chain wants it and is kept.  28 inner x 1 outer iterations make every stage odd (14 or 28 launches + 1 median): over the one
    level of `one` and the five of `odd` the flow ends in buffer 1 and the chain wants it in buffer 0 -- it is moved, and with one
    level the row padding is cleared by the same kernel."""
    from tests import tvl1_ref64_cases as K
    over = dict(CC.overrides(cid), inner_iterations=28, outer_iterations=1)
    fr = CC.frames(cid)
    cf, cit, cl = CC.composed_chain(oracle, fr, K.params(**over))
    eng = chain_engine(**over)
    try:
        with iter_form(eng, form):
            got = np.array(eng.calc_batch(fr, chain=True))
            iters = eng.last_iters()
            lf, lit = loop(eng, fr)
        print(f"{cid}/{form}: values that differ from the loop {int(np.sum(got != lf))}, from composed {int(np.sum(got != cf))}; iterations {iters[0].tolist()}")
        assert (iters[..., 0] == 28).all() and (iters[..., 1] == 1).all(), "a stage stopped early: the parity argument does not hold"
        assert np.array_equal(iters, lit) and np.array_equal(iters, cit)
        assert np.array_equal(got, lf) and np.array_equal(got, cf)
        assert not np.array_equal(got[1], CC.composed_chain(oracle, fr[1:3], K.params(**over))[0][0]), "the seed was not read"
    finally:
        eng.close()


# ---- 2. sub-batches --------------------------------------------------------------------------------------------------------------------
def test_chain_carries_across_sub_batches_as_one_queue_unit():
    """max_batch = 2: five pairs are three sub-batches, solved in order by one engine; the seed crosses the next sub-batch's pyramid build"""
    from tee_optical_flow_amd.synth import speckle_sequence
    over = CC.overrides("odd")
    fr = np.ascontiguousarray(speckle_sequence(CC.SEED, 7, 37, 53)[:6])
    whole = chain_engine(**over)
    try:
        ref = np.array(whole.calc_batch(fr, chain=True))
        ref_it = whole.last_iters()
    finally:
        whole.close()
    eng = chain_engine(max_batch=2, **over)
    try:
        steps, units, jobs = eng.counter("chain_steps"), eng.counter("queue_units_done"), eng.counter("queue_jobs")
        got = eng.calc_batch(fr, chain=True)
        d = (eng.counter("chain_steps") - steps, eng.counter("queue_units_done") - units, eng.counter("queue_jobs") - jobs)
        print("chain_steps, queue units, queue jobs grew by", d, "; values that differ from one sub-batch:", int(np.sum(got != ref)))
        assert np.array_equal(got, ref) and np.array_equal(eng.last_iters(), ref_it)
        assert d == (5, 1, 1)
    finally:
        eng.close()


# ---- 3. scale, float16, WASE, hold -----------------------------------------------------------------------------------------------------
def test_scale_float16_wase_and_hold_are_seeded_by_the_float32_flow():
    over, gray = CC.overrides("odd"), CC.frames("odd")
    rgb = CC.rgb_of(gray)
    N, H, W = gray.shape
    bkgd = np.random.default_rng(H).random((2, H, W, 2)) < 0.3
    eng = chain_engine(max_batch=3, **over)                      # (four pairs: two sub-batches)
    try:
        cond = eng.condition_frames(rgb)
        chain = np.array(eng.calc_batch(cond, chain=True))       # the unscaled float32 chain of the conditioned frames
        eng.setUseInitialFlow(False)
        assert not np.array_equal(chain[1], eng.calc_batch(cond)[1])
        plain_echo = np.array(eng.calc_study_payload(rgb, scale=0.37)[1])
        eng.setUseInitialFlow(True)
        assert np.array_equal(eng.calc_study(rgb, chain=True), chain)
        assert np.array_equal(eng.calc_batch(cond, scale=2.0, chain=True), chain * np.float32(2)), "scale 2: the seed was scaled"
        flow16, echo16 = eng.calc_study_payload(rgb, scale=0.37, chain=True)
        want16 = (chain * np.float32(0.37)).astype(np.float16)
        print("float16 payload: values that differ", int(np.sum(flow16[:N - 1] != want16)))
        assert flow16.dtype == np.float16 and np.array_equal(flow16[:N - 1], want16) and np.array_equal(flow16[N - 1], want16[-1])
        assert np.array_equal(echo16, plain_echo)
        want_w, want_bg = eng.wase_compensate(chain, bkgd, scale=0.37)
        got_w, got_bg = eng.calc_study_wase(rgb, bkgd, scale=0.37, pad_last=True, chain=True)
        assert np.array_equal(got_w[:N - 1], want_w) and np.array_equal(got_w[N - 1], want_w[-1]) and np.array_equal(got_bg, want_bg)
        held16, held_echo = eng.calc_study_payload(rgb, scale=0.37, chain=True, hold=True)
        assert np.array_equal(held16, flow16) and np.array_equal(held_echo, echo16)
        assert (eng.held.N, eng.held.H, eng.held.W, eng.held.n_echo) == (N, H, W, N)
        yy, xx = np.mgrid[:H, :W]
        mask = np.ascontiguousarray(np.broadcast_to((((yy - H / 2) / (0.35 * H)) ** 2 + ((xx - W / 2) / (0.4 * W)) ** 2 < 1)[None, ..., None], (N, H, W, 1)))
        eng.hold_mask("rv", mask)
        a = eng.held_polar_project_param("rv", 0, 1 / 50.0, True, N, return_arrays=True)
        b = eng.polar_project_param(flow16, mask, 0, 1 / 50.0, True, N, return_arrays=True)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), "the held chained study differs from the returned arrays"
    finally:
        eng.close()


# ---- 4. submitted ----------------------------------------------------------------------------------------------------------------------
def test_submitted_chains_run_as_one_unit_each():
    from tee_optical_flow_amd.synth import speckle_sequence
    over = CC.overrides("odd")
    studies = [CC.rgb_of(speckle_sequence(CC.SEED + 1 + i, 4, 37, 53)) for i in range(3)]
    eng = chain_engine(**over)
    try:
        sync = [np.array(eng.calc_study(s, scale=1.5, chain=True)) for s in studies]
        assert not np.array_equal(sync[0], sync[1])
        units, steps = eng.counter("queue_units_done"), eng.counter("chain_steps")
        tickets = [eng.submit_study(s, scale=1.5, chain=True) for s in studies]
        for i in (2, 1, 0):
            assert np.array_equal(eng.wait(tickets[i]), sync[i]), f"submitted study {i}"
        d = (eng.counter("queue_units_done") - units, eng.counter("chain_steps") - steps)
        print("queue units, chain_steps grew by", d)
        assert d == (3, 9)
    finally:
        eng.close()


# ---- 5. device pointers ----------------------------------------------------------------------------------------------------------------
DEVICE_FORM = r"""
import sys
import numpy as np, torch
sys.path.insert(0, ROOT)
import tee_optical_flow_amd as T
from tests import tvl1_chain_cases as CC
fr = CC.frames("odd")
N, H, W = fr.shape
dev = torch.device("cuda", 0)
dfr = torch.from_numpy(np.array(fr)).to(dev)
out = torch.zeros((N - 1, H, W, 2), dtype=torch.float32, device=dev)
torch.cuda.synchronize()
for mb in (3, 128):                                   # two sub-batches; one
    eng = T.DenseFlow(device_id=0, max_batch=mb, **CC.overrides("odd"))
    try:
        eng.setUseInitialFlow(True)
        host = np.array(eng.calc_batch(fr, scale=2.0, chain=True))
        host_it = eng.last_iters()
        eng.calc_seq_device(dfr.data_ptr(), N, H, W, out.data_ptr(), scale=2.0, chain=True)
        assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(eng.last_iters(), host_it), mb
        try:
            eng.calc_seq_device(dfr.data_ptr(), N, H, W, out.data_ptr())
            raise SystemExit("no refusal of the unarmed call")
        except T.OpticalFlowCalculationError as e:
            assert e.code == 2 and "tf_calc_pairs_init" in str(e), e
    finally:
        eng.close()
print("device form ok")
"""


def test_device_pointer_form_equals_host_form():
    """tf_calc_seq_device, armed, on torch tensors (a child process with torch imported first: the engine and torch must share one HIP
    runtime): equal to the host form"""
    r = subprocess.run([sys.executable, "-c", DEVICE_FORM.replace("ROOT", repr(ROOT))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device form ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- 6. state and refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_spent_flag(oracle):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import _lib
    Err = T.OpticalFlowCalculationError
    fr = CC.frames("one")
    eng = T.DenseFlow(**CC.overrides("one"))
    try:
        with pytest.raises(Err, match="useInitialFlow is clear") as e:       # arming with the flag clear
            eng.chain_next()
        assert e.value.code == _lib.TF_ERR_UNSUPPORTED
        with pytest.raises(Err, match="useInitialFlow is clear"):
            eng.calc_batch(fr, chain=True)
        assert np.array_equal(eng.calc_batch(fr[:2])[0], oracle.tvl1_calc(fr[0], fr[1], oracle.default_params(**CC.overrides("one")))), "nothing was left armed"
        eng.setUseInitialFlow(True)
        jobs = eng.counter("queue_jobs")
        eng.chain_next()                                                      # an armed pairs call
        with pytest.raises(Err, match="tf_chain_next arms a sequence call") as e:
            eng.calc(fr[0], fr[1], np.zeros(fr.shape[1:] + (2,), np.float32))
        assert e.value.code == _lib.TF_ERR_INVALID_ARG
        with pytest.raises(Err, match="tf_calc_pairs_init") as e:            # the refused call has spent the flag: the old refusal, old text
            eng.calc_batch(fr)
        assert e.value.code == _lib.TF_ERR_UNSUPPORTED
        eng.chain_next()
        with pytest.raises(Err, match="tf_chain_next arms a sequence call"):
            eng.submit_pairs(fr[:-1], fr[1:])
        eng.chain_next()
        eng.chain_next(False)                                                 # disarmed
        with pytest.raises(Err, match="tf_calc_pairs_init"):
            eng.calc_study(CC.rgb_of(fr))
        eng.chain_next()                                                      # spent by a sequence call refused for its arguments
        st = _lib.TfStats()
        rc = eng._L.tf_calc_seq(eng._h, fr.ctypes.data, 1, fr.shape[1], fr.shape[2], 1.0, np.empty(8, np.float32).ctypes.data, C.byref(st))
        assert rc == _lib.TF_ERR_INVALID_ARG
        with pytest.raises(Err, match="tf_calc_pairs_init"):
            eng.calc_batch(fr)
        assert eng.counter("queue_jobs") == jobs and not eng._jobs, "a refused call was queued"
        two = eng.calc_batch(fr[:2], chain=True)                              # a 2-frame chain is the plain solve
        assert np.array_equal(two[0], oracle.tvl1_calc(fr[0], fr[1], oracle.default_params(**CC.overrides("one"))))
        eng.setUseInitialFlow(False)
        assert np.array_equal(eng.calc_batch(fr)[2], oracle.tvl1_calc(fr[2], fr[3], oracle.default_params(**CC.overrides("one")))), "flag off: the plain solve"
        assert eng._L.tf_abi_version() == 2
    finally:
        eng.close()
    cuda = T.DenseFlow(variant="cuda")
    try:
        with pytest.raises(Err, match="TF_VARIANT_CUDA") as e:
            cuda.chain_next()
        assert e.value.code == _lib.TF_ERR_UNSUPPORTED
    finally:
        cuda.close()
    deep = T.createOptFlow_DeepFlow()
    try:
        with pytest.raises(Err, match="DeepFlow") as e:
            deep.chain_next()
        assert e.value.code == _lib.TF_ERR_UNSUPPORTED
    finally:
        deep.close()


def test_nothing_of_one_chain_leaks_into_the_next():
    """a 97x131 chain, then a 37x53 chain on the same handle: what a fresh handle gives"""
    over = CC.overrides("odd")
    used = chain_engine(**over)
    try:
        used.calc_batch(CC.frames("short"), chain=True)
        got = np.array(used.calc_batch(CC.frames("odd"), chain=True))
        got_it = used.last_iters()
    finally:
        used.close()
    fresh = chain_engine(**over)
    try:
        assert np.array_equal(got, fresh.calc_batch(CC.frames("odd"), chain=True)) and np.array_equal(got_it, fresh.last_iters())
    finally:
        fresh.close()
