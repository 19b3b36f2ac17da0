"""DualTVL1's chains in lock-step on the device (include/teeflow.h, tf_calc_chains; DenseFlow.calc_chains & co.): S chains of one frame
size solved in one call, step k as one batch of the chains still running, equal -- bit for bit and iteration count for iteration count --
to the oracle's stages composed on the CPU for each chain (tests/tvl1_chain_cases.composed_chain) and to a separate chained call of each
on the same handle; with slots that seed from different u buffers in one step; across sub-batches over time; in the study forms; with
fewer launches than the separate chains; and the refusals.  Each test prints its figures before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tvl1_chain_cases as CC
from tests import tvl1_chains_cases as LC
from tests import tvl1_ref64_cases as K
from tests.tvl1_forms import iter_form

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("strips2", "tiles")                      # iter_variant 2 and 0


def chain_engine(**over):
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(**over)
    eng.setUseInitialFlow(True)
    return eng


def expected(oracle, cid, names=None):
    """name -> (frames, composed flows, composed iters, levels) of the derived chains of a case"""
    chains = LC.derived(CC.frames(cid))
    return {n: (f,) + LC.expected(oracle, (cid, n), f, CC.overrides(cid)) for n, f in chains.items() if names is None or n in names}


def assert_chains(got, iters, exp, what):
    """got, iters: per chain, in the order of exp's values"""
    assert len(got) == len(iters) == len(exp)
    for (name, (fr, cf, cit, _)), g, it in zip(exp.items(), got, iters):
        g = np.asarray(g)
        print(f"{what} chain {name}: {len(fr) - 1} pairs, values that differ from composed {int(np.sum(g != cf)) if g.shape == cf.shape else g.shape}, "
              f"inner iterations {it[..., 0].sum(axis=(1, 2)).tolist()}, composed {cit[..., 0].sum(axis=(1, 2)).tolist()}")
    for (name, (fr, cf, cit, _)), g, it in zip(exp.items(), got, iters):
        assert np.array_equal(it, cit), f"{what}: iteration counts of chain {name}"
        assert np.asarray(g).dtype == np.float32 and np.array_equal(g, cf), f"{what}: flows of chain {name}"


# ---- 1. bit-equality, counts included ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cid", list(CC.CASES))
def test_lockstep_is_the_composed_chain_and_the_separate_chain_of_each(oracle, cid, form):
    """the four derived chains of every case, passed in an order that is not the library's (by length): the internal ordering, the
    ragged ends (one chain ends after step 0, one a step before the longest) and the scatter back to the caller's order"""
    exp = expected(oracle, cid)
    eng = chain_engine(**CC.overrides(cid))
    try:
        with iter_form(eng, form):
            steps = eng.counter("chain_steps")
            got = [np.array(g) for g in eng.calc_chains([fr for fr, *_ in exp.values()])]
            iters, stats = eng.last_iters(), eng.last_stats
            grew = eng.counter("chain_steps") - steps
            sep = []
            for fr, *_ in exp.values():
                sep.append((np.array(eng.calc_batch(fr, chain=True)), eng.last_iters()))
        n_pairs = sum(len(fr) - 1 for fr, *_ in exp.values())
        print(f"{cid}/{form}: {n_pairs} pairs, chain_steps grew by {grew}, stats n_pairs {stats['n_pairs']}, levels {stats['nscales_used']}")
        assert grew == n_pairs == stats["n_pairs"] and stats["nscales_used"] == next(iter(exp.values()))[3]
        assert isinstance(iters, list)
        assert_chains(got, iters, exp, f"{cid}/{form}")
        for (name, _), g, it, (sf, sit) in zip(exp.items(), got, iters, sep):
            assert np.array_equal(g, sf) and np.array_equal(it, sit), f"chain {name} differs from calc_batch(chain=True) of its frames"
        assert not np.array_equal(got[2][0], got[3][0]), "two chains gave one result"
    finally:
        eng.close()


# ---- 2. different seed buffers in one step ------------------------------------------------------------------------------------------------
def test_some_step_seeds_its_slots_from_both_u_buffers(oracle):
    """The hazard that is new with B slots: at a step, two slots whose finished pairs left their level-0 flow in DIFFERENT u buffers,
    so that k_chain_seed keeps one and moves the other in the same launch.  Which buffer is tvl1_chains_cases.final_ubase's rule over
    the pair's executed counts; the counts are the oracle's, which test 1 shows to be the engine's.  Test 1 runs every (case, form)
    listed here; this assertion keeps it from silently ceasing to cover the hazard."""
    mixed = []
    for cid in CC.CASES:
        exp = expected(oracle, cid)
        P = K.params(**CC.overrides(cid))
        for form in FORMS:
            seeds = LC.seed_buffers([cit for _, _, cit, _ in exp.values()], P.inner_iterations, P.median_filtering > 1,
                                    LC.form_step(form, P.inner_iterations))
            print(f"{cid}/{form}: u buffers the slots of step k seed from: {seeds}")
            mixed += [(cid, form, k) for k, bufs in seeds.items() if bufs == [0, 1]]
    print("steps whose slots seed from both buffers:", mixed)
    assert mixed, "no step of any case has slots that seed from different u buffers: derive other chains"


# ---- 3. sub-batches over time -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_batch,names,why", [
    (3, ("tail", "fwd"), "6 frame slots, S = 2: one step per sub-batch, the seeds cross three boundaries, then S = 1"),
    (5, ("two", "fwd"), "10 frame slots, S = 2: two steps per sub-batch, chain `two` ends inside the first"),
    (3, ("tail", "two", "fwd"), "S = 3 is the limit: every sub-batch is one step"),
])
def test_sub_batches_over_time_carry_the_seeds(oracle, max_batch, names, why):
    exp = {n: expected(oracle, "odd")[n] for n in names}
    eng = chain_engine(max_batch=max_batch, **CC.overrides("odd"))
    try:
        jobs = eng.counter("queue_jobs")
        got = eng.calc_chains([fr for fr, *_ in exp.values()])
        iters = eng.last_iters()
        print(f"max_batch {max_batch}, chains {names} ({why}); queue jobs grew by {eng.counter('queue_jobs') - jobs}")
        assert_chains(got, iters, exp, f"max_batch {max_batch}")
        assert eng.counter("queue_jobs") == jobs and eng.counter("queue_outstanding") == 0, "a lock-step call went to the lanes"
    finally:
        eng.close()


def test_lockstep_behind_submitted_jobs_is_solved_by_a_lane(oracle):
    """while a submitted job is in flight a lock-step call queues behind it as one unit, which a lane solves: the same results.  The job
    in flight is one chain of 71 pairs, 71 single-pair solves one after the other on one lane (a quarter of a second), and the
    lock-step call is made right behind its submission: it finds the job outstanding, so both are queue jobs of one unit each"""
    exp = {n: expected(oracle, "odd")[n] for n in ("tail", "two", "fwd")}
    fr = exp["fwd"][0]
    long = np.ascontiguousarray(np.concatenate([fr, fr[::-1][1:]] * 9)[:72])
    eng = chain_engine(max_batch=3, **CC.overrides("odd"))
    try:
        want_long = np.array(eng.calc_batch(long, chain=True))
        jobs, units, steps = eng.counter("queue_jobs"), eng.counter("queue_units_done"), eng.counter("chain_steps")
        ticket = eng.submit_batch(long, chain=True)
        got = eng.calc_chains([f for f, *_ in exp.values()])
        iters = eng.last_iters()
        still = eng.counter("queue_outstanding")
        assert_chains(got, iters, exp, "behind a submitted job")
        assert np.array_equal(eng.wait(ticket), want_long)
        d = (eng.counter("queue_jobs") - jobs, eng.counter("queue_units_done") - units)
        print(f"queue jobs, units done grew by {d}; jobs outstanding when the lock-step call returned: {still}")
        assert d == (2, 2), "the lock-step call was not queued as one unit behind the job in flight"
        assert eng.counter("chain_steps") - steps == 71 + 8 and eng.counter("queue_outstanding") == 0
    finally:
        eng.close()


def test_more_chains_than_a_sub_batch_holds_are_refused():
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import _lib
    fr = CC.frames("odd")
    eng = chain_engine(max_batch=3, **CC.overrides("odd"))
    try:
        with pytest.raises(T.OpticalFlowCalculationError, match="at most 3") as e:
            eng.calc_chains([fr[:2]] * 4)
        print(e.value)
        assert e.value.code == _lib.TF_ERR_UNSUPPORTED and "4 chains" in str(e.value)
        assert eng.counter("queue_outstanding") == 0
        assert len(eng.calc_chains([fr[:2]] * 3)) == 3, "the handle is usable after the refusal, at the limit"
    finally:
        eng.close()


# ---- 4. output forms ------------------------------------------------------------------------------------------------------------------
def test_study_forms_equal_the_chained_study_calls():
    scale = 0.04 * 50
    gray = CC.frames("odd")
    studies = [CC.rgb_of(gray[1:]), CC.rgb_of(gray), CC.rgb_of(gray[::-1][:3])]
    eng = chain_engine(**CC.overrides("odd"))
    try:
        for pad_last in (False, True):
            want = [np.array(eng.calc_study(s, scale=scale, pad_last=pad_last, chain=True)) for s in studies]
            got = eng.calc_study_chains(studies, scale=scale, pad_last=pad_last)
            for i, (g, w) in enumerate(zip(got, want)):
                print(f"float32 study {i}, pad_last {pad_last}: shape {g.shape}, values that differ {int(np.sum(np.asarray(g) != w))}")
                assert g.dtype == np.float32 and g.shape == w.shape == ((len(studies[i]) if pad_last else len(studies[i]) - 1,) + gray.shape[1:] + (2,))
                assert np.array_equal(g, w)
            want = [tuple(np.array(a) for a in eng.calc_study_payload(s, scale=scale, pad_last=pad_last, chain=True)) for s in studies]
            got = eng.calc_study_chains_payload(studies, scale=scale, pad_last=pad_last)
            for i, ((g, ge), (w, we)) in enumerate(zip(got, want)):
                print(f"float16 study {i}, pad_last {pad_last}: flow values that differ {int(np.sum(np.asarray(g) != w))}, echo {int(np.sum(np.asarray(ge) != we))}")
                assert g.dtype == np.float16 and ge.dtype == np.float16 and g.shape == w.shape and ge.shape == we.shape == studies[i].shape[:3]
                assert np.array_equal(g, w) and np.array_equal(ge, we)
        assert not np.array_equal(want[0][0][0], want[1][0][0])
        got = eng.calc_study_chains_payload(studies, scale=scale, echo=False)
        assert all(e is None for _, e in got) and all(np.array_equal(g, w) for (g, _), (w, _) in zip(got, want))
        assert eng.held is None, "a lock-step call holds nothing"
    finally:
        eng.close()


DEVICE_FORM = r"""
import sys
import numpy as np, torch
sys.path.insert(0, ROOT)
import tee_optical_flow_amd as T
from tests import tvl1_chain_cases as CC
fr = np.array(CC.frames("odd"))
chains = [fr[1:], fr[:2], fr]
H, W = fr.shape[1:]
dev = torch.device("cuda", 0)
dfr = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in chains]
outs = [torch.zeros((len(c) - 1, H, W, 2), dtype=torch.float32, device=dev) for c in chains]
torch.cuda.synchronize()
for mb in (3, 128):                                   # sub-batches over time; one
    eng = T.DenseFlow(device_id=0, max_batch=mb, **CC.overrides("odd"))
    try:
        eng.setUseInitialFlow(True)
        host = [np.array(g) for g in eng.calc_chains(chains, scale=2.0)]
        host_it = eng.last_iters()
        eng.calc_chains_device([t.data_ptr() for t in dfr], [len(c) for c in chains], H, W, [t.data_ptr() for t in outs], scale=2.0)
        dev_it = eng.last_iters()
        for i in range(len(chains)):
            print("max_batch", mb, "chain", i, "values that differ", int(np.sum(outs[i].cpu().numpy() != host[i])))
            assert np.array_equal(outs[i].cpu().numpy(), host[i]) and np.array_equal(dev_it[i], host_it[i]), (mb, i)
            outs[i].zero_()
    finally:
        eng.close()
print("device form ok")
"""


def test_device_pointer_form_equals_host_form():
    """tf_calc_chains_device on torch tensors (a child process with torch imported first: the engine and torch must share one HIP
    runtime): equal to the host form"""
    r = subprocess.run([sys.executable, "-c", DEVICE_FORM.replace("ROOT", repr(ROOT))], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "device form ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- 5. it really is lock-step -----------------------------------------------------------------------------------------------------------
def test_lockstep_launches_carry_all_chains():
    """S = 3 chains of equal length whose stages all run to their iteration budget (tvl1_chain_cases: no stage of `trunc` stops early),
    so every launch count here is the schedule's and does not depend on when the host read a stop report"""
    fr = np.array(CC.frames("trunc"))
    chains = [fr, np.ascontiguousarray(fr[::-1]), np.ascontiguousarray(fr[[0, 1, 0, 1]])]
    eng = chain_engine(**CC.overrides("trunc"))
    try:
        sep, sep_flows = [], []
        for c in chains:
            sep_flows.append(np.array(eng.calc_batch(c, chain=True)))
            sep.append(eng.last_stats["iter_launches"])
        steps = eng.counter("chain_steps")
        got = eng.calc_chains(chains)
        lock, grew = eng.last_stats["iter_launches"], eng.counter("chain_steps") - steps
        print(f"tvl1_iter launches: lock-step {lock}, separate chains {sep} (sum {sum(sep)}); chain_steps grew by {grew}")
        assert all(np.array_equal(g, s) for g, s in zip(got, sep_flows))
        assert max(sep) <= lock < sum(sep)
        assert grew == sum(len(c) - 1 for c in chains) == eng.last_stats["n_pairs"]
    finally:
        eng.close()


# ---- 6. refusals and state -----------------------------------------------------------------------------------------------------------------
def raw_chains(eng, frames, n_frames, n, H, W, outs, fn="tf_calc_chains"):
    """the C call with per-chain pointers given as ints or None -> (rc, message)"""
    from tee_optical_flow_amd import _lib
    arr = lambda ps: None if ps is None else (C.c_void_p * max(len(ps), 1))(*ps)
    nf = None if n_frames is None else (C.c_int * max(len(n_frames), 1))(*n_frames)
    rc = getattr(eng._L, fn)(eng._h, arr(frames), nf, n, H, W, 1.0, arr(outs), C.byref(_lib.TfStats()))
    return rc, eng._L.tf_last_error(eng._h).decode()


def test_refusals_spent_flags_and_what_the_handle_gives_afterwards(oracle):
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import _lib
    Err, INV, UNS = T.OpticalFlowCalculationError, _lib.TF_ERR_INVALID_ARG, _lib.TF_ERR_UNSUPPORTED
    over, fr = CC.overrides("one"), np.array(CC.frames("one"))
    N, H, W = fr.shape
    chains = [fr[1:], fr]
    eng = T.DenseFlow(**over)
    try:
        I0s, I1s = fr[:-1], fr[1:]
        pairs_before = np.array(eng.calc_pairs(I0s, I1s))
        with pytest.raises(Err, match="useInitialFlow is clear") as e:            # the flag is clear
            eng.calc_chains(chains)
        assert e.value.code == UNS
        eng.setUseInitialFlow(True)
        chain_before = np.array(eng.calc_batch(fr, chain=True))
        chain_it_before = eng.last_iters()
        jobs = eng.counter("queue_jobs")
        out = np.zeros((N - 1, H, W, 2), np.float32)
        p, o = fr.ctypes.data, out.ctypes.data
        for what, args, code, text in [
            ("n_chains 0", ([p], [N], 0, H, W, [o]), INV, "n_chains must be >= 1"),
            ("n_chains -1", ([p], [N], -1, H, W, [o]), INV, "n_chains must be >= 1"),
            ("a 1-frame chain", ([p, p], [N, 1], 2, H, W, [o, o]), INV, "chain 1 has 1 frames"),
            ("null frames array", (None, [N], 1, H, W, [o]), INV, "null"),
            ("null n_frames", ([p], None, 1, H, W, [o]), INV, "null"),
            ("null flows array", ([p], [N], 1, H, W, None), INV, "null"),
            ("a null frame pointer", ([p, None], [N, N], 2, H, W, [o, o]), INV, "null frame or flow pointer of chain 1"),
            ("a null flow pointer", ([p, p], [N, N], 2, H, W, [None, o]), INV, "null frame or flow pointer of chain 0"),
            ("an image above 2^24 pixels", ([p], [N], 1, 4097, 4097, [o]), UNS, "2\\^24"),
            ("a non-positive size", ([p], [N], 1, 0, W, [o]), INV, "bad sizes"),
        ]:
            for fn in ("tf_calc_chains", "tf_calc_chains_device"):
                rc, msg = raw_chains(eng, *args, fn=fn)
                print(f"{fn}, {what}: code {rc}: {msg}")
                assert rc == code and __import__("re").search(text, msg), (what, rc, msg)
        rc = eng._L.tf_calc_chains_rgb(eng._h, (C.c_void_p * 1)(p), (C.c_int * 1)(1), 1, H, W, 1.0, 1, (C.c_void_p * 1)(o), None, C.byref(_lib.TfStats()))
        assert rc == INV and "at least 2 frames" in eng._L.tf_last_error(eng._h).decode()
        assert eng._L.tf_calc_chains(None, None, None, 1, H, W, 1.0, None, None) == INV
        # an armed tf_hold_next: refused, and spent
        eng.hold_next()
        with pytest.raises(Err, match="tf_hold_next was armed") as e:
            eng.calc_study_chains_payload([CC.rgb_of(fr)])
        assert e.value.code == UNS
        eng.calc_study_payload(CC.rgb_of(fr), chain=True)
        assert eng.held is None, "the refused lock-step call did not spend tf_hold_next's flag"
        eng.hold_next()
        with pytest.raises(Err, match="tf_hold_next was armed"):
            eng.calc_chains(chains)
        # an armed tf_chain_next is spent: by a call that is solved, and by one that is refused
        eng.chain_next()
        got = [np.array(g) for g in eng.calc_chains(chains)]
        got_it = eng.last_iters()
        with pytest.raises(Err, match="tf_calc_pairs_init"):
            eng.calc_batch(fr)
        eng.chain_next()
        rc, _ = raw_chains(eng, [p], [N], 0, H, W, [o])
        assert rc == INV
        with pytest.raises(Err, match="tf_calc_pairs_init"):
            eng.calc_batch(fr)
        print("queue jobs grew by", eng.counter("queue_jobs") - jobs, "; outstanding", eng.counter("queue_outstanding"))
        assert eng.counter("queue_jobs") == jobs and eng.counter("queue_outstanding") == 0 and not eng._jobs, "a refused call was queued"
        # what the lock-step call gave, and what the handle gives after it
        assert np.array_equal(got[1], chain_before) and np.array_equal(got_it[1], chain_it_before)
        assert np.array_equal(got[0], LC.expected(oracle, ("one", "tail"), fr[1:], over)[0])
        assert np.array_equal(eng.calc_batch(fr, chain=True), chain_before) and np.array_equal(eng.last_iters(), chain_it_before)
        eng.setUseInitialFlow(False)
        assert np.array_equal(eng.calc_pairs(I0s, I1s), pairs_before)
        assert eng._L.tf_abi_version() == 2
    finally:
        eng.close()
    cuda = T.DenseFlow(variant="cuda")
    try:
        with pytest.raises(Err, match="TF_VARIANT_CUDA") as e:
            cuda.calc_chains(chains)
        assert e.value.code == UNS
    finally:
        cuda.close()
    deep = T.createOptFlow_DeepFlow()
    try:
        with pytest.raises(Err, match="DeepFlow") as e:
            deep.calc_chains(chains)
        assert e.value.code == UNS
    finally:
        deep.close()
