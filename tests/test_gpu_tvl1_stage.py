"""DualTVL1's stage loop on the GPU, one stage at a time (tf_dbg_stage: run_stage's own loop and k_stage_end on caller-supplied planes)
against the stage reference of tests/tvl1_stage_cases.py: every state plane and every exact error sum of every pair of a batch, per
strip layout (the "strip_test_slots" knob picks it), stop mode (NORMAL / REPLAY / EXIT blocks, both stop rules) and batch form (the
device-side work list, the fixed strips of a sub-batch above 1024 pairs, the lanes' share of the resident blocks).

Every comparison is on bit patterns, so signs of zero and denormals count; the error sums are compared as integers; no tolerance."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import tvl1_stage_cases as S
from tests.tvl1_forms import FORMS, iter_form

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {"strip_test_slots": 0, "strip_blocks": 2048}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@contextlib.contextmanager
def knobs(engine, **kw):
    """Run the block with the strip knobs set; they have their defaults again afterwards."""
    assert set(kw) <= set(KNOB_DEFAULTS)
    try:
        for name, v in kw.items():
            engine.set_tuning(name, v)
        yield engine
    finally:
        for name in kw:
            engine.set_tuning(name, KNOB_DEFAULTS[name])


def dbg_stage(engine, wx, wy, rho, state, inner, outer, ksize, thr, variant, pzero):
    """tf_dbg_stage on planes [B, h, w] -> (six state planes [B, h, w], err uint64 [B, inner * outer + 1], iters int32 [B, 2])"""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    B, h, w = wx.shape
    cst = [np.ascontiguousarray(a, np.float32) for a in (wx, wy, rho)]
    st = [np.array(a, np.float32, order="C") for a in state]
    err = np.full((B, inner * outer + 1), 0xdead, np.uint64)
    iters = np.full((B, 2), -7, np.int32)
    _lib.check(L.tf_dbg_stage(engine._h, *[_ptr(a) for a in cst], *[_ptr(a) for a in st], B, w, h, inner, outer, ksize, thr, variant,
                              pzero, _ptr(err), _ptr(iters)), engine._h, "tf_dbg_stage")
    return st, err, iters


def run_batch(engine, b, n=None):
    """the first n pairs of a batch of the cases through tf_dbg_stage"""
    n = b.B if n is None else n
    return dbg_stage(engine, b.wx[:n], b.wy[:n], b.rho[:n], [s[:n] for s in b.state], b.inner, b.outer, b.ksize, b.thr, b.variant, b.pzero)


def missed(b, got, step, what):
    """What a run of a batch misses against its reference, pair by pair -> a list of messages (empty: it passes)."""
    st, err, iters = got
    out = []
    for i in range(st[0].shape[0]):
        n = int(b.n_it[i])
        who = f"{what}: pair {i}, n_it {n}, modes {S.mode_history(n, b.total, step, b.variant)}"
        if tuple(iters[i]) != (n, int(b.n_out[i])):
            out.append(f"{who}: iters {tuple(iters[i])}, reference {(n, int(b.n_out[i]))}")
        if not np.array_equal(err[i, :n], b.ref_err[i, :n]):
            j = int(np.argmax(err[i, :n] != b.ref_err[i, :n]))
            out.append(f"{who}: error sum of iteration {j} is {int(err[i, j])}, reference {int(b.ref_err[i, j])}")
        for name, a, r in zip(S.PLANES, st, b.ref_state):
            bad = a[i].view(np.uint32) != r[i].view(np.uint32)
            if bad.any():
                y, x = np.argwhere(bad)[0]
                out.append(f"{who}: {name} differs in {int(bad.sum())} pixels, first at (y {y}, x {x}): {a[i, y, x]!r}, reference {r[i, y, x]!r}")
                break
    return out


def check(b, got, step, what):
    m = missed(b, got, step, what)
    assert not m, f"{len(m)} failures, the first ones:\n" + "\n".join(m[:6])


def form_step(form, inner, variant):
    """iterations per launch of a stage in `form`: iter_step's rule"""
    return 2 if variant == 1 or (form in ("strips2", "tiles2") and inner % 2 == 0) else 1


# ---- strip layouts, one pair -----------------------------------------------------------------------------------------------------------
_one = {}


def one_pair(O, shape, pzero):
    """planes of one pair at `shape` and oracle.iterate's six iterations on them; made once"""
    if (shape, pzero) not in _one:
        h, w = shape
        wx, wy, rho, state = S.pair_planes(O, 7, h, w, 1.0)
        if pzero:
            state = state[:2] + [np.zeros((h, w), np.float32) for _ in range(4)]
        ref = O.iterate(wx, wy, wx * wx + wy * wy, rho, *state, 6)
        _one[shape, pzero] = (wx, wy, rho, state, ref)
    return _one[shape, pzero]


def check_one(engine, O, shape, pzero, what):
    wx, wy, rho, state, ref = one_pair(O, shape, pzero)
    st, err, iters = dbg_stage(engine, wx[None], wy[None], rho[None], [s[None] for s in state], 6, 1, 0, -1.0, 0, pzero)
    for name, a, r in zip(S.PLANES, st, ref[:6]):
        bad = a[0].view(np.uint32) != r.view(np.uint32)
        assert not bad.any(), f"{what}: {name} differs in {int(bad.sum())} pixels, first at {np.argwhere(bad)[0]}"
    assert np.array_equal(err[0, :6], ref[6]) and err[0, 6] == 0, f"{what}: error sums {err[0].tolist()}, reference {ref[6].tolist()}"
    assert tuple(iters[0]) == (6, 1)


@pytest.mark.parametrize("pzero", [0, 1])
@pytest.mark.parametrize("shape", S.LAYOUT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_strips2_every_strip_layout_bit_exact(engine, oracle, shape, pzero):
    """k_iter2_rows at every (R, S) the strip rule can give one pair of this shape: strips whose length is no multiple of RY, a shorter
    last strip, one strip, strips that end at the last row; 320- and 512-thread blocks at the wide shapes."""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    h, w = shape
    ry = S.block_shape(w)[1]
    seen = []
    with iter_form(engine, "strips2"):
        for slots in S.slot_values(h, w):
            with knobs(engine, strip_test_slots=slots):
                check_one(engine, oracle, shape, pzero, f"{shape}, strip_test_slots {slots}")
            seen.append(S.strip_rule(L, 1, h, ry, slots))
    print(f"{shape} pzero {pzero}: RY {ry}, layouts (R, S) {seen}")
    assert seen[0] == (h, 1) and len(set(seen)) == len(seen) - 1


@pytest.mark.parametrize("pzero", [0, 1])
def test_strips_fixed_strip_lengths_bit_exact(engine, oracle, pzero):
    """k_iter_rows with strip_shape's n = 2, 3 and 16 steps per strip at 210 x 210 (R = 8, 12, 64: many strips, a shorter last one)"""
    ns = []
    with iter_form(engine, "strips"):
        for sb in S.STRIP_BLOCKS_210:
            n, R = S.fixed_strip_rows(210, 210, 1, sb)
            with knobs(engine, strip_blocks=sb):
                check_one(engine, oracle, (210, 210), pzero, f"strip_blocks {sb}: n {n}, R {R}")
            ns.append(n)
    assert ns == [2, 3, 16]


# ---- a batch whose pairs stop at different iterations ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ksize", [5, 3, 0])
def test_mixed70_every_pair_bit_exact(engine, oracle, ksize, form):
    """70 pairs, inner 4, outer 3, one threshold: pairs that stop after 1, 2, .. 12 iterations (REPLAY after an odd count, the median
    just skipped and just taken), stopped pairs at the ends of the 64-pair masks of the work list.  strips2 also with the resident-block
    count pretended to be 1 (many rounds), 5 (fewer than the active pairs), 12, and 1000 (every strip at its shortest)."""
    b = S.mixed70(oracle, ksize)
    step = form_step(form, b.inner, 0)
    with iter_form(engine, form):
        check(b, run_batch(engine, b), step, f"{b.name} {form}")
        for slots in (1, 5, 12, 1000) if form == "strips2" else ():
            with knobs(engine, strip_test_slots=slots):
                check(b, run_batch(engine, b), step, f"{b.name} {form} strip_test_slots {slots}")


@pytest.mark.parametrize("form", FORMS)
def test_stage_that_every_pair_leaves_early_bit_exact(engine, oracle, form):
    """The pairs of mixed70 that stop within 5 iterations, alone: a launch reports no active pair and the host stops enqueuing the
    stage; k_stage_end's counts and ping-pong halves do not depend on the launches that were never made."""
    full = S.mixed70(oracle, 5)
    b = full.subset(np.flatnonzero(full.n_it <= 5))
    assert b.B >= 40 and b.n_it.max() == 5
    with iter_form(engine, form):
        check(b, run_batch(engine, b), form_step(form, b.inner, 0), f"{b.name} {form}")


@pytest.mark.parametrize("form", ["strips2", "tiles2"])
def test_cuda70_every_pair_bit_exact(engine, oracle, form):
    """the same planes under TF_VARIANT_CUDA's stop rule (pair_mode_cuda in the work list, in k_stage_end and in the tiles)"""
    b = S.cuda70(oracle)
    with iter_form(engine, form):
        check(b, run_batch(engine, b), 2, f"{b.name} {form}")
        if form == "strips2":
            with knobs(engine, strip_test_slots=5):
                check(b, run_batch(engine, b), 2, f"{b.name} {form} strip_test_slots 5")


def test_over1024_fixed_strip_launch_bit_exact(oracle):
    """A sub-batch above 1024 pairs: k_iter2_rows' slots == 0 branch, grid (strips, 1, pairs), with two strips per pair and with one;
    the first 1024 pairs once more through the device-sized strips."""
    import tee_optical_flow_amd as T
    b = S.over1024(oracle)
    n2, R2 = S.fixed_strip_rows(b.h, b.w, b.B, 2048)
    n1, R1 = S.fixed_strip_rows(b.h, b.w, b.B, S.STRIP_BLOCKS_ONE)
    assert -(-b.h // R2) >= 2 and (n1, -(-b.h // R1)) == (16, 1)
    eng = T.DenseFlow(device_id=0, max_batch=1100)
    try:
        eng.set_tuning("min_rows_work", 0)
        with knobs(eng, strip_blocks=2048):
            two = run_batch(eng, b)
        check(b, two, 2, f"{b.name} R {R2}")
        with knobs(eng, strip_blocks=S.STRIP_BLOCKS_ONE):
            one = run_batch(eng, b)
        check(b, one, 2, f"{b.name} R {R1}")
        sized = run_batch(eng, b, 1024)
        check(b, sized, 2, f"{b.name} first 1024, device-sized strips")
        for a, c in zip(two[0] + list(two[1:]), sized[0] + list(sized[1:])):
            assert np.array_equal(a[:1024].view(np.uint32 if a.dtype == np.float32 else a.dtype),
                                  c.view(np.uint32 if c.dtype == np.float32 else c.dtype))
    finally:
        eng.close()


# ---- the lanes' share of the resident blocks, through the public API ---------------------------------------------------------------------
def test_lane_slots_pct_never_changes_a_flow(oracle):
    """12 pairs in sub-batches of 4 as queue units on the lanes, which size their strips for lane_slots_pct per cent of the resident
    blocks: flows and iteration counts of the handle solving alone, whatever the share.  (min_rows_work = 0: sub-batches this small
    would otherwise run on tiles, where the knob is not read.)"""
    import tee_optical_flow_amd as T
    from tests.test_gpu_batches import _mixed_pairs
    I0s, I1s = _mixed_pairs(12, 97, 131, seed0=700)
    eng = T.DenseFlow(device_id=0, max_batch=4)
    try:
        eng.set_tuning("min_rows_work", 0)
        eng.set_tuning("queue_lanes", 0)
        f0 = np.array(eng.calc_pairs(I0s, I1s)); it0 = eng.last_iters().copy()
        assert eng.counter("queue_jobs") == 0
        eng.set_tuning("queue_lanes", -1)
        for pct in (1, 33, 67, 100):
            eng.set_tuning("lane_slots_pct", pct)
            done = eng.counter("queue_units_done")
            f1 = np.array(eng.calc_pairs(I0s, I1s))
            assert eng.counter("queue_units_done") - done == 3, "the call did not go to the lanes as three units"
            assert np.array_equal(f1.view(np.uint32), f0.view(np.uint32)), f"lane_slots_pct {pct}: {int(np.sum(f1 != f0))} values differ"
            assert np.array_equal(eng.last_iters(), it0), f"lane_slots_pct {pct}: iteration counts differ"
        for i in (0, 5, 11):
            ref, ref_it, nl = oracle.tvl1_calc(I0s[i], I1s[i], return_iters=True)
            assert np.array_equal(it0[i], ref_it[:nl]) and np.array_equal(f0[i].view(np.uint32), ref.view(np.uint32)), f"pair {i}"
    finally:
        eng.close()


# ---- the hook's refusals -----------------------------------------------------------------------------------------------------------------
def test_stage_hook_refuses_bad_arguments(engine, oracle):
    from tee_optical_flow_amd import _lib
    from tee_optical_flow_amd.synth import speckle_pair
    L = _lib.load()
    a = np.zeros((1, 8, 8), np.float32)
    err, iters = np.zeros(16, np.uint64), np.zeros(2, np.int32)

    def call(planes=None, B=1, inner=2, outer=2, ksize=0, variant=0, e=err):
        planes = planes or [_ptr(a)] * 9
        return L.tf_dbg_stage(engine._h, *planes, B, 8, 8, inner, outer, ksize, -1.0, variant, 0, _ptr(e) if e is not None else None, _ptr(iters))

    assert call(B=4097) == _lib.TF_ERR_INVALID_ARG and b"4096" in L.tf_last_error(engine._h)
    assert call(B=0) == _lib.TF_ERR_INVALID_ARG
    assert call(inner=3, outer=1, variant=1) == _lib.TF_ERR_INVALID_ARG and b"even" in L.tf_last_error(engine._h)
    for k in range(9):
        assert call(planes=[None if j == k else _ptr(a) for j in range(9)]) == _lib.TF_ERR_INVALID_ARG
    assert call(e=None) == _lib.TF_ERR_INVALID_ARG
    assert call(ksize=4) == _lib.TF_ERR_INVALID_ARG and call(variant=2) == _lib.TF_ERR_INVALID_ARG
    assert not err.any() and not iters.any() and not a.any()                # nothing was written
    assert call(inner=3, outer=2, variant=1) == _lib.TF_OK             # an even product of an odd inner count is taken
    I0, I1, _ = speckle_pair(11, 64, 64)
    flow = engine.calc(I0, I1, None)
    assert np.array_equal(flow.view(np.uint32), oracle.tvl1_calc(I0, I1).view(np.uint32))
