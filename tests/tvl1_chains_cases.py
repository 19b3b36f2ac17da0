"""Chains in lock-step (include/teeflow.h, tf_calc_chains): the chains derived from the cases of tests/tvl1_chain_cases, their expected
results, and the rule that says in which u buffer a finished pair leaves its flow.  A helper module of tests/test_gpu_tvl1_chains.py:
nothing here is collected.

The expected values of a chain are tvl1_chain_cases.composed_chain of that chain's frames -- the oracle's stages composed on the CPU --
computed once per process and shared, read-only."""
import numpy as np

from tests import tvl1_chain_cases as CC
from tests import tvl1_ref64_cases as K


def derived(fr):
    """name -> frames of the S = 4 chains of a case's frames, in an order that is deliberately not sorted by length: one shorter; the
    first two frames only (ends after step 0); the frames; the frames reversed.  The library's order is then (fwd, rev, tail, two)."""
    return {"tail": np.ascontiguousarray(fr[1:]), "two": np.ascontiguousarray(fr[:2]), "fwd": np.ascontiguousarray(fr),
            "rev": np.ascontiguousarray(fr[::-1])}


def seed_buffers(iters_by_chain, inner, median, step):
    """step k >= 1 -> the u buffers the chains that solve a pair at step k seed it from: final_ubase of their pair k-1"""
    longest = max(len(it) for it in iters_by_chain)
    return {k: sorted({final_ubase(it[k - 1], inner, median, step) for it in iters_by_chain if len(it) > k}) for k in range(1, longest)}


_expected = {}


def expected(O, key, fr, over):
    """composed_chain of one chain -> (flows, iters, levels), cached under `key`"""
    if key not in _expected:
        out = CC.composed_chain(O, np.ascontiguousarray(fr), K.params(**over))
        out[0].setflags(write=False)
        out[1].setflags(write=False)
        _expected[key] = out
    return _expected[key]


def final_ubase(iters, inner, median, step):
    """The u buffer (0 or 1) that holds a finished pair's level-0 flow, from its executed counts iters [levels, warps, 2] = (inner
    iterations, outer iterations) per stage.  Read off the engine's run_stage / k_stage_end and solve_pairs:
      - the pair starts in buffer 0 at its coarsest level (k_ctl_set, mode 0);
      - every launch of the iteration kernels that the pair takes part in writes the other buffer: a stage of n_in executed iterations
        is n_in launches in the one-iteration forms (step 1: tiles, strips) and (n_in + 1) // 2 in the two-iteration form (step 2), where
        a launch that runs the pair's last, odd iteration still flips once;
      - every median pass flips it too: one per executed outer iteration, n_out, when median filtering is on;
      - the upsample to the next finer level (k_flow_up, then k_ctl_set mode 1) flips it once per level below the coarsest.
    So ubase = (sum over stages of launches + medians, + levels - 1) mod 2."""
    iters = np.asarray(iters)
    n_in, n_out = iters[..., 0].astype(np.int64), iters[..., 1].astype(np.int64)
    launches = (n_in + 1) // 2 if step == 2 else n_in
    return int((launches.sum() + (n_out.sum() if median else 0) + iters.shape[0] - 1) % 2)


def form_step(form, inner):
    """tvl1_iter iterations per launch of an iteration form (iter_step in the engine): two for "strips2" when `inner` is even"""
    return 2 if form == "strips2" and inner % 2 == 0 else 1
