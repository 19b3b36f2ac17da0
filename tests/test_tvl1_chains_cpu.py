"""Chains in lock-step (include/teeflow.h, tf_calc_chains; DenseFlow.calc_chains & co.) without a GPU: the Python layer's checks of the
list it is given, which run before any library call, and the library's pure helper that orders the chains by length and says where each
chain's results go (tf_dbg_chain_order: host arithmetic, no device call)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tee_optical_flow_amd import OpticalFlowCalculationError
from tee_optical_flow_amd.dense_flow import DenseFlow, _chain_stacks


def gray(n, h=8, w=12):
    return np.zeros((n, h, w), np.uint8)


def test_accepted_lists_come_back_contiguous_with_their_size():
    a, b = gray(5)[:, ::1], np.zeros((3, 16, 12), np.uint8)[:, ::2]            # (b: a strided view of 3 x 8 x 12)
    out, H, W = _chain_stacks([a, b], "frames", 3)
    assert (H, W) == (8, 12) and [o.shape for o in out] == [(5, 8, 12), (3, 8, 12)]
    assert all(o.flags["C_CONTIGUOUS"] and o.dtype == np.uint8 for o in out)
    out, H, W = _chain_stacks((np.zeros((2, 4, 6, 3), np.uint8),), "rgb", 4)
    assert (H, W) == (4, 6) and len(out) == 1


@pytest.mark.parametrize("stacks,ndim,match", [
    ([gray(4), gray(4, 8, 13)], 3, "one frame size"),                          # mixed shapes
    ([gray(4), gray(3, 9, 12)], 3, "one frame size"),
    ([], 3, "non-empty list"),                                                 # empty list
    ((), 3, "non-empty list"),
    (gray(4), 3, "non-empty list"),                                            # one array is not a list of chains
    ([gray(4), gray(4).astype(np.float32)], 3, "uint8"),                       # wrong dtype
    ([gray(4).astype(np.int16)], 3, "uint8"),
    ([gray(4), gray(1)], 3, "at least 2 frames"),                              # a 1-frame chain
    ([gray(4)[0]], 3, "3 dimensions"),
    ([np.zeros((3, 8, 12, 4), np.uint8)], 4, r"\[N,H,W,3\]"),                  # RGB studies have three channels
    ([np.zeros((3, 8, 12, 3), np.uint8), gray(3)], 4, "4 dimensions"),
])
def test_refused_lists(stacks, ndim, match):
    with pytest.raises(OpticalFlowCalculationError, match=match):
        _chain_stacks(stacks, "frames", ndim)


def test_public_methods_check_the_list_before_any_library_call():
    """an object that has no library and no handle: the checks come first"""
    eng = object.__new__(DenseFlow)
    for call in (lambda: eng.calc_chains([gray(3), gray(3, 9, 9)]), lambda: eng.calc_chains([]), lambda: eng.calc_study_chains([gray(3)]),
                 lambda: eng.calc_study_chains_payload([np.zeros((1, 8, 8, 3), np.uint8)]),
                 lambda: eng.calc_chains_device([1, 2], [3], 8, 8, [5, 6]), lambda: eng.calc_chains_device([1], [1], 8, 8, [5])):
        with pytest.raises(OpticalFlowCalculationError):
            call()


def chain_order(n_frames):
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    n = len(n_frames)
    order, first = (C.c_int * n)(), (C.c_longlong * n)()
    assert L.tf_dbg_chain_order((C.c_int * n)(*n_frames), n, order, first) == _lib.TF_OK
    return list(order), list(first)


def test_order_is_longest_first_stable_and_results_map_back():
    for lengths in ([5, 5, 4, 2], [2, 2, 2], [3], [2, 9, 2, 9, 5], [4, 3, 4, 3, 4]):
        for n_frames in set(itertools.permutations(lengths)):
            order, first = chain_order(n_frames)
            assert sorted(order) == list(range(len(n_frames))), "a permutation of the caller's indices"
            by_slot = [n_frames[i] for i in order]
            assert by_slot == sorted(n_frames, reverse=True), "longest first"
            for a, b in zip(order, order[1:]):
                assert n_frames[a] > n_frames[b] or a < b, "ties keep the caller's order"
            # the chains running at step k are a prefix of the slots
            for k in range(max(n_frames) - 1):
                running = [n - 1 > k for n in by_slot]
                assert running == sorted(running, reverse=True)
            # chain i's pairs start behind those of the chains the caller put before it
            assert first == [sum(n - 1 for n in n_frames[:i]) for i in range(len(n_frames))]
    assert chain_order([3, 5, 5, 2, 4]) == ([1, 2, 4, 0, 3], [0, 2, 6, 10, 11])


def test_order_helper_refuses_nothing_to_order():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    assert L.tf_dbg_chain_order(None, 1, None, None) == _lib.TF_ERR_INVALID_ARG
    one = (C.c_int * 1)(3)
    assert L.tf_dbg_chain_order(one, 0, (C.c_int * 1)(), None) == _lib.TF_ERR_INVALID_ARG
    out = (C.c_int * 1)(7)
    assert L.tf_dbg_chain_order(one, 1, out, None) == _lib.TF_OK and out[0] == 0


def test_last_iters_splits_by_chain():
    """last_iters() after a lock-step call: the library's chain-after-chain counts cut at the chains' pair counts"""
    eng = object.__new__(DenseFlow)
    counts = np.arange(6 * 2 * 1 * 2, dtype=np.int32)

    class L:
        @staticmethod
        def tf_get_iters(h, out, n, written):
            C.memmove(out, counts.ctypes.data, n * 4)
            return 0
    eng._L, eng._h = L, None
    eng.last_stats = dict(n_pairs=6, nscales_used=2, warps=1)
    eng._last_chain_pairs = [3, 1, 2]
    got = eng.last_iters()
    assert [g.shape for g in got] == [(3, 2, 1, 2), (1, 2, 1, 2), (2, 2, 1, 2)]
    assert np.array_equal(np.concatenate(got).ravel(), counts)
    eng._last_chain_pairs = None
    assert eng.last_iters().shape == (6, 2, 1, 2)
