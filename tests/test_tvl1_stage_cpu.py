"""The stage-level reference of tests/tvl1_stage_cases.py without a GPU: `stage_ref` chained after the oracle's warp is the oracle's own
whole solve bit for bit (both variants), the batches of tests/test_gpu_tvl1_stage.py still hold the pairs they are for, and the strip
layouts those tests ask for are the ones the strip rule gives."""
import ctypes as C

import numpy as np
import pytest

from tests import tvl1_stage_cases as S


def _warp(O, variant, I0, I1, u1, u2):
    """(wx, wy, rho) of the oracle's warp stage of `variant`"""
    if variant == 0:
        wx, wy, _, rho = O.warp(I0, I1, u1, u2)
        return wx, wy, rho
    h, w = I0.shape
    I1x, I1y = O.centered_gradient(I1)
    outs = [np.empty_like(I0) for _ in range(4)]
    O.lib().orc_warp_cuda(I0, I1, I1x, I1y, np.ascontiguousarray(u1), np.ascontiguousarray(u2), w, h, *outs)
    return outs[0], outs[1], outs[3]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mf", [5, 1])
def test_stage_ref_chained_is_the_oracles_whole_solve(oracle, variant, mf):
    """One level, two warps, an epsilon that ends the stages early: flow and iteration counts of orc_tvl1_calc == warp, stage_ref,
    warp, stage_ref.  This is what ties the stage reference (and its restated CUDA stop rule) to the oracle."""
    from tee_optical_flow_amd.synth import speckle_pairs
    O = oracle
    H, W, eps, inner, outer = 72, 88, 0.05, 6, 5
    I0s, I1s = speckle_pairs([40, 41, 42], H, W)
    P = O.default_params(nscales=1, warps=2, median_filtering=mf, epsilon=eps, inner_iterations=inner, outer_iterations=outer, variant=variant)
    thr = eps * eps * float(W * H)
    if variant == 0:
        thr = float(np.float32(thr))                    # the CPU class keeps a float, the CUDA class a double
    seen = set()
    for b in range(3):
        flow, iters, nl = O.tvl1_calc(I0s[b], I1s[b], P, return_iters=True)
        assert nl == 1
        I0, I1 = I0s[b].astype(np.float32), I1s[b].astype(np.float32)
        state = [np.zeros((H, W), np.float32) for _ in range(6)]
        for wi in range(2):
            wx, wy, rho = _warp(O, variant, I0, I1, state[0], state[1])
            state, err, n_it, n_out = S.stage_ref(O, wx, wy, rho, state, inner, outer, mf, thr, variant, wi == 0)
            assert (n_it, n_out) == tuple(iters[0, wi]), f"pair {b} warp {wi}: {(n_it, n_out)} against the oracle's {iters[0, wi]}"
            assert not err[n_it:].any() and err[:n_it].all()
            seen.add(n_it)
        got = np.stack(state[:2], -1)
        assert np.array_equal(got.view(np.uint32), flow.view(np.uint32)), f"pair {b}: {int(np.sum(got != flow))} values differ"
    assert len(seen) >= 4 and min(seen) < inner * outer, f"the stages no longer stop early: {sorted(seen)}"


@pytest.mark.parametrize("ksize", [5, 3, 0])
def test_mixed70_holds_the_pairs_it_is_for(oracle, ksize):
    b = S.mixed70(oracle, ksize)
    n, total, inner = b.n_it, b.total, b.inner
    print(b.name, "thr", b.thr, "n_it histogram", b.histogram())
    assert (b.B, b.h, b.w, inner, b.outer) == (70, 97, 131, 4, 3)
    assert (n == 1).any(), "no pair stops after its first iteration"
    assert ((n % 2 == 1) & (n > 1)).any(), "no pair stops after an odd iteration > 1 (REPLAY)"
    assert ((n % 2 == 0) & (n < total)).any() and (n == total).any()
    assert (n == inner).any() and (n == inner + 1).any(), "median just skipped / just taken"
    assert all(n[i] <= 2 for i in (0, 63, 64, 69)), n[[0, 63, 64, 69]]
    assert all(n[i] == total for i in (1, 65)), n[[1, 65]]
    assert np.array_equal(b.n_out, (n - 1) // inner + 1)
    # every sum the stop tests of the batch read is well away from the threshold
    e = b.ref_err[b.ref_err > 0].astype(np.float64) / 2.0 ** 30
    assert np.abs(e / b.thr - 1).min() > S.THR_MARGIN and float(np.float32(b.thr)) == b.thr
    assert S.has_denormals(b), "the batch no longer reaches the denormal range"
    # stops() (which chose the threshold from the never-stopping run) and stage_ref agree pair by pair
    for i in (0, 1, 17, 42, 69):
        full = S.stage_ref(oracle, b.wx[i], b.wy[i], b.rho[i], [s[i] for s in b.state], inner, b.outer, ksize, -1.0, 0, 0)[1]
        assert S.stops(full, b.thr, 0, inner) == (n[i], b.n_out[i]) and np.array_equal(full[:n[i]], b.ref_err[i, :n[i]])


def test_cuda70_and_over1024_hold_the_pairs_they_are_for(oracle):
    c = S.cuda70(oracle)
    print(c.name, "thr", c.thr, "n_it histogram", c.histogram())
    assert (c.B, c.variant, c.ksize, c.total) == (70, 1, 0, 12) and not (c.n_it % 2).any() and not c.n_out.any()
    assert (c.n_it == 2).any() and ((c.n_it == 4) | (c.n_it == 6)).any() and (c.n_it == 12).any()
    assert float(np.float32(c.thr)) == c.thr
    e = c.ref_err[c.ref_err > 0].astype(np.float64) / 2.0 ** 30
    assert np.abs(e / c.thr - 1).min() > S.THR_MARGIN
    # the running prevError of the CUDA rule is compared with the threshold too: prev = e - k * thr < thr, so e / thr near an integer
    r = e / c.thr
    assert np.abs(r - np.rint(r))[r < 16].min() > S.THR_MARGIN
    o = S.over1024(oracle)
    print(o.name, "thr", o.thr, "n_it histogram", o.histogram())
    assert (o.B, o.h, o.w, o.inner, o.outer, o.ksize) == (1025, 40, 64, 6, 1, 0)
    stopped = o.n_it < o.total
    assert 0.35 < stopped.mean() < 0.65 and (o.n_it[stopped] % 2 == 1).any() and (o.n_it[stopped] % 2 == 0).any()
    assert len({a.tobytes() for a in o.wx}) == 16
    assert stopped[:1024].any() and not stopped[:1024].all()
    e = o.ref_err[o.ref_err > 0].astype(np.float64) / 2.0 ** 30
    assert np.abs(e / o.thr - 1).min() > S.THR_MARGIN


def _strip_rule(n, H, RY, slots):
    """strip_rule of teeflow_tvl1_iter.hip.h, restated"""
    minrows = max(1, 4 * RY)
    k = -(-max(n, 1) // slots)
    s = max(1, min(k * slots // max(n, 1), max(1, H // minrows)))
    r = -(-H // s)
    return r, -(-H // r)


def test_layouts_the_gpu_tests_ask_for():
    """The (R, S) that strip_test_slots = 1 .. smax + 1 gives one pair at every shape of the layout tests, and what the table is for."""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    table = {}
    for h, w in S.LAYOUT_SHAPES:
        qx, ry, threads = S.block_shape(w)
        rows = [S.strip_rule(L, 1, h, ry, s) for s in S.slot_values(h, w)]
        assert rows == [_strip_rule(1, h, ry, s) for s in S.slot_values(h, w)]
        assert all((S_ - 1) * R < h <= S_ * R for R, S_ in rows)
        assert rows[0] == (h, 1) and rows[-1] == rows[-2], "the single strip, and the value beyond smax changes nothing"
        table[h, w] = (ry, threads, rows)
        print((h, w), "RY", ry, "threads", threads, "(R, S):", rows)
    assert {k: v[:2] for k, v in table.items()} == {(97, 131): (7, 256), (210, 210): (4, 256), (40, 300): (3, 256), (61, 16): (64, 256),
                                                    (9, 1100): (1, 320), (6, 2048): (1, 512)}
    assert len(table[210, 210][2]) == 14 and [S_ for _, S_ in table[210, 210][2][:13]] == list(range(1, 14))
    assert table[61, 16][2] == [(61, 1), (61, 1)]
    for (h, w), (ry, _, rows) in table.items():
        if (h, w) in ((97, 131), (210, 210), (40, 300)):
            assert any(R % ry for R, _ in rows), f"{(h, w)}: no strip length that is not a multiple of RY"
            assert any(S_ > 1 and h % R for R, S_ in rows), f"{(h, w)}: no layout with a shorter last strip"
            assert any(S_ > 1 and h % R == 0 for R, S_ in rows) or (h, w) == (97, 131)
    # the fixed strips of k_iter_rows at (210, 210): the strip_blocks values the GPU test uses give n = 2, 3 and 16
    assert [S.fixed_strip_rows(210, 210, 1, sb) for sb in S.STRIP_BLOCKS_210] == [(2, 8), (3, 12), (16, 64)]
    # and those of a sub-batch above 1024 pairs
    assert S.fixed_strip_rows(40, 64, 1025, 2048) == (2, 32) and S.fixed_strip_rows(40, 64, 1025, S.STRIP_BLOCKS_ONE)[1] >= 40


def test_tf_dbg_stage_refuses_bad_arguments_without_a_device():
    """null handle: TF_ERR_INVALID_ARG, nothing touched (the refusals that need a handle are in the GPU tests)"""
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    a = np.zeros((1, 4, 4), np.float32)
    p = a.ctypes.data_as(C.c_void_p)
    assert L.tf_dbg_stage(None, *([p] * 9), 1, 4, 4, 2, 1, 0, -1.0, 0, 0, p, p) == _lib.TF_ERR_INVALID_ARG
