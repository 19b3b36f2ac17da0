"""tests/luma_cases.py is what it claims: the order-explicit luma equals a pure-Python evaluation of the same expression, `condition`
reproduces the reference's own conditioning fixtures, and the corpus holds what tests/test_gpu_luma.py relies on -- exact .5 ties, pixels
on histogram edges, ramps that fire each of hist_bin's two fix-up steps, frames that lose every base byte with a lost extreme.  The
counts are deterministic (elementwise float64), so they are asserted as equalities."""
import os

import numpy as np
import pytest

from tests import luma_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def one_luma():
    return LC.luma(LC.cube_one_frame()[0])


def test_luma_is_the_plain_python_expression():
    rng = np.random.default_rng(1)
    tri = np.concatenate([rng.integers(0, 256, (20000, 3), dtype=np.uint8),
                          np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)])
    want = [((int(R) / 255.0) * 0.2125 + (int(G) / 255.0) * 0.7154) + (int(B) / 255.0) * 0.0721 for R, G, B in tri]
    assert np.array_equal(LC.luma(tri).view(np.uint64), np.array(want, np.float64).view(np.uint64))
    assert LC.luma(tri[-8:])[0] == 0.0 and LC.luma(tri[-1:])[0] == 1.0


def test_condition_reproduces_the_reference_fixtures():
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_host_side.npz"))
    assert np.array_equal(LC.condition(z["cond_in_rgb"][None])[0], z["cond_out_u8"])
    assert np.array_equal(LC.condition(z["cond_in_ramp"][None])[0], z["cond_out_ramp"])


def test_reference_is_the_single_functions_in_one_pass():
    for rgb in (LC.flat(), LC.ramps(), LC.sizes_calls()["5x1x257"], LC.cube_frames()[100:103]):
        ref = LC.reference(rgb)
        assert np.array_equal(ref["cond"], LC.condition(rgb)) and np.array_equal(ref["hist"], LC.hist(rgb))
        assert np.array_equal(ref["minmax"].view(np.uint64), LC.minmax(rgb).view(np.uint64))
        assert np.array_equal(ref["thr"].view(np.uint64), LC.threshold(rgb).view(np.uint64)) and np.array_equal(ref["echo"], LC.echo_bits(rgb))
        assert ref["cond"].dtype == np.uint8 and ref["echo"].dtype == np.uint16 and ref["hist"].shape == (len(rgb), 256)


def test_flat_frames_condition_to_zero_and_have_no_histogram():
    f = LC.flat()
    assert not LC.condition(f).any() and not LC.hist(f).any()
    mm = LC.minmax(f)
    assert np.array_equal(mm[:, 0], mm[:, 1]) and np.array_equal(LC.threshold(f), mm[:, 0]) and mm[0, 0] == 0.0 and mm[1, 0] == 1.0
    lit = LC.one_lit()
    assert np.array_equal(LC.minmax(lit), [[0.0, (1 / 255.0) * 0.2125], [0.0, 1.0]])
    assert sorted(LC.condition(lit).sum((1, 2)).tolist()) == [255, 255]                # the lit pixel alone, at full scale


def test_cube_as_one_frame_has_its_ties_and_edge_pixels(one_luma):
    assert one_luma.min() == 0.0 and one_luma.max() == 1.0
    assert LC.ties(one_luma) == 1040
    edges = np.linspace(0.0, 1.0, LC.NBINS + 1)
    assert int(np.isin(one_luma.ravel(), edges[1:-1]).sum()) == 82
    # floor(x + .5) in place of rint gives another byte at the ties above an even integer: 500 of the 1,040
    x = one_luma * 255.0
    assert int((np.floor(x + 0.5) != np.rint(x)).sum()) == 500


def test_hist_model_is_np_histogram_and_the_cube_fires_no_fixup(one_luma):
    c, d, i = LC.numpy_hist_model(one_luma)
    assert np.array_equal(c, LC.hist_luma(one_luma)) and (d, i) == (0, 0)
    n_ties = fix = 0
    pairs = set()
    for f in LC.cube_frames():
        g = LC.luma(f)
        c, d, i = LC.numpy_hist_model(g)
        assert np.array_equal(c, LC.hist_luma(g))
        fix += d + i
        n_ties += LC.ties(g)
        pairs.add((g.min(), g.max()))
    assert fix == 0 and n_ties == 387 and len(pairs) == 256


def test_hist_model_is_np_histogram_on_the_rest_of_the_corpus():
    for name, call in LC.corpus_calls(cube=False).items():
        for f in call[:: 7 if name.startswith("planted") else 1]:      # (a planted call's frames are one multiset of values)
            g = LC.luma(f)
            if g.min() < g.max():
                assert np.array_equal(LC.numpy_hist_model(g)[0], LC.hist_luma(g)), name


def test_ramps_fire_both_fixups():
    fired = {r: LC.numpy_hist_model(LC.luma(LC.grey_ramp(*r)))[1:] for r in LC.ramp_ranges()}
    assert set(LC.RAMPS_FIXED) >= {(0, 132), (0, 160), (1, 9), (17, 18), (254, 255)}
    assert fired[(0, 132)][0] >= 1 and fired[(0, 160)][1] >= 1
    dec, inc = LC.searched_ramps()
    assert len(set(dec + inc + LC.RAMPS_FIXED)) == 15
    assert all(fired[r][0] >= 1 for r in dec) and all(fired[r][1] >= 1 for r in inc)
    assert len({lo for lo, _ in dec}) == 5 and len({lo for lo, _ in inc}) == 5
    # a hist_bin without its two steps would count these frames otherwise
    for r in dec + inc + ((0, 132), (0, 160)):
        g = LC.luma(LC.grey_ramp(*r)).ravel()
        naive = np.clip((((g - g.min()) / (g.max() - g.min())) * 256.0).astype(np.int64), 0, 255)
        assert not np.array_equal(np.bincount(naive, minlength=256), LC.hist_luma(g)), r
    assert sum(LC.ties(LC.luma(f)) for f in LC.ramps()) >= 100


def test_planted_frames_lose_every_base_byte_with_a_lost_extreme():
    npx = 131072
    assert LC.planted_positions(npx) == [0, 63, 64, 255, 256, 131071]
    assert LC.planted_positions(131073) == [0, 63, 64, 255, 256, 131071, 131072]
    assert LC.planted_positions(262145) == [0, 63, 64, 255, 256, 131071, 131072, 262144]
    assert [len(LC.planted_pairs(n)) for n in LC.PLANTED_SHAPES] == [30, 42, 56]
    assert all(h * w == n for n, (h, w) in LC.PLANTED_SHAPES.items())
    a, b = 131071, 64
    f = LC.planted(npx, a, b)
    g = LC.luma(f).ravel()
    base = np.ones(npx, bool)
    base[[a, b]] = False
    full = LC.condition_luma(g)
    assert (full[base] == 95).all() and full[a] == 0 and full[b] == 248
    no_min, no_max = g.copy(), g.copy()
    no_min[a] = g[0]
    no_max[b] = g[0]
    assert (LC.condition_luma(no_min)[base] != full[base]).all() and (LC.condition_luma(no_max)[base] != full[base]).all()
    assert LC.hist_luma(g).sum() == npx and LC.hist_luma(g)[0] == 1 and LC.hist_luma(g)[255] == 1


def test_sizes_hold_every_echo_tail():
    calls = LC.sizes_calls()
    assert {v[0].size // 3 for v in calls.values()} == {1, 63, 64, 65, 255, 256, 257, 1021}
    assert {(v.size // 3) % 4 for v in calls.values()} == {0, 1, 2, 3}
    assert f"5x{LC.SIZES_REVERSED[0]}x{LC.SIZES_REVERSED[1]}" in calls
    assert LC.threshold(LC.two_valued()).tolist() == [LC.TWO_VALUED_THRESHOLD] * 2


def test_the_matmul_twin_differs_from_the_plain_order_on_this_host(capsys):
    """frames.rgb2gray is `a @ coeffs`: its summation order belongs to the host's BLAS.  The counts are printed, not asserted (DESIGN.md
    section 9, row a1 records the ones of the machine this was written on: 2,460,884 triples, 70 conditioned bytes in 38 frames)."""
    from tee_optical_flow_amd.frames import condition_frames, rgb2gray
    cube = LC.cube_frames()
    plain, twin = LC.luma(cube), rgb2gray(cube)
    ulp = np.abs(plain.view(np.int64) - twin.view(np.int64))
    a, b = LC.condition(cube), condition_frames(cube)
    with capsys.disabled():
        print(f"\nplain order vs frames.rgb2gray (numpy {np.__version__}): {int((ulp != 0).sum())} of 2^24 triples differ, by at most "
              f"{int(ulp.max())} ulp; conditioned bytes of cube_frames: {int((a != b).sum())} differ in {int((a != b).any((1, 2)).sum())} frames")
    assert int(np.abs(a.astype(int) - b.astype(int)).max()) <= 1  # whatever the order, a byte moves by one count at the most
