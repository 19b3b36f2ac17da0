"""WASE background compensation on the device against numpy's own np.mean -- bit for bit."""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _host(flows, mask):
    from tee_optical_flow_amd.pipeline import wase_background
    bg = np.array([wase_background(f, mask) for f in flows], np.float32)
    return np.stack([f - b for f, b in zip(flows, bg)]), bg


@pytest.mark.parametrize("shape", [(3, 5, 24, 40), (2, 9, 64, 64), (4, 33, 97, 131), (1, 2, 3, 5), (2, 40, 128, 128)])
def test_wase_matches_numpy_mean_bitwise(engine, shape):
    P, N, H, W = shape
    rng = np.random.default_rng(P * 1000 + N)
    flows = (rng.standard_normal((P, H, W, 2)) * 3).astype(np.float32)
    flows[:, : H // 4, : W // 3] = 0.0                       # exact zeros never count
    flows[0, -1, -1] = -0.0
    mask = rng.random((N, H, W, 2)) < 0.37
    mask[0] = False
    ref, ref_bg = _host(flows, mask)
    out, bg = engine.wase_compensate(flows, mask)
    assert bg.tobytes() == ref_bg.tobytes(), (bg, ref_bg)
    assert np.ascontiguousarray(out).view(np.uint32).tobytes() == np.ascontiguousarray(ref).view(np.uint32).tobytes()


def test_wase_scale_empty_selection_and_sizes_across_numpy_pieces(engine):
    rng = np.random.default_rng(77)
    P, N, H, W = 3, 3, 64, 65
    flows = rng.standard_normal((P, H, W, 2)).astype(np.float32)
    mask = np.zeros((N, H, W, 2), bool)
    # selections of 0, 1, 7, 8, 129, 8191, 8192, 8193 and 20000 terms exercise every branch of the summation order
    for p, k in enumerate([0, 8193, 20000]):
        m = np.zeros(N * H * W * 2, bool)
        m[rng.choice(m.size, k, replace=False)] = True
        mk = m.reshape(N, H, W, 2)
        import warnings
        with warnings.catch_warnings(), np.errstate(invalid="ignore"):
            warnings.simplefilter("ignore")
            ref, ref_bg = _host(flows[p:p + 1], mk)
        out, bg = engine.wase_compensate(flows[p:p + 1], mk, scale=2.5)
        if k == 0:                                            # np.mean of an empty selection: nan (its sign bit is the host FPU's)
            assert np.isnan(bg[0]) and np.isnan(ref_bg[0]) and np.isnan(out).all()
            continue
        assert bg.tobytes() == ref_bg.tobytes(), (k, bg, ref_bg)
        assert np.array_equal(out, ref * np.float32(2.5))
    for k in (1, 7, 8, 129, 8191, 8192):
        m = np.zeros(N * H * W * 2, bool)
        m[rng.choice(m.size, k, replace=False)] = True
        mk = m.reshape(N, H, W, 2)
        _, ref_bg = _host(flows[:1], mk)
        _, bg = engine.wase_compensate(flows[:1], mk)
        assert bg.tobytes() == ref_bg.tobytes(), (k, bg, ref_bg)


def test_flow_for_study_wase_device_equals_host_path(engine):
    from tee_optical_flow_amd.pipeline import flow_for_study, _compensate
    from tee_optical_flow_amd.synth import speckle_sequence
    fr = speckle_sequence(5, 6, 48, 64)
    rng = np.random.default_rng(3)
    mask = {"bkgd": rng.random((6, 48, 64, 2)) < 0.5}
    dev = flow_for_study(fr, engine, mask_dict=mask, bkgd_comp="WASE", conversion_factor=0.04 * 50.0)
    flows = engine.calc_batch(fr)
    host = np.stack([_compensate(f, mask, "WASE") for f in flows])
    host = np.concatenate([host, host[-1:]]) * (0.04 * 50.0)
    assert np.array_equal(dev, host)


# ---- the paths of the kernels that a real study takes: scan passes, piece lengths, apply stride, value classes, both entries ----------
# The reference is numpy itself, (flow - np.mean(masked[masked != 0])) * float32(scale); every comparison is of bits.  Data spans six
# decades of magnitude, so that an element summed at another place of numpy's order changes the bits of the sum.

def _six_decades(rng, shape):
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)


def _numpy(flows, mask, scale=1.0):
    from tee_optical_flow_amd.pipeline import wase_background
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        bg = np.array([wase_background(f, mask) for f in flows], np.float32)
        out = np.stack([(f - b) * np.float32(scale) for f, b in zip(flows, bg)])
    return out, bg


def _assert_identical(got, ref, what, nan_ok=False):
    """Bit for bit.  nan_ok: NaNs must sit at the same places, their sign and payload are the FPU's own (host and GPU differ)."""
    got = np.ascontiguousarray(got, np.float32).reshape(-1)
    ref = np.ascontiguousarray(ref, np.float32).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if nan_ok:
        gn, rn = np.isnan(got), np.isnan(ref)
        assert np.array_equal(gn, rn), f"{what}: NaN at {np.flatnonzero(gn)[:5]} on the device, at {np.flatnonzero(rn)[:5]} in numpy"
        got, ref = got[~gn], ref[~rn]
    if got.tobytes() != ref.tobytes():
        bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: device {got[bad[0]]!r} "
                             f"({got.view(np.uint32)[bad[0]]:#010x}), numpy {ref[bad[0]]!r} ({ref.view(np.uint32)[bad[0]]:#010x})")


def _check(engine, flows, mask, scale=1.0, nan_ok=False, what=""):
    ref, ref_bg = _numpy(flows, mask, scale)
    out, bg = engine.wase_compensate(flows, mask, scale=scale)
    _assert_identical(bg, ref_bg, f"{what} backgrounds", nan_ok)
    _assert_identical(out, ref, f"{what} compensated flows", nan_ok)
    return bg, ref_bg


def _scan_case(n_frames, H, W, edge):
    """Two flows over n_frames masks of differing density; the frames that hold the table entries on either side of every multiple
    of 1024 (where k_wase_scan hands its carry to the next pass, and where it takes the total) are all False or all True."""
    rng = np.random.default_rng([n_frames, H, W, int(edge)])
    chunks = -(-2 * H * W // 2048)
    mask = rng.random((n_frames, H, W, 2)) < rng.random(n_frames)[:, None, None, None]
    for b in range(1024, n_frames * chunks + 1, 1024):
        for fr in {(b - 1) // chunks, b // chunks}:
            if fr < n_frames:
                mask[fr] = edge
    flows = _six_decades(rng, (2, H, W, 2))
    flows[0][rng.random((H, W, 2)) < 0.3] = 0.0
    flows[1, : H // 2, : W // 3] = 0.0
    flows[1, -1, -1, 0] = -0.0
    return flows, mask


@pytest.mark.parametrize("n_frames,H,W", [(1023, 4, 4), (1024, 4, 4), (1025, 4, 4), (2048, 4, 4), (2049, 4, 4), (3000, 4, 4),
                                          (341, 16, 130), (342, 16, 130), (700, 16, 130)])
def test_scan_carries_across_passes_of_1024_block_counts(engine, n_frames, H, W):
    """n_frames x ceil(2HW / 2048) block counts: 1023 ... 3000 with one chunk per frame, 1023, 1026 and 2100 with three (the last of
    64 elements)."""
    for edge in (False, True):
        flows, mask = _scan_case(n_frames, H, W, edge)
        _check(engine, flows, mask, what=f"{n_frames} frames of {H}x{W}, boundary frames all {edge}:")


def _sparse_flows(rng, ks, H, W):
    """Flow p: exactly ks[p] non-zero values at random places, exact zeros elsewhere."""
    flows = np.zeros((len(ks), H * W * 2), np.float32)
    for p, k in enumerate(ks):
        v = _six_decades(rng, k)
        v[v == 0] = 1.0
        flows[p, rng.choice(H * W * 2, k, replace=False)] = v
    assert [(f != 0).sum() for f in flows] == list(ks)
    return flows.reshape(len(ks), H, W, 2)


def test_piece_lengths_within_one_piece_and_flow_chunks_of_64(engine):
    """2HW = 8192 under an all-True mask: the selection of flow p is one piece of exactly k_p elements, so thread 0's two tree walks
    and the leaf groups see every length listed above.  386 flows are also six full chunks of 64 of the host entry and one of 2."""
    from tests.test_wase_cpu import piece_lengths
    ks = piece_lengths()
    flows = _sparse_flows(np.random.default_rng(64), ks, 64, 64)
    mask = np.ones((1, 64, 64, 2), bool)
    ref, ref_bg = _numpy(flows, mask)
    out, bg = engine.wase_compensate(flows, mask)
    for p, k in enumerate(ks):                                   # name the length that broke
        assert bg[p].tobytes() == ref_bg[p].tobytes(), f"flow {p}, piece of {k} elements: device {bg[p]!r}, numpy {ref_bg[p]!r}"
    _assert_identical(out, ref, "compensated flows")


@pytest.mark.parametrize("W", [129, 200])
def test_several_pieces_and_their_last_piece(engine, W):
    """2HW = 2*8192 + 128 and 3*8192 + 1024: selections of 8192 j + r elements, a running total over j full pieces and a last one of r."""
    hw2 = 64 * W * 2
    from tests.test_wase_cpu import MULTI_PIECE_LENGTHS
    ks = [k for k in MULTI_PIECE_LENGTHS if k <= hw2]
    assert len(ks) == (15 if W == 129 else 24)
    flows = _sparse_flows(np.random.default_rng(W), ks, 64, W)
    mask = np.ones((1, 64, W, 2), bool)
    ref, ref_bg = _numpy(flows, mask)
    out, bg = engine.wase_compensate(flows, mask)
    for p, k in enumerate(ks):
        assert bg[p].tobytes() == ref_bg[p].tobytes(), f"flow {p}, {k} elements: device {bg[p]!r}, numpy {ref_bg[p]!r}"
    _assert_identical(out, ref, "compensated flows")


def test_apply_pass_strides_over_a_plane_above_its_grid(engine):
    """2HW = 270 000 is more than the 1024 x 256 elements one sweep of k_wase_apply's grid covers, and no multiple of 256."""
    rng = np.random.default_rng(300450)
    flows = _six_decades(rng, (2, 300, 450, 2))
    flows[1][rng.random((300, 450, 2)) < 0.5] = 0.0
    mask = rng.random((1, 300, 450, 2)) < 0.4
    _check(engine, flows, mask, scale=2.5)


VN, VH, VW = 3, 24, 40                                           # the value-class cases


def test_subnormal_flows_are_counted_and_stay_subnormal(engine):
    rng = np.random.default_rng(40)
    tiny = np.float32(2.0 ** -149)
    sub = (rng.integers(1, 71362, (VH, VW, 2)) * tiny).astype(np.float32)          # 0 < f <= 1e-40
    assert sub.max() <= np.float32(1e-40) and (sub > 0).all()
    signed = sub * rng.choice(np.float32([-1, 1]), sub.shape)
    mixed = np.where(rng.random(sub.shape) < 0.5, signed, _six_decades(rng, sub.shape))
    flows = np.stack([sub, signed, mixed]).astype(np.float32)
    flows[:, :5, :7] = 0.0
    mask = rng.random((VN, VH, VW, 2)) < 0.5
    bg, ref_bg = _check(engine, flows, mask)
    assert 0 < ref_bg[0] < np.finfo(np.float32).tiny and 0 < bg[0] < np.finfo(np.float32).tiny
    _check(engine, flows, mask, scale=0.5)


def test_negative_zeros_are_never_counted(engine):
    rng = np.random.default_rng(41)
    flows = _six_decades(rng, (2, VH, VW, 2))
    u = rng.random(flows.shape)
    flows[u < 0.4] = -0.0
    flows[u > 0.9] = 0.0
    flows[1] = -0.0
    flows[1, 3, 4, 1] = 7.25                                     # one term among negative zeros: the background is that term
    mask = rng.random((VN, VH, VW, 2)) < 0.5
    mask[:, 3, 4, 1] = True
    bg, ref_bg = _check(engine, flows, mask)
    assert ref_bg[1] == np.float32(7.25)


def test_inf_under_true_masks_gives_an_inf_background(engine):
    rng = np.random.default_rng(42)
    flows = _six_decades(rng, (1, VH, VW, 2))
    flows[0, 10, 20, 1] = np.inf
    mask = rng.random((VN, VH, VW, 2)) < 0.5
    mask[:, 10, 20, 1] = True
    ref, ref_bg = _numpy(flows, mask)
    out, bg = engine.wase_compensate(flows, mask)
    assert ref_bg[0] == np.inf and bg.tobytes() == ref_bg.tobytes(), (bg, ref_bg)
    _assert_identical(out, ref, "compensated flows", nan_ok=True)      # inf - inf at the one place


@pytest.mark.parametrize("value", [np.inf, np.nan])
@pytest.mark.parametrize("column", ["one frame False", "all frames False"])
def test_non_finite_flow_times_a_false_mask_is_nan_and_counted(engine, value, column):
    """inf * 0 and nan * 0 are NaN, and NaN != 0: the term is selected whatever the mask says, as in numpy."""
    rng = np.random.default_rng(43)
    flows = _six_decades(rng, (2, VH, VW, 2))
    flows[0, 7, 31, 0] = value
    mask = rng.random((VN, VH, VW, 2)) < 0.5
    mask[:, 7, 31, 0] = True
    mask[1 if column == "one frame False" else slice(None), 7, 31, 0] = False
    ref, ref_bg = _numpy(flows, mask)
    out, bg = engine.wase_compensate(flows, mask)
    assert np.isnan(ref_bg[0]) and np.isnan(bg[0]), (bg, ref_bg)
    assert np.isfinite(ref_bg[1]) and bg[1].tobytes() == ref_bg[1].tobytes(), (bg, ref_bg)   # the flow beside it is untouched
    _assert_identical(out, ref, "compensated flows", nan_ok=True)


def test_partial_sums_that_overflow(engine):
    rng = np.random.default_rng(44)
    big = np.float32(3e38)
    flows = np.stack([big * rng.choice(np.float32([-1, 1]), (VH, VW, 2)), np.full((VH, VW, 2), big)]).astype(np.float32)
    flows[:, :3] = 0.0
    mask = rng.random((VN, VH, VW, 2)) < 0.5
    ref, ref_bg = _numpy(flows, mask)
    assert not np.isfinite(ref_bg).any() and ref_bg[1] == np.inf
    out, bg = engine.wase_compensate(flows, mask)
    _assert_identical(bg, ref_bg, "backgrounds", nan_ok=True)
    _assert_identical(out, ref, "compensated flows", nan_ok=True)


def test_bad_arguments_are_refused_by_both_entries_and_the_handle_goes_on(engine):
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(45)
    H, W = 6, 5
    flows = _six_decades(rng, (2, H, W, 2))
    mask = rng.random((2, H, W, 2)) < 0.6
    # pinned host memory, which the device can read too: neither entry may touch it in a refused call, and nothing faults if one does
    pf, pm = L.tf_host_alloc(flows.nbytes), L.tf_host_alloc(mask.size)
    assert pf and pm
    try:
        C.memmove(pf, flows.ctypes.data, flows.nbytes)
        C.memmove(pm, mask.ctypes.data, mask.size)
        bad = {"n_flows=0": (pf, 0, pm, 2, H, W), "n_frames=0": (pf, 2, pm, 0, H, W), "H=0": (pf, 2, pm, 2, 0, W), "null mask": (pf, 2, None, 2, H, W)}
        for entry in ("tf_wase_compensate", "tf_wase_compensate_device"):
            for name, (f, P, m, N, h_, w_) in bad.items():
                assert L.tf_set_tuning(engine._h, b"no_such_knob", 0) == _lib.TF_ERR_INVALID_ARG      # another message first
                assert b"knob" in L.tf_last_error(engine._h)
                bg = np.full(2, 5.0, np.float32)
                assert getattr(L, entry)(engine._h, f, P, m, N, h_, w_, 1.0, bg.ctypes.data) == _lib.TF_ERR_INVALID_ARG, (entry, name)
                msg = L.tf_last_error(engine._h)
                assert msg and b"wase" in msg, (entry, name, msg)
                assert (bg == 5.0).all() and C.string_at(pf, flows.nbytes) == flows.tobytes(), (entry, name)
                _check(engine, flows, mask, what=f"after {entry} with {name}:")
    finally:
        L.tf_host_free(pf)
        L.tf_host_free(pm)


def device_entry_cases():
    flows, mask = _scan_case(342, 16, 130, True)
    ks = [8192 * j + r for j in (1, 2) for r in (0, 1, 7, 8, 9, 127, 128)]
    return {"scan of 1026 block counts": (flows, mask, 1.0),
            "several pieces, 2HW = 16512": (_sparse_flows(np.random.default_rng(129), ks, 64, 129), np.ones((1, 64, 129, 2), bool), 2.5)}


DEVICE_ENTRY = r"""
import sys
import numpy as np, torch
sys.path.insert(0, ROOT)
import tee_optical_flow_amd as T
from tee_optical_flow_amd import _lib
from tests import test_gpu_wase as G
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
eng = T.DenseFlow(device_id=0)
L = _lib.load()
try:
    for name, (flows, mask, scale) in G.device_entry_cases().items():
        P, H, W, _ = flows.shape
        ref, ref_bg = G._numpy(flows, mask, scale)
        host, host_bg = eng.wase_compensate(flows, mask, scale=scale)
        for with_bg in (True, False):
            df = torch.from_numpy(flows).to(dev)
            dm = torch.from_numpy(mask.view(np.uint8)).to(dev)
            torch.cuda.synchronize()
            bg = np.full(P, 12345.0, np.float32)
            _lib.check(L.tf_wase_compensate_device(eng._h, df.data_ptr(), P, dm.data_ptr(), mask.shape[0], H, W, scale,
                                                   bg.ctypes.data if with_bg else None), eng._h, "tf_wase_compensate_device")
            out = df.cpu().numpy()
            G._assert_identical(out, ref, f"{name}: flows in place vs numpy")
            G._assert_identical(out, host, f"{name}: flows in place vs tf_wase_compensate")
            assert np.array_equal(dm.cpu().numpy(), mask.view(np.uint8)), name
            if with_bg:
                G._assert_identical(bg, ref_bg, f"{name}: backgrounds vs numpy")
                G._assert_identical(bg, host_bg, f"{name}: backgrounds vs tf_wase_compensate")
            else:
                assert (bg == 12345.0).all()
finally:
    eng.close()
print("device entry ok")
"""


def test_device_pointer_entry_on_torch_tensors_equals_host_entry_and_numpy():
    """tf_wase_compensate_device through _lib.load() on torch device tensors, with a host background_out and with NULL (a child process
    with torch imported first: the engine and torch must share one HIP runtime, as in test_gpu_queue.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", DEVICE_ENTRY.replace("ROOT", repr(root))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device entry ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
