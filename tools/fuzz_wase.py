#!/usr/bin/env python3
"""Randomised parity of the device WASE compensation (tf_wase_compensate, tf_wase_compensate_device: csrc/teeflow_wase.hip.h) with
numpy itself, `(flow - np.mean(masked[masked != 0])) * float32(scale)`: backgrounds and compensated flows bit for bit.

A case draws n_flows in 1..70 (beyond the host entry's chunk of 64), n_frames, H, W with n_frames * 2HW <= 2^20 and
n_flows * n_frames * 2HW <= 2^22 (what bounds the numpy side), shapes biased towards 2HW near multiples of 8, 2048 and 8192 (the leaf
width, the compaction chunk, numpy's piece) and towards n_frames * ceil(2HW / 2048) near multiples of 1024 (a pass of the scan), a mask
density per frame in [0, 1], a zero fraction of the flow in [0, 0.99], the scale, the entry (host pointers, or torch device tensors)
and a data family: normal, six decades of magnitude, subnormal, near FLT_MAX, non-finite.

No case is skipped.  Only the non-finite family (inf, nan, sums that overflow; exactly every tenth case) is compared by NaN position
with bits elsewhere; every other case has a non-empty selection and a finite numpy background and is compared by bits alone.  Both
conditions are asserted on the whole draw before the GPU is touched.  Stops at the first mismatch and prints how to run that case
alone; never retries.

usage: python tools/fuzz_wase.py [cases] [seed] [only] [--host]
  only:   run just that case number of the same draw
  --host: no GPU: the same draw, numpy's np.mean against numpy_order_mean (tests/test_wase_cpu.py, the order the kernels implement) on
          every flow's selection; prints the family counts"""
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = ("normal", "six_decades", "subnormal", "near_flt_max")       # compared by bits alone
NON_FINITE = "non_finite"                                               # compared by NaN position, bits elsewhere
MAX_FRAME_ELEMS, MAX_ELEMS = 1 << 20, 1 << 22
FLT_MAX = float(np.finfo(np.float32).max)


def family_of(seed, c):
    """Every tenth case is non-finite, so at most cases // 10 of any run are."""
    if c % 10 == 9:
        return NON_FINITE
    return FAMILIES[int(np.random.default_rng([seed, c, 1]).integers(0, len(FAMILIES)))]


def _near(rng, base, hi):
    """A value in [1, hi] within 3 of a multiple of base."""
    m = int(rng.integers(1, max(hi // base, 1) + 1))
    return int(min(max(m * base + int(rng.integers(-3, 4)), 1), hi))


def _shape(rng):
    kind = int(rng.integers(0, 6))
    if kind == 5:                                                        # table of block counts near a multiple of 1024, one chunk per frame
        N = int(rng.integers(1, 4)) * 1024 + int(rng.integers(-2, 3))
        hw2 = 2 * int(rng.integers(1, MAX_FRAME_ELEMS // N // 2 + 1))
    else:
        N = int(rng.choice([1, 1, 2, 3, 5, 17, 65, int(rng.integers(1, 130))]))
        hi = MAX_FRAME_ELEMS // N
        hw2 = (int(rng.integers(2, 400)), _near(rng, 8, min(hi, 1200)), _near(rng, 2048, hi), _near(rng, 8192, hi),
               int(rng.integers(2, hi + 1)))[kind]
    hw = max(hw2 // 2, 1)
    H = int(rng.choice([1, 1, 2, 3, 4, 8, 16, int(rng.integers(1, 65))]))
    H = min(H, hw)
    W = max(hw // H, 1)
    return N, H, W


def draw(seed, c):
    """-> dict(family, flows [P,H,W,2] float32, mask [N,H,W,2] bool, scale, entry)"""
    family = family_of(seed, c)
    rng = np.random.default_rng([seed, c])
    N, H, W = _shape(rng)
    hw2 = 2 * H * W
    assert N * hw2 <= MAX_FRAME_ELEMS
    pmax = min(70, MAX_ELEMS // (N * hw2))
    P = int(rng.integers(max(pmax - 5, 1), pmax + 1)) if rng.random() < 0.3 else int(rng.integers(1, pmax + 1))
    dens = rng.random(N)
    dens[rng.random(N) < 0.15] = 0.0
    dens[rng.random(N) < 0.15] = 1.0
    mask = rng.random((N, H, W, 2)) < dens[:, None, None, None]
    zero = rng.random(P) * 0.99
    shape = (P, H, W, 2)
    if family == "normal":
        flows = rng.standard_normal(shape) * 3
    elif family == "subnormal":
        flows = rng.integers(-71362, 71363, shape) * 2.0 ** -149                    # |f| <= 1e-40
        if rng.random() < 0.5:
            flows = np.where(rng.random(shape) < 0.5, flows, rng.standard_normal(shape) * 1e-3)
    else:
        flows = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)
    flows = flows.astype(np.float32)
    flows[rng.random(shape) < zero[:, None, None, None]] = 0.0
    if rng.random() < 0.3:
        flows[rng.random(shape) < 0.05] = -0.0
    if family == NON_FINITE:
        if rng.random() < 0.4:                                                      # sums that overflow
            flows = np.where(flows != 0, np.float32(3e38) * np.sign(flows), flows).astype(np.float32)
        else:
            for v in (np.inf, -np.inf, np.nan):
                k = int(rng.integers(0, 3))
                flows.reshape(-1)[rng.integers(0, flows.size, k)] = v
    else:
        # a non-empty selection for every flow: one place that is non-zero in the flow and True in some frame
        for p in range(P):
            at = (int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(0, 2)))
            if flows[p][at] == 0:
                flows[p][at] = np.float32(2.0 ** -149) if family == "subnormal" else np.float32(0.375)
            mask[(int(rng.integers(0, N)),) + at] = True
        if family == "near_flt_max":
            # as large as the count of selected terms allows: no sum of them, in any order, passes 0.99 FLT_MAX
            for p in range(P):
                cnt = int((mask & (flows[p] != 0)[None]).sum())
                mag = rng.uniform(0.5, 1.0, (H, W, 2)) * (0.99 * FLT_MAX / cnt)
                flows[p] = np.where(flows[p] != 0, np.sign(flows[p]) * mag, flows[p]).astype(np.float32)
    scale = float(np.float32(rng.choice([1.0, 1.0, 2.5, 0.04 * 50.0, -1.0, rng.uniform(0.1, 10.0)])))
    entry = "device" if rng.random() < 0.4 else "host"
    return dict(family=family, flows=np.ascontiguousarray(flows, np.float32), mask=np.ascontiguousarray(mask), scale=scale, entry=entry)


def describe(case):
    P, H, W, _ = case["flows"].shape
    return f"{case['family']} {P} flows x {case['mask'].shape[0]} frames of {H}x{W}, scale {case['scale']!r}, {case['entry']} entry"


def selections(case):
    """masked[masked != 0] of every flow, as numpy builds it."""
    for f in case["flows"]:
        masked = f * case["mask"]
        yield masked[masked != 0]


def numpy_backgrounds(case):
    return np.array([np.mean(a) for a in selections(case)], np.float32)


def same(got, ref, nan_ok):
    got = np.ascontiguousarray(got, np.float32).reshape(-1)
    ref = np.ascontiguousarray(ref, np.float32).reshape(-1)
    if nan_ok:
        gn, rn = np.isnan(got), np.isnan(ref)
        if not np.array_equal(gn, rn):
            return f"NaN at {np.flatnonzero(gn)[:4]} (device) vs {np.flatnonzero(rn)[:4]} (numpy)"
        got, ref = got[~gn], ref[~rn]
    if got.tobytes() != ref.tobytes():
        bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
        return f"{bad.size} of {got.size} differ, first at {bad[0]}: device {got[bad[0]]!r}, numpy {ref[bad[0]]!r}"
    return None


def main():
    args = [a for a in sys.argv[1:] if a != "--host"]
    host_only = "--host" in sys.argv[1:]
    cases = int(args[0]) if len(args) > 0 else 30
    seed = int(args[1]) if len(args) > 1 else 0
    only = int(args[2]) if len(args) > 2 else None
    if cases < 1 or (only is not None and not 0 <= only < cases):
        sys.exit(f"{__doc__}\n\ncases must be at least 1 and only in 0 .. cases - 1, got cases {cases}, only {only}")
    todo = list(range(cases)) if only is None else [only]
    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    t0 = time.time()

    # ---- the draw is judged first, on the host alone
    fams = [family_of(seed, c) for c in range(cases)]
    assert sum(f == NON_FINITE for f in fams) * 10 <= cases, "more than one case in ten is compared by NaN position"
    if host_only:
        from tests.test_wase_cpu import numpy_order_mean
    ref_bg = {}
    for c in todo:
        case = draw(seed, c)
        assert case["family"] == fams[c]
        P, H, W, _ = case["flows"].shape
        N = case["mask"].shape[0]
        assert 1 <= P <= 70 and N * 2 * H * W <= MAX_FRAME_ELEMS and P * N * 2 * H * W <= MAX_ELEMS and case["scale"] != 0
        ref_bg[c] = numpy_backgrounds(case)
        if case["family"] != NON_FINITE:
            assert np.isfinite(ref_bg[c]).all(), f"case {c} ({describe(case)}): numpy's background is not finite: {ref_bg[c]}"
        if host_only:
            for p, a in enumerate(selections(case)):
                want = numpy_order_mean(a)
                if want.tobytes() == ref_bg[c][p].tobytes() or (case["family"] == NON_FINITE and np.isnan(want) and np.isnan(ref_bg[c][p])):
                    continue
                print(f"MISMATCH case {c} (seed {seed}): {describe(case)}\n  flow {p}, {len(a)} terms: np.mean {ref_bg[c][p]!r}, restated order {want!r}"
                      f"\n  rerun alone: python tools/fuzz_wase.py {cases} {seed} {c} --host", flush=True)
                sys.exit(1)
            print(f"case {c}: {describe(case)} ok", flush=True)
    if host_only:
        count = {f: fams.count(f) for f in FAMILIES + (NON_FINITE,)}
        print(f"{len(todo)}/{len(todo)} cases identical in {time.time() - t0:.0f} s (np.mean against its restated order; families of the {cases}: {count})")
        return

    # ---- the device
    import torch                                                                    # before the engine's library: one HIP runtime for both
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import _lib
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    eng = T.DenseFlow(device_id=0)
    L = _lib.load()
    t1 = time.time()
    done = 0
    for c in todo:
        case = draw(seed, c)
        flows, mask, scale = case["flows"], case["mask"], case["scale"]
        P, H, W, _ = flows.shape
        want_bg = ref_bg.pop(c)
        ref = np.stack([(f - b) * np.float32(scale) for f, b in zip(flows, want_bg)])
        if case["entry"] == "host":
            out, bg = eng.wase_compensate(flows, mask, scale=scale)
        else:
            df = torch.from_numpy(flows).to(dev)
            dm = torch.from_numpy(mask.view(np.uint8)).to(dev)
            torch.cuda.synchronize()
            bg = np.empty(P, np.float32)
            _lib.check(L.tf_wase_compensate_device(eng._h, df.data_ptr(), P, dm.data_ptr(), mask.shape[0], H, W, scale, bg.ctypes.data),
                       eng._h, "tf_wase_compensate_device")
            out = df.cpu().numpy()
        nan_ok = case["family"] == NON_FINITE
        err = same(bg, want_bg, nan_ok)
        err = f"backgrounds: {err}" if err else same(out, ref, nan_ok)
        if err:
            print(f"MISMATCH case {c} (seed {seed}): {describe(case)}\n  {err}\n  rerun alone: python tools/fuzz_wase.py {cases} {seed} {c}", flush=True)
            eng.close()
            sys.exit(1)
        done += 1
        print(f"case {c}: {describe(case)} ok", flush=True)
    eng.close()
    print(f"{done}/{done} cases identical in {time.time() - t1:.0f} s on the device, {t1 - t0:.0f} s before it")


if __name__ == "__main__":
    main()
