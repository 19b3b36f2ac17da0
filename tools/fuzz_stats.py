#!/usr/bin/env python3
"""Randomised parity of the device statistics tail (tf_radlong_hist, tf_radlong_select, the angle bins and mode, and their glue in
analysis.py) with plain numpy: draws the path (rad/long float64, polar float32), the param, sizes from 1x1 to 600x800, the frame
count, the mask density, a data family, nbins in 1..10000 and percentiles anywhere in [0, 100], and compares as
tests/test_gpu_stats_tail.py does (tests/stats_cases.py: values, dtypes, shapes, bit for bit).  Where numpy itself raises (an empty
first polar frame, too many bins for the range) the device call must raise the same.  Stops at the first mismatch and prints how to
run that case alone; never retries; an error return from the library ends the run.
usage: python tools/fuzz_stats.py [cases] [seed] [only]      ("only": run just that case number of the same draw)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = ("speckle_f16", "coarse", "axis", "few_values", "sparse", "constant")


def draw(seed, c):
    from tee_optical_flow_amd import analysis as A
    from tests import stats_cases as S
    rng = np.random.default_rng([seed, c])
    path = "radlong" if rng.random() < 0.5 else "polar"
    param = A.PARAMS[int(rng.integers(0, 3))]
    shape = int(rng.integers(0, 4))
    if shape == 0:
        H, W = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    elif shape == 1:
        H, W = (int(rng.integers(1, 3000)), 1) if rng.random() < 0.5 else (1, int(rng.integers(1, 3000)))
    elif shape == 2:
        H, W = int(rng.integers(5, 161)), int(rng.integers(5, 201))
    else:
        H, W = int(rng.integers(161, 601)), int(rng.integers(201, 801))
    n = int(rng.integers(1, 4 if H * W > 100000 else 9))
    extra = int(rng.integers(0, 3))
    if param != "velocity" and n + extra < 2:
        extra = 1
    N = n + extra
    family = FAMILIES[int(rng.integers(0, len(FAMILIES)))]
    if family == "speckle_f16":
        flow = rng.normal(0, 4, (N, H, W, 2)).astype(np.float16)
    elif family == "coarse":
        flow = (np.round(rng.normal(0, 2, (N, H, W, 2)) * 2) / 2).astype(np.float16)
    elif family == "axis":
        flow = np.zeros((N, H, W, 2), np.float16)
        flow[..., int(rng.integers(0, 2))] = rng.integers(-64, 65, (N, H, W)) / 2.0 ** int(rng.integers(0, 6))
    elif family == "few_values":
        vals = (rng.normal(0, 3, (int(rng.integers(1, 5)), 2))).astype(np.float16)
        flow = vals[rng.integers(0, len(vals), (N, H, W))]
    elif family == "sparse":
        flow = (rng.normal(0, 4, (N, H, W, 2)) * (rng.random((N, H, W, 1)) < 3.0 / (H * W) + 0.01)).astype(np.float16)
    else:
        flow = np.broadcast_to(rng.normal(0, 3, 2).astype(np.float16), (N, H, W, 2)).copy()
    if rng.random() < 0.4:
        flow = flow.astype(np.float32)
    C = int(rng.integers(1, 3))
    density = float(rng.choice([1.0, 0.9, 0.5, 0.05]))
    mask = rng.random((N, H, W, 1)) < density
    mask = np.ascontiguousarray(np.repeat(mask, C, axis=3))
    for f in range(n):
        if rng.random() < 0.12:
            mask[f] = False                                                   # an empty frame, the first one included
    if path == "radlong" and W == 1 and rng.random() < 0.5:
        cent = [S.CENT] * n                                                   # the planes are the flow itself
    else:
        cent = [(float(rng.uniform(-2, H + 2)), float(rng.uniform(-2, W + 2))) for _ in range(n)]
    fr = float(rng.uniform(10, 120))
    if rng.random() < 0.5:
        fr = np.float64(fr)
    nbins = int(rng.choice([int(rng.integers(1, 10001)), int(rng.integers(1, 65)), 1000]))
    qs = [float(rng.choice([rng.uniform(0, 100), rng.uniform(0, 100), 0.0, 100.0, 50.0, 99.0, 1.0])) for _ in range(3)]
    return S.Case(f"fuzz_{seed}_{c}_{family}_{H}x{W}", path, flow, mask, n, cent=cent if path == "radlong" else None, frame_rate=fr, param=param,
                  nbins=nbins, perc_lo=qs[0], perc_hi=qs[1], percentile=qs[2])


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    only = int(sys.argv[3]) if len(sys.argv) > 3 else None
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import analysis as A
    from tests import stats_cases as S
    eng = T.DenseFlow(device_id=0)
    t0 = time.time()
    done = 0
    for c in range(cases) if only is None else [only]:
        case = draw(seed, c)
        # what numpy does with the draw decides what the device has to do: the same numbers, or the same exception
        try:
            with np.errstate(all="ignore"):
                if case.path == "radlong":
                    S.host_radlong(case)
                else:
                    A.calculate_3dhist(case.study(), case.param, "m", nbins=case.nbins, percentile=case.percentile)
        except (ValueError, IndexError) as e:
            case.raises = type(e)
        try:
            with np.errstate(all="ignore"):
                (S.check_radlong if case.path == "radlong" else S.check_polar)(eng, case)
        except AssertionError as e:
            print(f"MISMATCH case {c} (seed {seed}): {case!r}\n  {e}\n  rerun alone: python tools/fuzz_stats.py {cases} {seed} {c}", flush=True)
            eng.close()
            sys.exit(1)
        done += 1
        print(f"case {c}: {case!r} ok", flush=True)
    eng.close()
    print(f"{done}/{done} cases identical in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
