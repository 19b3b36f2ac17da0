#!/usr/bin/env python3
"""The area detector's per-frame series of one 65-frame study, area_series(ds, label) (AreaDetector.detect's skimage label +
regionprops loop, cardiac_cycle_detection.py:159-172): on the host (the scipy twin of this repository: NOT the reference's skimage
call, which is not installed here) against the device (tf_first_region_areas, host uint8 masks in, host int64 out, transfers
included), at 512x512 and 600x800.  The mask is a drifting ellipse plus speckle pixels, some of them ahead of the ellipse in raster
order.  Alternates the two after a warm-up, takes the median of --reps, checks that the series are identical, and times
DenseFlow.first_region_areas on its own (the call alone, without area_series' Python around it).  Writes the lines to --out.
    python tools/area_series_bench.py [--reps 5] [--out profiles/r14_area_series.txt]"""
import argparse
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_mask(seed, N, H, W):
    """uint8 [N,H,W,2]: an ellipse that drifts, speckle pixels at 0.05 %, two empty frames"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((N, H, W), np.uint8)
    for f in range(N):
        m[f] = ((yy - H / 2 - 0.5 * f) / (0.3 * H)) ** 2 + ((xx - W / 2 + 0.5 * f) / (0.35 * W)) ** 2 < 1
        if f % 3:
            m[f] |= rng.random((H, W)) < 0.0005
    m[N // 2] = 0
    m[N - 1] = 0
    return np.stack([m, m], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_area_series.txt"))
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    logging.getLogger("tee_optical_flow_amd.analysis").setLevel(logging.ERROR)      # the two empty frames' warnings, on both paths
    eng = T.DenseFlow(device_id=0)
    lines = ["# tools/area_series_bench.py: area_series(ds, label), host (scipy twin of this repository) vs device "
             "(tf_first_region_areas, host uint8 masks in, host int64 out, transfers included)"]
    for H, W in ((512, 512), (600, 800)):
        mask = make_mask(a.frames + H + W, a.frames, H, W)
        st = T.FlowStudy(np.zeros((a.frames, 1, 1, 2), np.float16), {"rv": mask}, 50.0, nframes=a.frames)
        T.area_series(T.FlowStudy(np.zeros((4, 1, 1, 2), np.float16), {"rv": mask[:4]}, 50.0, nframes=4), "rv")   # warm-up of both
        T.area_series(st, "rv", engine=eng)
        th, td, tc, equal = [], [], [], True
        for _ in range(a.reps):
            t = time.perf_counter(); h = T.area_series(st, "rv"); th.append(time.perf_counter() - t)
            t = time.perf_counter(); d = T.area_series(st, "rv", engine=eng); td.append(time.perf_counter() - t)
            t = time.perf_counter(); eng.first_region_areas(mask); tc.append(time.perf_counter() - t)
            equal = equal and np.array_equal(h, d)
        mh, md, mc = (float(np.median(x)) * 1e3 for x in (th, td, tc))
        first = int(np.sum(h != np.array([int(np.count_nonzero(mask[i, :, :, 0])) for i in range(a.frames)])))
        lines.append(f"  {a.frames}x{H}x{W}: host {mh:8.1f} ms ({min(th) * 1e3:.1f}-{max(th) * 1e3:.1f}; {mh / a.frames:.2f} ms per frame)  "
                     f"device {md:7.2f} ms ({min(td) * 1e3:.2f}-{max(td) * 1e3:.2f})  the call alone {mc:7.2f} ms  speed-up {mh / md:6.1f}x  "
                     f"frames whose first region is not the whole mask {first}  identical {bool(equal)}  (median of {a.reps})")
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
