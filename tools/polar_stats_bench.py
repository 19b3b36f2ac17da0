#!/usr/bin/env python3
"""The consumer's polar steps of one 65-frame study, calculate_3dhist(ds, param, label) and angle_mode_series(ds, param, label) (the
angle detector's per-frame mode) for velocity, acceleration and PWR of one label: on the host (the numpy twin, cart_to_polar standing
in for cv2.cartToPolar, which is not installed: NOT a speed-up over the reference's cv2 call) against the device
(tf_polar_project_param + tf_radlong_hist / _select, host arrays in and out, transfers included), at 512x512 and 600x800, float16 flow
as the study file holds it.  Alternates the two after a warm-up and checks bit-equality.  Prints one JSON line (and writes it to
--out when given).
    python tools/polar_stats_bench.py [--reps 3] [--out profiles/r08_polar_stats.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_study(seed, N, H, W):
    """speckle flow (float16), an rv disc that drifts"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    flow = rng.normal(0, 4, (N, H, W, 2)).astype(np.float16)
    rv = np.zeros((N, H, W), bool)
    for f in range(N):
        rv[f] = ((yy - H / 2 - f) / (0.35 * H)) ** 2 + ((xx - W / 2 + f) / (0.4 * W)) ** 2 < 1
    return np.stack([rv, rv], -1), flow


def run(study, engine):
    from tee_optical_flow_amd import analysis as A
    return {p: (A.calculate_3dhist(study, p, "rv", engine=engine), A.angle_mode_series(study, p, "rv", engine=engine)) for p in A.PARAMS}


def same(a, b):
    return all(np.array_equal(np.asarray(a[p][0][i]), np.asarray(b[p][0][i])) for p in a for i in range(5)) and \
        all(np.array_equal(a[p][1], b[p][1], equal_nan=True) for p in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    res = {"what": "calculate_3dhist + angle_mode_series x3 params, one label, one study", "frames": a.frames, "reps": a.reps,
           "host": "numpy twin (cv2 absent): not the reference's cv2 path", "sizes": {}}
    for H, W in ((512, 512), (600, 800)):
        rv, flow = make_study(a.frames + H + W, a.frames, H, W)
        st = T.FlowStudy(flow, {"rv": rv}, np.float64(50.0))
        run(T.FlowStudy(flow[:4], {"rv": rv[:4]}, np.float64(50.0), nframes=2), None)          # warm-up of both
        run(st, eng)
        th, td, equal = [], [], True
        for _ in range(a.reps):
            t = time.perf_counter(); h = run(st, None); th.append(time.perf_counter() - t)
            t = time.perf_counter(); d = run(st, eng); td.append(time.perf_counter() - t)
            equal = equal and same(h, d)
        mh, md = float(np.median(th)) * 1e3, float(np.median(td)) * 1e3
        res["sizes"][f"{H}x{W}"] = {"host_ms": round(mh, 1), "device_ms": round(md, 1), "device_ms_min": round(min(td) * 1e3, 1),
                                    "device_ms_max": round(max(td) * 1e3, 1), "speedup": round(mh / md, 1), "bit_equal": bool(equal)}
    eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
