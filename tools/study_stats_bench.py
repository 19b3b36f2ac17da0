#!/usr/bin/env python3
"""The consumer's rad/long call of one 65-frame study, calculate_3dhist_radlong(ds, param) for velocity, acceleration and PWR with the
AV centroids computed once and shared: on the host (numpy / scipy, the same work as the reference's numpy / skimage path) against the
device (tf_av_centroids + tf_radlong_project_param + tf_radlong_hist / _select, host arrays in and out, transfers included), at
512x512 and 600x800, float16 flow as the study file holds it.  Alternates the two after a warm-up and checks bit-equality; the
engine's av_centroids call is also timed on its own (centroids_device_ms: it is a small share of device_ms).
Prints one JSON line (and writes it to --out when given).
    python tools/study_stats_bench.py [--reps 3] [--out profiles/r07_study_stats.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_study(seed, N, H, W):
    """speckle flow (float16), an rv disc that drifts, av masks of a few random blobs per frame with specks"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    flow = rng.normal(0, 4, (N, H, W, 2)).astype(np.float16)
    rv = np.zeros((N, H, W), bool)
    av = np.zeros((N, H, W), bool)
    for f in range(N):
        rv[f] = ((yy - H / 2 - f) / (0.35 * H)) ** 2 + ((xx - W / 2 + f) / (0.4 * W)) ** 2 < 1
        for _ in range(3):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            av[f] |= ((yy - cy) / rng.uniform(5, H / 6)) ** 2 + ((xx - cx) / rng.uniform(5, W / 6)) ** 2 < 1
        av[f] ^= rng.random((H, W)) < 0.002
    return np.stack([rv, rv], -1), np.stack([av, av], -1), flow


def run(study, engine):
    from tee_optical_flow_amd import analysis as A
    cent = A.av_centroids(study.get_mask("av"), study.nframes, engine=engine)
    return {p: A.calculate_3dhist_radlong(study, p, engine=engine, centroids=cent) for p in A.PARAMS}


def same(a, b):
    return all(np.array_equal(np.asarray(a[p][c][i]), np.asarray(b[p][c][i])) for p in a for c in ("radial", "longitudinal") for i in range(4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    res = {"what": "calculate_3dhist_radlong x3 params, shared AV centroids, one study", "frames": a.frames, "reps": a.reps, "sizes": {}}
    for H, W in ((512, 512), (600, 800)):
        rv, av, flow = make_study(a.frames + H + W, a.frames, H, W)
        st = T.FlowStudy(flow, {"rv": rv, "av": av}, 50.0)
        run(T.FlowStudy(flow[:4], {"rv": rv[:4], "av": av[:4]}, 50.0, nframes=2), None)          # warm-up of both
        run(st, eng)
        th, td, equal = [], [], True
        for _ in range(a.reps):
            t = time.perf_counter(); h = run(st, None); th.append(time.perf_counter() - t)
            t = time.perf_counter(); d = run(st, eng); td.append(time.perf_counter() - t)
            equal = equal and same(h, d)
        tc = []
        for _ in range(a.reps):
            t = time.perf_counter(); eng.av_centroids(av[:st.nframes]); tc.append(time.perf_counter() - t)
        mh, md = float(np.median(th)) * 1e3, float(np.median(td)) * 1e3
        res["sizes"][f"{H}x{W}"] = {"host_ms": round(mh, 1), "device_ms": round(md, 1), "device_ms_min": round(min(td) * 1e3, 1),
                                    "device_ms_max": round(max(td) * 1e3, 1), "centroids_device_ms": round(float(np.median(tc)) * 1e3, 2), "speedup": round(mh / md, 1), "bit_equal": bool(equal)}
    eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
