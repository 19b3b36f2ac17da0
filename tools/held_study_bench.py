#!/usr/bin/env python3
"""The consumer's whole tail of one 65-frame study -- AV centroids, calculate_3dhist_radlong x 3 params, calculate_3dhist x 3 params for
one label, angle_mode_series, area_series, radlong_overlay -- timed three ways on the study a solve has just made, at 512x512 and
600x800:
    host    the host-pointer calls (FlowStudy + engine): every call uploads its flow, mask and echo again
    held    HeldStudy.from_study, its one upload of flow, echo and masks included, then the same tail on the held arrays
    solved  after calc_study_payload(hold=True) (not timed: the solve is the same work in all three): the masks uploaded once, then the tail
The three are interleaved in one process, median of --reps after a warm-up, results checked bit-equal across the three; upload_mb is what
tail_upload_bytes counted for one tail.  Prints one JSON line per size (and appends them to --out when given); run the command twice.
    python tools/held_study_bench.py [--reps 5] [--out profiles/r17_held_study.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.study_stats_bench import make_study  # noqa: E402


def tail(ds, engine):
    from tee_optical_flow_amd import analysis as A
    cent = A.av_centroids(ds.get_mask("av"), ds.nframes, engine=engine)
    out = [np.asarray(cent)]
    for p in A.PARAMS:
        st = A.calculate_3dhist_radlong(ds, p, engine=engine, centroids=cent)
        out += [np.asarray(x) for c in ("radial", "longitudinal") for x in st[c]]
    for p in A.PARAMS:
        out += [np.asarray(x) for x in A.calculate_3dhist(ds, p, "rv", engine=engine)]
    out.append(A.angle_mode_series(ds, "velocity", "rv", engine=engine))
    out.append(A.area_series(ds, "rv", engine=engine))
    out.append(A.radlong_overlay(ds, "velocity", engine=engine, centroids=cent))
    return out


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd.synth import speckle_sequence
    eng = T.DenseFlow(device_id=0)
    lines = []
    for H, W in ((512, 512), (600, 800)):
        N = a.frames
        rv, av, _ = make_study(N + H + W, N, H, W)
        masks = {"rv": rv, "av": av}
        rgb = np.ascontiguousarray(np.repeat(speckle_sequence(N + H, N, H, W)[..., None], 3, axis=3))
        flow, echo = eng.calc_study_payload(rgb, scale=50.0)
        st = T.FlowStudy(flow, masks, 50.0, echo=echo)

        def host():
            return tail(st, eng)

        def held():
            return tail(T.HeldStudy.from_study(eng, st), eng)

        def solved():
            for label, m in masks.items():
                eng.hold_mask(label, m)
            return tail(T.HeldStudy(eng, 50.0), eng)

        ways = (("host", host), ("held", held), ("solved", solved))
        times, mb, equal, ref = {k: [] for k, _ in ways}, {}, True, None
        for rep in range(a.reps + 1):                         # rep 0: the warm-up
            for name, fn in ways:
                if name == "solved":
                    f2, e2 = eng.calc_study_payload(rgb, scale=50.0, hold=True)
                    equal = equal and np.array_equal(f2, flow) and np.array_equal(e2, echo)
                c = eng.counter("tail_upload_bytes")
                t = time.perf_counter(); r = fn(); dt = time.perf_counter() - t
                mb[name] = round((eng.counter("tail_upload_bytes") - c) / 1e6, 1)
                ref = r if ref is None else ref
                equal = equal and same(r, ref)
                if rep:
                    times[name].append(dt * 1e3)
        eng.release_study()
        res = {"what": "full study tail, host-pointer calls vs held study", "size": f"{H}x{W}", "frames": N, "reps": a.reps, "bit_equal": bool(equal)}
        for name, _ in ways:
            res[name] = {"ms": round(float(np.median(times[name])), 1), "ms_min": round(min(times[name]), 1), "ms_max": round(max(times[name]), 1),
                         "upload_mb": mb[name]}
        res["held_over_host"] = round(res["held"]["ms"] / res["host"]["ms"], 3)
        res["solved_over_host"] = round(res["solved"]["ms"] / res["host"]["ms"], 3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    eng.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
