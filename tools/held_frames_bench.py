#!/usr/bin/env python3
"""One 65-frame study at 512x512 and 600x800 from YBR_FULL frames in host memory to the file's float16 payload plus its Otsu masks,
timed three ways that are interleaved in one process:
    host     today's path: frames.ybr_full_to_rgb on this thread, otsu_masks(rgb), calc_study_payload(rgb) -- two uploads of the RGB
    held     hold_frames(ybr, "YBR_FULL"), then the two calls from the token -- one upload, as stored, converted by k_ingest
    held_rgb the same from RGB frames (the twin's, converted outside the clock): what the single upload alone is worth
Median of --reps after a warm-up; flows, echo, masks and thresholds of the three ways are checked bit-equal in the warm-up round.  The
yardstick is `host`, measured in the same run; `held` alone says nothing.  Per way: the wall time, the host conversion's share of it,
the bytes of frames that went host -> device (the library's frames_upload_bytes) and, for the held ways, k_ingest's device time against
the bytes it read and wrote (the library's events).  The walk (process_folder) is not measured here.  Prints one JSON line per size and
writes them to --out (default profiles/r24_held_frames.txt, replaced by every run).
    python tools/held_frames_bench.py [--reps 5] [--out profiles/r24_held_frames.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_held_frames.txt"))
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import frames as F
    from tee_optical_flow_amd.synth import speckle_sequence
    eng = T.DenseFlow(device_id=0)
    lines = []
    for H, W in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        N = a.frames
        rng = np.random.default_rng(N + H)
        g = speckle_sequence(N + H, N, H, W)
        ybr = np.ascontiguousarray(np.stack([g, rng.integers(96, 160, g.shape, dtype=np.uint8), rng.integers(96, 160, g.shape, dtype=np.uint8)], -1))
        rgb_twin = F.ybr_full_to_rgb(ybr)
        convert_ms = []

        def solve(frames):
            masks, thr = eng.otsu_masks(frames, 64, return_thresholds=True)
            flow, echo = eng.calc_study_payload(frames, scale=50.0)
            return [np.asarray(x) for x in (flow, echo, masks, thr)]

        def host():
            t = time.perf_counter()
            rgb = F.ybr_full_to_rgb(ybr)
            convert_ms.append((time.perf_counter() - t) * 1e3)
            return solve(rgb)

        ways = (("host", host), ("held", lambda: solve(eng.hold_frames(ybr, "YBR_FULL"))), ("held_rgb", lambda: solve(eng.hold_frames(rgb_twin, "RGB"))))
        times, up, kern, equal, ref = {k: [] for k, _ in ways}, {}, {}, True, None
        for rep in range(a.reps + 1):                         # rep 0: the warm-up, and the comparison of the results
            for name, fn in ways:
                u0 = eng.counter("frames_upload_bytes")
                t = time.perf_counter(); r = fn(); dt = time.perf_counter() - t
                up[name] = eng.counter("frames_upload_bytes") - u0
                if name != "host":
                    kern[name] = {"us": eng.counter("ingest_kernel_us"), "bytes": eng.counter("ingest_bytes")}
                if rep == 0:
                    ref = r if ref is None else ref
                    equal = equal and all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(r, ref))
                else:
                    times[name].append(dt * 1e3)
        eng.release_frames()
        res = {"what": "YBR_FULL frames in host memory -> float16 payload + Otsu masks", "size": f"{H}x{W}", "frames": N, "reps": a.reps,
               "bit_equal": bool(equal), "numpy": np.__version__}
        for name, _ in ways:
            res[name] = {"ms": round(float(np.median(times[name])), 1), "ms_min": round(min(times[name]), 1), "ms_max": round(max(times[name]), 1),
                         "frames_upload_bytes": int(up[name])}
        res["host"]["convert_ms"] = round(float(np.median(convert_ms[1:])), 1)
        for name in ("held", "held_rgb"):
            k = kern[name]
            res[name]["k_ingest"] = {"us": int(k["us"]), "bytes": int(k["bytes"]), "gb_per_s": round(k["bytes"] / k["us"] / 1e3, 1) if k["us"] else None}
        res["held_over_host"] = round(res["held"]["ms"] / res["host"]["ms"], 3)
        res["held_rgb_over_host_less_convert"] = round(res["held_rgb"]["ms"] / (res["host"]["ms"] - res["host"]["convert_ms"]), 3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    eng.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln)["bit_equal"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
