#!/usr/bin/env python3
"""One 65-frame sector-masked speckle study (an ultrasound fan: speckle inside, black outside; 3 samples a pixel) at 512x512 and 600x800,
stored as DICOM RLE Lossless frames, from host memory to the held RGB frames, timed three ways that are interleaved in one process:
    rle_device      hold_frames_rle(record): the compressed bytes go up, k_rle_decode and k_ingest_planar make the held frames
    twin_then_hold  frames.rle_decode_frame on this thread, then hold_frames(decoded): the host decode is the PYTHON TWIN, not pydicom
                    (pydicom is not installed here: no pydicom figure is measured or claimed)
    raw_hold        hold_frames of the already decoded array: the parent commit's path, and the yardstick for the device side alone
rle_device and raw_hold are timed for the forms RGB (raw_hold is then one plain upload, no kernel) and YBR_FULL, twin_then_hold for
YBR_FULL.  Median of --reps after a warm-up; in the warm-up round the held frames of every way are downloaded and checked bit-equal.
Every way is run twice back to back and its second run is timed: timed singly, the way that followed the twin's host-only stretch (a few
hundred ms without GPU work) took 12-54 ms where it takes 2-3 ms in any other position -- the cost of that position (a device gone idle,
it is supposed), not of the way.
Per size: compressed and raw bytes, the controls (literal, run and no-op bytes) per segment, and for rle_device k_rle_decode's and the
ingest kernel's device time (the library's events).  The verdict line says plainly whether the device decode beats uploading the raw
frames; the host decode it replaces is not part of that comparison.  The walk (process_folder) is not measured here.  Prints one JSON
line per size and writes them to --out (replaced by every run).
    python tools/rle_frames_bench.py [--reps 5] [--out profiles/r25_rle_frames.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sector_study(N, H, W, seed=0):
    """N frames of speckle inside a fan, black outside, three samples that differ"""
    rng = np.random.default_rng(seed + N + H)
    y, x = np.mgrid[0:H, 0:W]
    inside = (np.abs(x - (W - 1) / 2) <= 0.8 * (y + 1)) & ((x - (W - 1) / 2) ** 2 + y ** 2 <= (0.95 * H) ** 2)
    return rng.integers(1, 256, (N, H, W, 3), dtype=np.uint8) * inside[None, ..., None].astype(np.uint8)


def controls(frame, plane):
    """the control bytes a decoder reads in each segment of a conformant frame, to the plane's last byte"""
    head = np.frombuffer(frame[:64], "<u4")
    n = []
    for k in range(int(head[0])):
        seg = frame[head[1 + k]:head[2 + k] if k + 1 < head[0] else len(frame)]
        pos = made = hops = 0
        while made < plane:
            c = seg[pos]
            hops += 1
            if c < 128:
                pos += c + 2
                made += c + 1
            elif c > 128:
                pos += 2
                made += 257 - c
            else:
                pos += 1
        n.append(hops)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_rle_frames.txt"))
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import frames as F
    eng = T.DenseFlow(device_id=0)
    lines = []
    for H, W in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        N = a.frames
        raw = sector_study(N, H, W)
        enc = [F.rle_encode_frame(f) for f in raw]
        rec = F.rle_record(enc)
        hops = np.array([controls(f, H * W) for f in enc])
        decode_ms = []

        def twin(form):
            t = time.perf_counter()
            arr = np.stack([F.rle_decode_frame(f, H, W, 3)[0] for f in enc])
            decode_ms.append((time.perf_counter() - t) * 1e3)
            return eng.hold_frames(arr, form)

        ways = [(f"rle_device_{form}", form, lambda form=form: eng.hold_frames_rle(rec, H, W, 3, form)) for form in ("RGB", "YBR_FULL")]
        ways += [(f"raw_hold_{form}", form, lambda form=form: eng.hold_frames(raw, form)) for form in ("RGB", "YBR_FULL")]
        ways.append(("twin_then_hold_YBR_FULL", "YBR_FULL", lambda: twin("YBR_FULL")))
        times, up, kern, equal = {k: [] for k, _, _ in ways}, {}, {}, True
        want = {form: F.ingest_host(raw, form) for form in ("RGB", "YBR_FULL")}
        for rep in range(a.reps + 1):                         # rep 0: the warm-up, and the comparison of the results
            for name, form, fn in ways:
                fn()                                          # untimed: the run that follows the twin's host-only stretch is 10-50 ms slower
                u0 = eng.counter("frames_upload_bytes")
                t = time.perf_counter(); fn(); dt = time.perf_counter() - t
                up[name] = eng.counter("frames_upload_bytes") - u0
                kern[name] = {k: eng.counter(k) for k in ("rle_kernel_us", "rle_bytes", "ingest_kernel_us", "ingest_bytes")}
                if rep == 0:
                    equal = equal and bool(np.array_equal(eng.download_frames(), want[form]))
                else:
                    times[name].append(dt * 1e3)
        eng.release_frames()
        res = {"what": "RLE Lossless frames in host memory -> held RGB frames", "study": "sector-masked speckle, 3 samples", "size": f"{H}x{W}", "frames": N,
               "reps": a.reps, "bit_equal": bool(equal), "compressed_bytes": int(rec[0].size), "raw_bytes": int(raw.nbytes),
               "compressed_over_raw": round(rec[0].size / raw.nbytes, 3),
               "controls_per_segment": {"median": int(np.median(hops)), "min": int(hops.min()), "max": int(hops.max())}, "numpy": np.__version__}
        for name, _, _ in ways:
            res[name] = {"ms": round(float(np.median(times[name])), 2), "ms_min": round(min(times[name]), 2), "ms_max": round(max(times[name]), 2),
                         "frames_upload_bytes": int(up[name])}
        for form in ("RGB", "YBR_FULL"):
            k = kern[f"rle_device_{form}"]
            res[f"rle_device_{form}"].update(rle_kernel_us=int(k["rle_kernel_us"]), rle_bytes=int(k["rle_bytes"]), ingest_kernel_us=int(k["ingest_kernel_us"]),
                                             ingest_bytes=int(k["ingest_bytes"]))
            res[f"raw_hold_{form}"].update(ingest_kernel_us=int(kern[f"raw_hold_{form}"]["ingest_kernel_us"]))
            ratio = res[f"rle_device_{form}"]["ms"] / res[f"raw_hold_{form}"]["ms"]
            res[f"rle_device_over_raw_hold_{form}"] = round(ratio, 3)
        res["twin_then_hold_YBR_FULL"]["python_twin_decode_ms"] = round(float(np.median(decode_ms[1:])), 1)
        res["pydicom_decode_ms"] = "not measured (pydicom is not installed)"
        beats = [form for form in ("RGB", "YBR_FULL") if res[f"rle_device_over_raw_hold_{form}"] < 1.0]
        res["verdict"] = ("the device decode beats uploading the raw frames for " + " and ".join(beats) if len(beats) == 2 else
                          "the device decode beats uploading the raw frames for " + beats[0] + " only" if beats else
                          "the device decode LOSES to uploading the raw frames (already decoded): what it saves is the host decode, which this comparison leaves out")
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    eng.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln)["bit_equal"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
