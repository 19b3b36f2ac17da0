#!/usr/bin/env python3
"""One 65-frame sector-masked speckle study (an ultrasound fan: blurred noise inside, black outside), 3 samples, at 512x512 and 600x800,
stored as JPEG Lossless frames (SOF3, predictor 1: the SV1 transfer syntax) -- without restart markers and with a restart interval of
one row -- from host memory to the held RGB frames, timed three ways that are interleaved in one process:
    jpegll_device  hold_frames_jpeg_lossless(record, form="RGB"): the compressed bytes go up, k_jpeg_marks, the three k_jpegll_* kernels
                   and k_ingest_planar make the held frames
    raw_hold       hold_frames of the already decoded RGB array: the parent commit's upload-only path, the yardstick for the device side
    pil_then_hold  PIL's decode of every frame on this thread, then hold_frames: only where PIL imports and takes an SOF3 stream
Median of --reps after a warm-up; in the warm-up round the held frames of every way are downloaded and compared with the encoded study
bit for bit.  Every way is run twice back to back and its second run is timed (see tools/rle_frames_bench.py for why).  The verdict
says plainly whether the device decode beats either yardstick.  The walk (process_folder) and the pydicom plug-ins' decode are not
measured here.  The streams come from frames.jpegll_encode_frame (numpy; no PIL needed).
    python tools/jpegll_frames_bench.py [--reps 5] [--out profiles/r30_jpegll_frames.txt]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.jpeg_frames_bench import sector_study  # noqa: E402

RESTARTS = ("none", "row")


def pil_decoder(probe):
    """PIL's Image where it imports on libjpeg-turbo and decodes this SOF3 stream, else None"""
    try:
        from PIL import Image, features
        if not features.check_feature("libjpeg_turbo"):
            return None
        np.asarray(Image.open(io.BytesIO(probe)))
        return Image
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_jpegll_frames.txt"))
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    from tee_optical_flow_amd import frames as F
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    lines = []
    for H, W in sizes:
        raw = sector_study(a.frames, H, W)
        for restart in RESTARTS:
            streams = [F.jpegll_encode_frame(f, 1 if restart == "row" else 0) for f in raw]
            N = len(streams)
            rec = F.jpegll_record(streams)
            Image = pil_decoder(streams[0])
            pil_ms = []

            def pil_then_hold():
                t = time.perf_counter()
                arr = np.stack([np.asarray(Image.open(io.BytesIO(s))) for s in streams])
                pil_ms.append((time.perf_counter() - t) * 1e3)
                return eng.hold_frames(arr, "RGB")

            ways = [("jpegll_device", lambda: eng.hold_frames_jpeg_lossless(rec, H, W, 3, "RGB")), ("raw_hold", lambda: eng.hold_frames(raw, "RGB"))]
            if Image is not None:
                ways.append(("pil_then_hold", pil_then_hold))
            times, up, kern, equal = {k: [] for k, _ in ways}, {}, {}, True
            for rep in range(a.reps + 1):                         # rep 0: the warm-up, and the comparison of the results
                for name, fn in ways:
                    fn()
                    u0 = eng.counter("frames_upload_bytes")
                    t = time.perf_counter(); fn(); dt = time.perf_counter() - t
                    up[name] = eng.counter("frames_upload_bytes") - u0
                    kern[name] = {k: eng.counter(k) for k in ("jpegll_entropy_us", "jpegll_restore_us", "jpegll_bytes", "ingest_kernel_us")}
                    if rep == 0:
                        equal = equal and np.array_equal(eng.download_frames(), raw)
                    else:
                        times[name].append(dt * 1e3)
            eng.release_frames()
            res = {"what": "JPEG Lossless frames in host memory -> held RGB frames", "study": "sector-masked speckle, 3 samples, SOF3 predictor 1", "size": f"{H}x{W}",
                   "restart": restart, "intervals_per_frame": 1 if restart == "none" else H, "frames": N, "reps": a.reps, "bit_equal": bool(equal),
                   "compressed_bytes": int(rec[0].size), "raw_bytes": int(raw.nbytes), "compressed_over_raw": round(rec[0].size / raw.nbytes, 3),
                   "numpy": np.__version__}
            for name, _ in ways:
                res[name] = {"ms": round(float(np.median(times[name])), 2), "ms_min": round(min(times[name]), 2), "ms_max": round(max(times[name]), 2),
                             "frames_upload_bytes": int(up[name])}
            res["jpegll_device"].update({k: int(v) for k, v in kern["jpegll_device"].items()})
            res["jpegll_device_over_raw_hold"] = round(res["jpegll_device"]["ms"] / res["raw_hold"]["ms"], 3)
            if Image is not None:
                res["pil_then_hold"]["pil_decode_ms"] = round(float(np.median(pil_ms[1:])), 1)
                res["jpegll_device_over_pil_then_hold"] = round(res["jpegll_device"]["ms"] / res["pil_then_hold"]["ms"], 3)
            else:
                res["pil_then_hold"] = "not measured (no PIL here that decodes SOF3)"
            res["verdict"] = ("the device decode " + ("beats" if res["jpegll_device_over_raw_hold"] < 1 else "LOSES to") + " uploading the already decoded frames"
                              + ("" if Image is None else "; it " + ("beats" if res["jpegll_device_over_pil_then_hold"] < 1 else "LOSES to")
                                 + " PIL's host decode followed by the upload"))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    eng.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln)["bit_equal"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
