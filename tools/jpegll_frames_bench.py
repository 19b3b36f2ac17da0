#!/usr/bin/env python3
"""One 65-frame sector-masked speckle study (an ultrasound fan: blurred noise inside, black outside), 3 samples and 1, at 512x512 and
600x800, stored as JPEG Lossless frames (SOF3, predictor 1: the SV1 transfer syntax) -- without restart markers, with restart intervals
of 64 and of 8 rows, and of one row -- from host memory to the held frames, timed in ways that are interleaved in one process:
    split_1        hold_frames_jpeg_lossless with tf_set_tuning "jpegll_split" = 1: the serial entropy kernel only, one wave an interval
                   (the path before there was a split decode: the yardstick for the two below)
    split_2        ... = 2: the split entropy decode for every interval (pieces of tf_jpegll_segment_bytes bytes, speculation, the
                   default rounds, prefix sums, emit; what did not converge goes to the serial kernel)
    split_0        ... = 0, the default: the host picks per frame by the bytes of entropy data an interval holds on average
    raw_hold       hold_frames of the already decoded array: upload only, the yardstick for the device side as a whole
    pil_then_hold  PIL's decode of every frame on this thread, then hold_frames: only where PIL imports and takes an SOF3 stream
Median of --reps after a warm-up; in the warm-up round the held frames of every way are downloaded and compared with the encoded study
bit for bit.  Every way is run twice back to back and its second run is timed (see tools/rle_frames_bench.py for why).  Per case the
device time of the entropy work and of the reconstruction is recorded for the three device ways, the counters of the split decode, and
the fewest rounds at which no interval falls back to the serial kernel ("rounds_needed", from a sweep of "jpegll_sync_rounds").
The last line lists, per interval length, split_2 over split_1: the automatic rule's threshold is read from it.  The walk
(process_folder), the pydicom plug-ins' decode and real scanner files are not measured here.  The streams come from
frames.jpegll_encode_frame (numpy; no PIL needed).
    python tools/jpegll_frames_bench.py [--reps 5] [--out profiles/r31_jpegll_split.txt]"""
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

RESTARTS = (("none", 0), ("64_rows", 64), ("8_rows", 8), ("row", 1))
NOISE = 0.04                                                               # the box-to-box noise the README documents


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
    ap.add_argument("--samples", default="3,1")
    ap.add_argument("--max-rounds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_jpegll_split.txt"))
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    from tee_optical_flow_amd import frames as F
    from tee_optical_flow_amd import _lib
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    lines, ratio = [], []
    for H, W in sizes:
        rgb = sector_study(a.frames, H, W)
        for samples in (int(v) for v in a.samples.split(",")):
            raw = rgb if samples == 3 else np.ascontiguousarray(rgb[..., 0])
            form = "RGB" if samples == 3 else "GRAY"
            want = F.ingest_host(raw, form, False)
            for restart, rows in RESTARTS:
                if rows * W > 65535:
                    continue
                streams = [F.jpegll_encode_frame(f, rows) for f in raw]
                N = len(streams)
                rec = F.jpegll_record(streams)
                Image = pil_decoder(streams[0])
                pil_ms = []

                def device(mode):
                    def run():
                        eng.set_tuning("jpegll_split", mode)
                        try:
                            return eng.hold_frames_jpeg_lossless(rec, H, W, samples, form)
                        finally:
                            eng.set_tuning("jpegll_split", 0)
                    return run

                def pil_then_hold():
                    t = time.perf_counter()
                    arr = np.stack([np.asarray(Image.open(io.BytesIO(s))) for s in streams])
                    pil_ms.append((time.perf_counter() - t) * 1e3)
                    return eng.hold_frames(arr, form)

                ways = [("split_1", device(1)), ("split_2", device(2)), ("split_0", device(0)), ("raw_hold", lambda: eng.hold_frames(raw, form))]
                if Image is not None:
                    ways.append(("pil_then_hold", pil_then_hold))
                times, up, kern, equal = {k: [] for k, _ in ways}, {}, {}, True
                for rep in range(a.reps + 1):                     # rep 0: the warm-up, and the comparison of the results
                    for name, fn in ways:
                        fn()
                        u0, s0, f0 = (eng.counter(k) for k in ("frames_upload_bytes", "jpegll_split_intervals", "jpegll_serial_fallbacks"))
                        t = time.perf_counter(); fn(); dt = time.perf_counter() - t
                        up[name] = eng.counter("frames_upload_bytes") - u0
                        kern[name] = {k: eng.counter(k) for k in ("jpegll_entropy_us", "jpegll_restore_us", "ingest_kernel_us", "jpegll_sync_rounds")}
                        kern[name].update(split_intervals=eng.counter("jpegll_split_intervals") - s0, serial_fallbacks=eng.counter("jpegll_serial_fallbacks") - f0)
                        if rep == 0:
                            equal = equal and np.array_equal(eng.download_frames(), want)
                        else:
                            times[name].append(dt * 1e3)
                needed = None                                     # the fewest rounds at which nothing falls back
                for r in range(a.max_rounds + 1):
                    eng.set_tuning("jpegll_sync_rounds", r)
                    f0 = eng.counter("jpegll_serial_fallbacks")
                    try:
                        device(2)()
                    finally:
                        eng.set_tuning("jpegll_sync_rounds", _lib.JPEGLL_SYNC_ROUNDS)
                    if eng.counter("jpegll_serial_fallbacks") == f0:
                        needed = r
                        break
                eng.release_frames()
                nint = 1 if rows == 0 else -(-H // rows)
                res = {"what": "JPEG Lossless frames in host memory -> held frames", "study": f"sector-masked speckle, {samples} sample(s), SOF3 predictor 1",
                       "size": f"{H}x{W}", "samples": samples, "restart": restart, "intervals_per_frame": nint, "frames": N, "reps": a.reps, "bit_equal": bool(equal),
                       "compressed_bytes": int(rec[0].size), "raw_bytes": int(raw.nbytes), "bytes_per_interval": int(rec[0].size // (N * nint)),
                       "segment_bytes": _lib.JPEGLL_SEGMENT_BYTES, "default_rounds": _lib.JPEGLL_SYNC_ROUNDS, "rounds_needed": needed, "numpy": np.__version__}
                for name, _ in ways:
                    res[name] = {"ms": round(float(np.median(times[name])), 2), "ms_min": round(min(times[name]), 2), "ms_max": round(max(times[name]), 2),
                                 "frames_upload_bytes": int(up[name])}
                    if name.startswith("split_"):
                        res[name].update({k: int(v) for k, v in kern[name].items()})
                for name in ("split_2", "split_0"):
                    res[f"{name}_over_split_1"] = round(res[name]["ms"] / res["split_1"]["ms"], 3)
                res["split_0_over_raw_hold"] = round(res["split_0"]["ms"] / res["raw_hold"]["ms"], 3)
                if Image is not None:
                    res["pil_then_hold"]["pil_decode_ms"] = round(float(np.median(pil_ms[1:])), 1)
                    res["split_0_over_pil_then_hold"] = round(res["split_0"]["ms"] / res["pil_then_hold"]["ms"], 3)
                else:
                    res["pil_then_hold"] = "not measured (no PIL here that decodes SOF3)"
                res["verdict"] = ("the split decode " + ("beats" if res["split_2_over_split_1"] < 1 - NOISE else "does NOT beat") + " the serial kernel; the default is "
                                  + ("NOT slower" if res["split_0_over_split_1"] <= 1 + NOISE else "SLOWER") + " than the serial kernel; it "
                                  + ("beats" if res["split_0_over_raw_hold"] < 1 else "LOSES to") + " uploading the already decoded frames"
                                  + ("" if Image is None else " and " + ("beats" if res["split_0_over_pil_then_hold"] < 1 else "LOSES to") + " PIL's host decode followed by the upload"))
                ratio.append((res["bytes_per_interval"], res["size"], samples, restart, res["split_2_over_split_1"], res["split_0_over_split_1"], needed))
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
    eng.close()
    won = [b for b, *_, r2, _r0, _n in ratio if r2 < 1 - NOISE]
    lost = [b for b, *_, r2, _r0, _n in ratio if r2 >= 1 - NOISE]
    lines.append(json.dumps({"what": "split_2 over split_1 by the bytes of entropy data an interval holds", "cases": sorted(ratio),
                             "smallest_interval_the_split_decode_wins_at": min(won) if won else None,
                             "largest_interval_it_does_not_win_at": max(lost) if lost else None,
                             "rounds_needed_max": max((n for *_, n in ratio if n is not None), default=None)}))
    print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln).get("bit_equal", True) for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
