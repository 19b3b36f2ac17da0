#!/usr/bin/env python3
"""One 65-frame sector-masked speckle study (an ultrasound fan: blurred noise inside, black outside) at 512x512 and 600x800, stored as
JPEG Baseline frames -- 4:2:2, quality 90, without restart markers and with a restart interval of one MCU row -- from host memory to the
held RGB frames, timed three ways that are interleaved in one process:
    jpeg_device    hold_frames_jpeg(record, form="YBR_FULL", color="libjpeg"): the compressed bytes go up, the four k_jpeg_* kernels and
                   k_ingest_planar make the held frames
    raw_hold       hold_frames of the already decoded RGB array: the parent commit's upload-only path, the yardstick for the device side
    pil_then_hold  PIL's decode of every frame on this thread, then hold_frames: only where PIL imports
Median of --reps after a warm-up; in the warm-up round the held frames of every way are downloaded and their SHA-256 compared with the
digest of Pillow's RGB decode that travels with the streams.  Every way is run twice back to back and its second run is timed (see
tools/rle_frames_bench.py for why).  The verdict says plainly whether the device decode beats either yardstick.  The walk
(process_folder) is not measured here.
The streams come from Pillow's encoder.  Where PIL does not import (the GPU box may lack it), --streams names an .npz that
`--make-streams` wrote on a machine that has it: the same frames, the same bytes.
    python tools/jpeg_frames_bench.py --make-streams S.npz          (needs PIL on libjpeg-turbo; no GPU)
    python tools/jpeg_frames_bench.py [--streams S.npz] [--reps 5] [--out profiles/r29_jpeg_frames.txt]"""
import argparse
import hashlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RESTARTS = ("none", "mcu_row")


def sector_study(N, H, W, seed=0):
    """N RGB frames of speckle (noise under a 3 x 3 box blur, so that neighbours correlate as speckle does) inside a fan, black outside"""
    rng = np.random.default_rng(seed + N + H)
    y, x = np.mgrid[0:H, 0:W]
    inside = (np.abs(x - (W - 1) / 2) <= 0.8 * (y + 1)) & ((x - (W - 1) / 2) ** 2 + y ** 2 <= (0.95 * H) ** 2)
    g = rng.integers(1, 256, (N, H + 2, W + 2)).astype(np.float32)
    g = sum(g[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) / 9.0
    g = np.clip((g - 128.0) * 2.5 + 128.0, 0, 255).astype(np.uint8) * inside[None].astype(np.uint8)
    return np.stack([g, g, (g // 2 + 64) * inside[None].astype(np.uint8)], -1)


def encode_study(raw, restart):
    from PIL import Image
    W = raw.shape[2]
    out, sha = [], hashlib.sha256()
    for f in raw:
        bio = io.BytesIO()
        Image.fromarray(f, "RGB").save(bio, "JPEG", quality=90, subsampling=1, restart_marker_blocks=(-(-W // 16) if restart == "mcu_row" else 0))
        out.append(bio.getvalue())
        sha.update(np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(out[-1])))).tobytes())
    return out, sha.hexdigest()


def studies(a, sizes):
    """{(H, W, restart): (list of streams, digest of Pillow's RGB decode of all of them)}"""
    if a.streams and os.path.exists(a.streams) and not a.make_streams:
        z = np.load(a.streams)
        got = {}
        for k, key in enumerate(z["keys"].tolist()):
            H, W, restart = key.split("_", 2)
            blob, off, ln = z[f"blob{k}"].tobytes(), z[f"off{k}"], z[f"len{k}"]
            got[(int(H), int(W), restart)] = ([blob[int(o):int(o) + int(n)] for o, n in zip(off, ln)], str(z["sha"][k]))
        return got
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "the yardstick is libjpeg-turbo as Pillow drives it"
    return {(H, W, r): encode_study(sector_study(a.frames, H, W), r) for H, W in sizes for r in RESTARTS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--streams", default=None)
    ap.add_argument("--make-streams", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_jpeg_frames.txt"))
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    from tee_optical_flow_amd import frames as F
    got = studies(a, sizes)
    if a.make_streams:
        arrays = {"keys": np.array([f"{H}_{W}_{r}" for H, W, r in got]), "sha": np.array([v[1] for v in got.values()])}
        for k, (streams, _) in enumerate(got.values()):
            arrays[f"blob{k}"], arrays[f"off{k}"], arrays[f"len{k}"] = F.jpeg_record(streams)
        np.savez(a.make_streams, **arrays)
        print(f"{len(got)} studies, {sum(len(s) for v in got.values() for s in v[0])} bytes -> {a.make_streams}")
        return 0
    try:
        from PIL import Image
    except ImportError:
        Image = None
    import tee_optical_flow_amd as T
    eng = T.DenseFlow(device_id=0)
    sha = lambda arr: hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()
    lines = []
    for (H, W, restart), (streams, want_sha) in got.items():
        N = len(streams)
        rec = F.jpeg_record(streams)
        eng.hold_frames_jpeg(rec, H, W, 3, "YBR_FULL", color="libjpeg")
        rgb = eng.download_frames()                            # the decoded array of the upload-only path (checked against the digest below)
        pil_ms = []

        def pil_then_hold():
            t = time.perf_counter()
            arr = np.stack([np.asarray(Image.open(io.BytesIO(s))) for s in streams])
            pil_ms.append((time.perf_counter() - t) * 1e3)
            return eng.hold_frames(arr, "RGB")

        ways = [("jpeg_device", lambda: eng.hold_frames_jpeg(rec, H, W, 3, "YBR_FULL", color="libjpeg")), ("raw_hold", lambda: eng.hold_frames(rgb, "RGB"))]
        if Image is not None:
            ways.append(("pil_then_hold", pil_then_hold))
        times, up, kern, equal = {k: [] for k, _ in ways}, {}, {}, True
        for rep in range(a.reps + 1):                         # rep 0: the warm-up, and the comparison of the results
            for name, fn in ways:
                fn()
                u0 = eng.counter("frames_upload_bytes")
                t = time.perf_counter(); fn(); dt = time.perf_counter() - t
                up[name] = eng.counter("frames_upload_bytes") - u0
                kern[name] = {k: eng.counter(k) for k in ("jpeg_marks_us", "jpeg_entropy_us", "jpeg_idct_us", "jpeg_finish_us", "jpeg_bytes", "ingest_kernel_us")}
                if rep == 0:
                    equal = equal and sha(eng.download_frames()) == want_sha
                else:
                    times[name].append(dt * 1e3)
        eng.release_frames()
        res = {"what": "JPEG Baseline frames in host memory -> held RGB frames", "study": "sector-masked speckle, 4:2:2, quality 90", "size": f"{H}x{W}",
               "restart": restart, "intervals_per_frame": 1 if restart == "none" else -(-H // 8), "frames": N, "reps": a.reps, "bit_equal": bool(equal),
               "compressed_bytes": int(rec[0].size), "raw_bytes": int(rgb.nbytes), "compressed_over_raw": round(rec[0].size / rgb.nbytes, 3),
               "numpy": np.__version__}
        for name, _ in ways:
            res[name] = {"ms": round(float(np.median(times[name])), 2), "ms_min": round(min(times[name]), 2), "ms_max": round(max(times[name]), 2),
                         "frames_upload_bytes": int(up[name])}
        res["jpeg_device"].update({k: int(v) for k, v in kern["jpeg_device"].items()})
        res["jpeg_device_over_raw_hold"] = round(res["jpeg_device"]["ms"] / res["raw_hold"]["ms"], 3)
        if Image is not None:
            res["pil_then_hold"]["pil_decode_ms"] = round(float(np.median(pil_ms[1:])), 1)
            res["jpeg_device_over_pil_then_hold"] = round(res["jpeg_device"]["ms"] / res["pil_then_hold"]["ms"], 3)
        else:
            res["pil_then_hold"] = "not measured (PIL does not import here)"
        res["verdict"] = ("the device decode " + ("beats" if res["jpeg_device_over_raw_hold"] < 1 else "LOSES to") + " uploading the already decoded frames"
                          + ("" if Image is None else "; it " + ("beats" if res["jpeg_device_over_pil_then_hold"] < 1 else "LOSES to") + " PIL's host decode followed by the upload"))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    eng.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln)["bit_equal"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
