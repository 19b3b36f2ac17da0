#!/usr/bin/env python3
"""The Otsu mode's masks (reference calculate_optical_flow.py:184-213) on the host against the device call (DenseFlow.otsu_masks /
tf_otsu_masks: host uint8 RGB in, host bool out, transfers included), alternating the two after a warm-up, with bit-equality of the
results; then a tools/study_throughput.py-style walk, process_folder(mode="otsu") over studies of 65 frames 512x512 with reader and
writer processes and the real gzip-9 HDF5 write, with otsu_masks="host" (the reader stage makes the masks, one study ahead) and
"device" (the walk asks the engine), alternating.  The walk needs h5py, which lives in the image's second interpreter:
    LD_PRELOAD="$LD_PRELOAD /usr/lib/x86_64-linux-gnu/libstdc++.so.6" /opt/conda/bin/python3.9 tools/otsu_bench.py [--reps 3] [--studies 16] [--runs 2]
`--profile-call SIZE` (speckle512 | sector800) makes only warmed device calls of that size, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/otsu_bench.py --profile-call speckle512"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sector(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    ang = np.arctan2(xx - W / 2, yy + H * 0.05)
    return (np.abs(ang) < 0.7) & (np.hypot(xx - W / 2, yy + H * 0.05) < H * 0.98)


def study(kind, N, H, W):
    """speckle512: true RGB speckle (independent noise per channel); sector800: sector-masked grey speckle on a zero background"""
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(N + H + W, N, H, W)
    if kind == "sector800":
        g = np.where(sector(H, W)[None], g, 0).astype(np.uint8)
        return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=3))
    rng = np.random.default_rng(N + H)
    out = np.empty((N, H, W, 3), np.uint8)
    for c in range(3):
        out[..., c] = np.clip(g.astype(np.int16) + rng.integers(-12, 13, g.shape, dtype=np.int16), 0, 255)
    return out


SIZES = {"speckle512": (65, 512, 512), "sector800": (65, 600, 800)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--studies", type=int, default=16)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--readers", type=int, default=3)
    ap.add_argument("--writers", type=int, default=3)
    ap.add_argument("--profile-call", choices=sorted(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_otsu_masks.txt"))
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import masks
    from tee_optical_flow_amd import pipeline as P

    class Cfg:
        min_mask_size = 500

    if a.profile_call:
        frames = study(a.profile_call, *SIZES[a.profile_call])
        eng = T.DenseFlow(device_id=0)
        for _ in range(1 + a.reps):
            eng.otsu_masks(frames, Cfg.min_mask_size)
        eng.close()
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    workers = None
    try:
        import h5py  # noqa: F401
        workers = P.StudyWorkers(a.readers, a.writers)       # the worker processes must exist before anything here touches the GPU
    except ImportError:
        say("(no h5py in this interpreter: the process_folder walk is left out)")
    eng = T.DenseFlow(device_id=0)
    say("predict_movie_thres, host (numpy / scipy) vs device (tf_otsu_masks, host uint8 RGB in, host bool out, transfers included); min_mask_size 500")
    for kind, (N, H, W) in SIZES.items():
        frames = study(kind, N, H, W)
        masks.predict_movie_thres(frames[:4], config=Cfg)                       # warm-up of both
        masks.predict_movie_thres(frames, config=Cfg, engine=eng)
        th, td, equal = [], [], True
        for _ in range(a.reps):
            t = time.perf_counter(); h = masks.predict_movie_thres(frames, config=Cfg)["otsu"]; th.append(time.perf_counter() - t)
            t = time.perf_counter(); d = masks.predict_movie_thres(frames, config=Cfg, engine=eng)["otsu"]; td.append(time.perf_counter() - t)
            equal = equal and d.dtype == h.dtype and np.array_equal(h, d)
        mh, md = np.median(th) * 1e3, np.median(td) * 1e3
        say(f"  {N}x{H}x{W} {kind:10s}: host {mh:8.1f} ms ({min(th) * 1e3:.1f}-{max(th) * 1e3:.1f}; {mh / N:.1f} ms per frame)  "
            f"device {md:7.1f} ms ({min(td) * 1e3:.1f}-{max(td) * 1e3:.1f})  speed-up {mh / md:6.1f}x  foreground {h.mean() * 100:.1f} %  "
            f"bit-equal {equal}  (median of {a.reps})")
    eng.close()
    if workers is not None:
        from tee_optical_flow_amd.synth import speckle_sequence
        tmp = tempfile.mkdtemp(prefix="teeflow_otsu_")
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        for k in range(a.studies):
            g = speckle_sequence(500 + k, 65, 512, 512)
            np.savez(os.path.join(src, f"study{k:02d}.npz"), nparr=np.repeat(g[..., None], 3, axis=3), pixel_spacing=0.04, frame_rate=50.0, patient_id=f"S{k}")
        model = P.make_flow_model("TVL1")
        kw = dict(nchunks=1, chunk_index=0, mode="otsu", verbose=False, extensions=("npz",), OF_algo="TVL1", flow_model=model, workers=workers,
                  recalculate=True)
        say(f"process_folder(mode='otsu'), {a.studies} studies of 65 frames 512x512, DualTVL1, {a.readers} reader + {a.writers} writer processes, "
            f"gzip-9 HDF5 write included")
        try:
            for where in ("host", "device"):                                     # warm-up: allocations, both code paths
                P.process_folder(src, os.path.join(tmp, "warm"), None, process_subset=True, file_subset_list=["study00.npz", "study01.npz"],
                                 otsu_masks=where, **kw)
            for run in range(a.runs):
                for where in ("host", "device"):
                    t = time.perf_counter()
                    errs = P.process_folder(src, os.path.join(tmp, "out"), None, otsu_masks=where, **kw)
                    dt = time.perf_counter() - t
                    say(f"  run {run}  otsu_masks={where:6s}: {dt:6.2f} s = {dt / a.studies * 1e3:7.1f} ms per study  errors {errs}")
        finally:
            workers.close()
            model.close()
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
