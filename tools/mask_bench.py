#!/usr/bin/env python3
"""clean_mask (reference calculate_optical_flow.py:113-182) on the host against the device call (DenseFlow.clean_masks /
tf_clean_masks: host arrays in and out, transfers included), alternating the two after a warm-up, with bit-equality of the results;
then process_folder with a stand-in segmentor and DeepFlow, studies_in_flight 1 and 2, with the masks cleaned on the host (the
engine's clean_masks hidden: the walk before the wiring) and on the device, plus the engine's coop_aborts.  The HDF5 write is
replaced by a no-op (h5py is not part of this interpreter; the writer stage runs beside the walk anyway).
    python tools/mask_bench.py [--reps 3] [--studies 3] [--out profiles/r06_mask_clean.txt]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def class_map(seed, N, H, W, n_cls):
    """drifting elliptical blobs of every class with holes, a border-touching band, salt noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((N, H, W), np.uint8)
    shapes = [(int(rng.integers(1, n_cls + 1)), rng.uniform(0, H), rng.uniform(0, W), rng.uniform(20, H / 4), rng.uniform(20, W / 4),
               rng.uniform(-2, 2, 2)) for _ in range(3 * n_cls)]
    for f in range(N):
        m = out[f]
        for c, cy, cx, ry, rx, v in shapes:
            d = ((yy - cy - v[0] * f) / ry) ** 2 + ((xx - cx - v[1] * f) / rx) ** 2
            m[d < 1.0] = c
            m[d < 0.08] = 0
        m[: H // 10, : W // 3] = 1
        salt = rng.random((H, W)) < 0.002
        m[salt] = rng.integers(0, n_cls + 1, int(salt.sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--studies", type=int, default=3)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_mask_clean.txt"))
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import hdf5_out, masks
    from tee_optical_flow_amd import pipeline as P
    from tests.test_study_driver_cpu import _FakeSam
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    class Cfg:
        min_mask_size = 500

    eng = T.DenseFlow(device_id=0, algo="deepflow")
    say("clean_mask, host (numpy / scipy) vs device (tf_clean_masks, host uint8 in, host bool out, transfers included); min_mask_size 500")
    for N, H, W, mode in ((65, 512, 512, "RVIO_2class"), (65, 512, 512, "A4C"), (65, 600, 800, "RVIO_2class")):
        arr = class_map(N + H + W, N, H, W, len(masks._MODE_LABELS[mode]))
        masks.clean_mask(arr[:4], mode, config=Cfg)                          # warm-up of both
        masks.clean_mask(arr, mode, config=Cfg, engine=eng)
        th, td, equal = [], [], True
        for _ in range(a.reps):
            t = time.perf_counter(); h = masks.clean_mask(arr, mode, config=Cfg); th.append(time.perf_counter() - t)
            t = time.perf_counter(); d = masks.clean_mask(arr, mode, config=Cfg, engine=eng); td.append(time.perf_counter() - t)
            equal = equal and list(h) == list(d) and all(np.array_equal(h[k], d[k]) and d[k].dtype == h[k].dtype for k in h)
        mh, md = np.median(th) * 1e3, np.median(td) * 1e3
        say(f"  {N}x{H}x{W} {mode:12s}: host {mh:8.1f} ms  device {md:7.1f} ms  ({min(td) * 1e3:.1f}-{max(td) * 1e3:.1f})  speed-up {mh / md:6.1f}x  "
            f"bit-equal {equal}  (median of {a.reps})")
    eng.close()

    # process_folder: stand-in segmentor, DeepFlow, the walk's own threads; HDF5 writer stubbed
    tmp = tempfile.mkdtemp(prefix="teeflow_masks_")
    src = os.path.join(tmp, "in")
    os.makedirs(src)
    from tee_optical_flow_amd.synth import speckle_sequence
    for k in range(a.studies):
        g = speckle_sequence(700 + k, a.frames, 512, 512)
        np.savez(os.path.join(src, f"study{k:02d}.npz"), nparr=np.repeat(g[..., None], 3, axis=3), pixel_spacing=0.04, frame_rate=50.0)
    real_write = hdf5_out.save_optical_flow_to_hdf5
    hdf5_out.save_optical_flow_to_hdf5 = lambda *args, **kw: None
    sam = _FakeSam()
    model = P.make_flow_model("deepflow")
    saved = T.DenseFlow.clean_masks
    say(f"process_folder, {a.studies} studies of {a.frames} frames 512x512, mode RVIO_2class with a stand-in segmentor (torch on the host), "
        f"DeepFlow, workers='thread', HDF5 write stubbed")
    try:
        kw = dict(nchunks=1, chunk_index=0, mode="RVIO_2class", verbose=False, extensions=("npz",), OF_algo="deepflow", flow_model=model,
                  workers="thread", recalculate=True)
        P.process_folder(src, os.path.join(tmp, "warm"), sam, studies_in_flight=2, **kw)
        for wired in (False, True, False, True):
            for sif in (1, 2):
                if not wired:
                    del T.DenseFlow.clean_masks                           # the walk before the wiring: masks cleaned on the host
                try:
                    ab0 = model.counter("coop_aborts")
                    t = time.perf_counter()
                    errs = P.process_folder(src, os.path.join(tmp, "out"), sam, studies_in_flight=sif, **kw)
                    dt = time.perf_counter() - t
                finally:
                    T.DenseFlow.clean_masks = saved
                say(f"  masks on the {'device' if wired else 'host  '}  studies_in_flight={sif}: {dt / a.studies * 1e3:8.1f} ms per study  "
                    f"coop_aborts {model.counter('coop_aborts') - ab0}  errors {errs}")
        say(f"  coop_launches of the engine: {model.counter('coop_launches')}")
    finally:
        T.DenseFlow.clean_masks = saved
        hdf5_out.save_optical_flow_to_hdf5 = real_write
        model.close()
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
