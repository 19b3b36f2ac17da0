#!/usr/bin/env python3
"""Compressing one 65-frame study's datasets into the gzip-9 chunks of its file, at 512x512 and 600x800, timed three ways that are
interleaved in one process:
    host1   zlib.compress(chunk, 9) of every chunk of flow, echo and the Otsu mask on this thread: what create_gzip9 does on one
            thread, less the HDF5 write
    host    the same in create_gzip9's thread pool (hdf5_out._workers(): 16 threads where there are 16 cores): the yardstick
    device  DenseFlow.held_deflate of the three arrays of the held payload, the download of the streams included
    mixed   held_deflate of flow and echo, the mask in the host's thread pool behind them: what process_video(deflate="device") does
The study is made here, without h5py: flows and echo from the solver on a speckle sequence (calc_study_payload(hold=True)), the mask
from the Otsu mode (held under "otsu"), in the chunk shapes h5py would pick (tools/held_inflate_bench.py's auto_chunks).  Median of
--reps after a warm-up; the device's streams are checked equal to the host's, chunk by chunk.  device also gives its time per dataset
and the library's counter split: match (links and match search), emit (parse, trees, bits, compaction), chunk (the gather).  Prints one
JSON line per size and writes them to --out (default profiles/r22_deflate.txt, replaced by every run).
    python tools/deflate_bench.py [--reps 5] [--out profiles/r22_deflate.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from held_inflate_bench import auto_chunks, deflate_dataset  # noqa: E402

COUNTERS = ("deflate_match_us", "deflate_emit_us", "chunk_kernel_us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_deflate.txt"))
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import analysis as A
    from tee_optical_flow_amd.hdf5_out import _workers
    from tee_optical_flow_amd.synth import speckle_sequence
    eng = T.DenseFlow(device_id=0)
    lines = []
    for H, W in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        N = a.frames
        rgb = np.ascontiguousarray(np.repeat(speckle_sequence(N + H, N, H, W)[..., None], 3, axis=3))
        flow, echo = eng.calc_study_payload(rgb, scale=50.0, hold=True)
        arrays = {"flow": flow, "echo": echo, "otsu": np.asarray(eng.otsu_masks(rgb, 64))}
        eng.hold_mask("otsu", arrays["otsu"])
        chunkings = {k: auto_chunks(arr.shape, arr.dtype.itemsize) for k, arr in arrays.items()}
        got = {}

        per, per_host, kern = {k: [] for k in arrays}, {k: [] for k in arrays}, {}

        def host(workers):
            got["host"] = {}
            for k, arr in arrays.items():
                t = time.perf_counter()
                got["host"][k] = A.chunks_record(arr.shape, arr.dtype, chunkings[k], deflate_dataset(arr, workers)[0])
                if workers > 1:
                    per_host[k].append((time.perf_counter() - t) * 1e3)

        def mixed():
            got["mixed"] = {k: eng.held_deflate(k, chunkings[k]) for k in ("flow", "echo")}
            got["mixed"]["otsu"] = A.chunks_record(arrays["otsu"].shape, arrays["otsu"].dtype, chunkings["otsu"], deflate_dataset(arrays["otsu"], _workers())[0])

        def device():
            c0 = [eng.counter(c) for c in COUNTERS]
            got["device"] = {}
            for k in arrays:
                t = time.perf_counter()
                got["device"][k] = eng.held_deflate(k, chunkings[k])
                per[k].append((time.perf_counter() - t) * 1e3)
            kern.update({c[:-3] + "_ms": round((eng.counter(c) - k0) / 1e3, 1) for c, k0 in zip(COUNTERS, c0)})

        ways = (("host1", lambda: host(1)), ("host", lambda: host(_workers())), ("device", device), ("mixed", mixed))
        times, equal = {k: [] for k, _ in ways}, True
        for rep in range(a.reps + 1):                         # rep 0: the warm-up, and the comparison of the streams
            for name, fn in ways:
                t = time.perf_counter(); fn(); dt = time.perf_counter() - t
                if rep:
                    times[name].append(dt * 1e3)
            if rep == 0:
                for k in arrays:
                    for d in (got["device"][k], got["mixed"][k]):
                        equal = equal and all(np.array_equal(np.asarray(got["host"][k][f]).reshape(-1), np.asarray(d[f]).reshape(-1)) for f in ("coord", "off", "len", "blob"))
                for k in arrays:
                    per[k].clear()
                    per_host[k].clear()
            print(f"# {H}x{W} rep {rep}: " + ", ".join(f"{k} {times[k][-1]:.0f} ms" for k, _ in ways if times[k]), flush=True)
        res = {"what": "deflate one study's datasets into gzip-9 chunks", "size": f"{H}x{W}", "frames": N, "reps": a.reps, "streams_equal": bool(equal),
               "raw_mb": round(sum(arr.nbytes for arr in arrays.values()) / 1e6, 1),
               "compressed_mb": round(sum(r["blob"].size for r in got["host"].values()) / 1e6, 1),
               "chunks": {k: [len(got["host"][k]["len"]), list(chunkings[k])] for k in arrays}, "host_threads": _workers()}
        for name, _ in ways:
            res[name] = {"ms": round(float(np.median(times[name])), 1), "ms_min": round(min(times[name]), 1), "ms_max": round(max(times[name]), 1)}
        res["device"]["per_dataset_ms"] = {k: round(float(np.median(v)), 1) for k, v in per.items()}
        res["host"]["per_dataset_ms"] = {k: round(float(np.median(v)), 1) for k, v in per_host.items()}
        res["mixed_over_host"] = round(res["mixed"]["ms"] / res["host"]["ms"], 3)
        res["device"]["kernel_ms"] = kern
        res["device_over_host1"] = round(res["device"]["ms"] / res["host1"]["ms"], 3)
        res["device_over_host"] = round(res["device"]["ms"] / res["host"]["ms"], 3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        eng.release_study()
    eng.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln)["streams_equal"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
