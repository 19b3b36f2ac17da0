#!/usr/bin/env python3
"""Holding one 65-frame study from the gzip chunks of its file, at 512x512 and 600x800, timed three ways that are interleaved in one
process:
    serial  zlib.decompress of every chunk on this thread + assembly + hold_study / hold_mask: what HeldStudy.from_hdf5(inflate="h5py")
            does, less the file read
    host    the same with the chunks inflated in a thread pool (analysis.unchunk_host), inflate="host"
    device  the compressed chunks uploaded and inflated on the device (hold_study_chunks / hold_mask_chunks), inflate="device"
The study is made here, without h5py: flows from the solver on a speckle sequence, the mask from the Otsu mode, every dataset deflated
at level 9 in the chunk shape h5py would pick for it (auto_chunks: h5py's documented rule, restated).  Median of --reps after a warm-up;
the held results of the three ways are checked bit-equal (first-region areas, a polar and a rad/long projection, the overlay).  The
yardsticks are `serial` and `host`; `device` alone says nothing.  kernel_ms is the device time of k_inflate / k_unchunk in one
`device` hold, from the library's events.  Prints one JSON line per size and writes them to --out (default
profiles/r20_held_inflate.txt, replaced by every run).
    python tools/held_inflate_bench.py [--reps 5] [--out profiles/r20_held_inflate.txt]"""
import argparse
import itertools
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def auto_chunks(shape, itemsize):
    """the chunk shape h5py picks for a dataset without one: halve the dimensions in turn, from the first, until a chunk is within
    half of a target size that grows with the dataset (16 KiB at 1 MiB, doubling per decade, within 8 KiB .. 1 MiB)"""
    chunks = np.array(shape, dtype="=f8")
    dset = np.prod(chunks) * itemsize
    target = min(max(16384 * 2 ** np.log10(dset / (1024.0 * 1024)), 8192), 1 << 20)
    for idx in itertools.count():
        size = np.prod(chunks) * itemsize
        if (size < target or abs(size - target) / target < 0.5) and size < (1 << 20):
            break
        if np.prod(chunks) == 1:
            break
        chunks[idx % len(shape)] = np.ceil(chunks[idx % len(shape)] / 2.0)
    return tuple(int(x) for x in chunks)


def deflate_dataset(arr, workers):
    """[(coord, 0, level-9 stream)] of arr's chunks as a file holds them (edge chunks whole, zero-padded), and the chunk shape"""
    ch = auto_chunks(arr.shape, arr.dtype.itemsize)
    coords = list(itertools.product(*[range(0, s, c) for s, c in zip(arr.shape, ch)]))

    def one(at):
        blk = arr[tuple(slice(o, min(o + c, s)) for o, c, s in zip(at, ch, arr.shape))]
        if blk.shape != ch:
            full = np.zeros(ch, arr.dtype)
            full[tuple(slice(0, n) for n in blk.shape)] = blk
            blk = full
        return at, 0, zlib.compress(np.ascontiguousarray(blk), 9)
    with ThreadPoolExecutor(workers) as pool:
        return list(pool.map(one, coords)), ch


def check(eng, N, lut):
    """a few held results that read the flow, the mask and the echo"""
    out = [eng.held_first_region_areas("otsu", N)]
    out += list(eng.held_polar_project_param("otsu", 0, 1 / 50.0, True, N))
    out += list(eng.held_radlong_project_param("otsu", 1, 1 / 50.0, True, N - 2, np.full((N - 2, 2), 200.0)))
    out += list(eng.held_radlong_overlay(*lut))
    return [np.asarray(x) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_held_inflate.txt"))
    a = ap.parse_args()
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import analysis as A
    from tee_optical_flow_amd.hdf5_out import _workers
    from tee_optical_flow_amd.synth import speckle_sequence
    eng = T.DenseFlow(device_id=0)
    luts = A.committed_colormap_luts()
    lut = (luts["bwr"], luts["BrBG"])
    lines = []
    for H, W in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        N = a.frames
        rgb = np.ascontiguousarray(np.repeat(speckle_sequence(N + H, N, H, W)[..., None], 3, axis=3))
        flow, echo = eng.calc_study_payload(rgb, scale=50.0)
        arrays = {"flow": flow, "echo": echo, "otsu": np.asarray(eng.otsu_masks(rgb, 64))}
        recs, raw_mb, comp_mb, chunks = {}, 0.0, 0.0, {}
        for k, arr in arrays.items():
            stored, ch = deflate_dataset(arr, _workers())
            recs[k] = A.chunks_record(arr.shape, arr.dtype, ch, stored)
            raw_mb += arr.nbytes / 1e6
            comp_mb += recs[k]["blob"].size / 1e6
            chunks[k] = [len(stored), list(ch)]

        def from_arrays(workers):
            got = {k: A.unchunk_host(r, workers=workers) for k, r in recs.items()}
            eng.hold_study(got["flow"], got["echo"])
            eng.hold_mask("otsu", got["otsu"])

        def device():
            eng.hold_study_chunks(recs["flow"], recs["echo"])
            eng.hold_mask_chunks("otsu", recs["otsu"])

        ways = (("serial", lambda: from_arrays(1)), ("host", lambda: from_arrays(None)), ("device", device))
        times, equal, ref, kern = {k: [] for k, _ in ways}, True, None, {}
        for rep in range(a.reps + 1):                         # rep 0: the warm-up, and the comparison of what is held
            for name, fn in ways:
                k0 = [eng.counter(c) for c in ("inflate_kernel_us", "unchunk_kernel_us")]
                t = time.perf_counter(); fn(); dt = time.perf_counter() - t
                if name == "device":
                    kern = {c: round((eng.counter(c + "_kernel_us") - k) / 1e3, 2) for c, k in zip(("inflate", "unchunk"), k0)}
                if rep == 0:
                    r = check(eng, N, lut)
                    ref = r if ref is None else ref
                    equal = equal and len(r) == len(ref) and all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(r, ref))
                else:
                    times[name].append(dt * 1e3)
        eng.release_study()
        res = {"what": "hold one study from its gzip-9 chunks", "size": f"{H}x{W}", "frames": N, "reps": a.reps, "bit_equal": bool(equal),
               "raw_mb": round(raw_mb, 1), "compressed_mb": round(comp_mb, 1), "chunks": chunks, "host_threads": _workers()}
        for name, _ in ways:
            res[name] = {"ms": round(float(np.median(times[name])), 1), "ms_min": round(min(times[name]), 1), "ms_max": round(max(times[name]), 1)}
        res["device"]["kernel_ms"] = kern
        res["device_over_serial"] = round(res["device"]["ms"] / res["serial"]["ms"], 3)
        res["device_over_host"] = round(res["device"]["ms"] / res["host"]["ms"], 3)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    eng.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(json.loads(ln)["bit_equal"] for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
