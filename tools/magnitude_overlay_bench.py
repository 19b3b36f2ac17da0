#!/usr/bin/env python3
"""The magnitude overlay frames of one 65-frame study (the reference's single-component video, example_peak_plots.py:459-513, the video
writer left out), at 512x512 and 600x800, float16 flow and echo as the study file holds them, host uint8 frames out.  Three ways,
interleaved on the same box:
  device  analysis.magnitude_overlay(ds, 'velocity', 'rv', engine=): host arrays in, transfers included
  held    the same of a HeldStudy: the flow, the mask and the echo are on the device already; the frames still come back
  host    the numpy twin (param_field over all frames + magnitude_overlay_host)
Checks bit-equality first, then takes the median of `--reps` after a warm-up.  Prints a text report; `--out FILE` appends it to FILE.
    python tools/magnitude_overlay_bench.py [--reps 5] [--out FILE]
`--profile-call SIZE` (512x512 | 600x800) makes only warmed held calls at that size -- the magnitude overlay, and tf_radlong_overlay of
the same study on resident planes, the yardstick: the two move comparable bytes -- for a kernel trace in a run of its own;
`--trace-summary DIR` then reads that run's kernel statistics and prints (and appends to `--out`) the kernels' device time per call,
side by side:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/magnitude_overlay_bench.py --profile-call 600x800
    python tools/magnitude_overlay_bench.py --profile-call 600x800 --trace-summary <dir> [--out FILE]
profiles/r21_magnitude_overlay.txt is the reports of one session, one after the other."""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"512x512": (512, 512), "600x800": (600, 800)}
HBM_PEAK = 8.0e12


def make_study(seed, N, H, W):
    """speckle flow (float16), an rv disc that drifts, a float16 echo of 256 grey levels; centroids for the rad/long yardstick"""
    import tee_optical_flow_amd as T
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    amp = np.concatenate([[1.0], rng.uniform(1, 4, N - 1)])[:, None, None, None]
    flow = (rng.normal(0, 2, (N, H, W, 2)) * amp).astype(np.float16)
    rv = np.zeros((N, H, W), bool)
    for f in range(N):
        rv[f] = ((yy - H / 2 - f) / (0.35 * H)) ** 2 + ((xx - W / 2 + f) / (0.4 * W)) ** 2 < 1
    echo = rng.integers(0, 256, (N, H, W)).astype(np.float16)
    rv = np.stack([rv, rv], -1)
    cent = [(H / 3 + 0.1 * f, W / 2 - 0.1 * f) for f in range(N - 2)]
    return T.FlowStudy(flow, {"rv": rv, "av": rv}, 50.0, echo=echo), cent


def med(ts):
    return f"{np.median(ts) * 1e3:8.1f} ms ({min(ts) * 1e3:.1f}-{max(ts) * 1e3:.1f})"


def emit(lines, out):
    text = "\n".join(lines)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def trace_summary(directory, size, frames, reps, out):
    """the kernel statistics rocprofv3 --kernel-trace --stats left under `directory` for a --profile-call run of the same size / frames / reps"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit(f"expected one *kernel_stats.csv under {directory}, found {files}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    H, W = SIZES[size]
    N, n = frames, frames - 2
    calls = 1 + reps
    lines = [f"kernel trace, {frames}x{size}: {calls} held calls each (1 warm-up + {reps}) of the magnitude overlay (velocity) and of tf_radlong_overlay on "
             f"resident planes, {n} frames rendered; device time of the kernels per call"]
    totals = {}
    for fam, what in (("k_mo_", "tf_held_magnitude_overlay"), ("k_ov_", "tf_held_radlong_overlay")):
        hit = [r for r in rows if fam in r["Name"]]
        if not hit:
            raise SystemExit(f"{files[0]}: no {fam}* kernel")
        tot = 0.0
        lines.append(f"  {what}:")
        for r in sorted(hit, key=lambda r: r["Name"]):
            per_call = float(r["AverageNs"]) * int(r["Calls"]) / calls * 1e-9
            tot += per_call
            lines.append(f"    {r['Name'][r['Name'].find(fam):].split('(')[0][:44]:<44} launches {int(r['Calls']):4d}  {per_call * 1e6:8.1f} us per call")
        totals[fam] = tot
    px, PX = n * H * W, N * H * W
    mo_bytes = PX * (4 + 2) + px * (4 + 2 + 1) + px * 2 + px * (1 + 2 + 3)     # range; index (+ 1 B written); echo maxima; compose
    ov_bytes = px * (16 + 2) + px * 2 + px * (2 + 2 + 6)                         # index; echo maximum; compose
    for fam, b, what in (("k_mo_", mo_bytes, "flow 4 B + mask 2 B over all frames, again over the frames rendered, 1 B of index out and in, echo 2 B twice, 3 B out"),
                         ("k_ov_", ov_bytes, "planes 16 B, 2 B of indices out and in, echo 2 B twice, 6 B out")):
        bw = b / totals[fam]
        lines.append(f"  {fam}* total {totals[fam] * 1e6:8.0f} us per call for {b / 1e6:.0f} MB it moves ({what}) = {bw / 1e12:.2f} TB/s = "
                     f"{100 * bw / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak")
    lines.append(f"  magnitude overlay / rad-long overlay kernels: {totals['k_mo_'] / totals['k_ov_']:.2f}x the device time, "
                 f"{mo_bytes / ov_bytes:.2f}x the bytes")
    emit(lines, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--profile-call", choices=sorted(SIZES))
    ap.add_argument("--trace-summary", metavar="DIR", help="with --profile-call: summarise the kernel statistics of that run's rocprofv3 output, no GPU work")
    ap.add_argument("--out", help="append the report to this file as well")
    a = ap.parse_args()
    if a.trace_summary:
        if not a.profile_call:
            ap.error("--trace-summary needs --profile-call SIZE (the size of the traced run)")
        return trace_summary(a.trace_summary, a.profile_call, a.frames, a.reps, a.out)
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import analysis as A
    hot = A.magnitude_colormap_lut("hot")
    eng = T.DenseFlow(device_id=0)
    if a.profile_call:
        H, W = SIZES[a.profile_call]
        st, cent = make_study(a.frames + H + W, a.frames, H, W)
        n = st.nframes
        A.HeldStudy.from_study(eng, st)
        eng.held_radlong_project_param("rv", 0, 1 / 50.0, False, n, cent)
        lr, ll = A.colormap_lut("bwr"), A.colormap_lut("BrBG")
        for _ in range(1 + a.reps):
            eng.held_magnitude_overlay("rv", 0, 1 / 50.0, False, A.norm_is_f64(), n, hot)
            eng.held_radlong_overlay(lr, ll)
        print(f"{a.profile_call}: {1 + a.reps} held calls each of the magnitude overlay and the rad/long overlay, {n} of {a.frames} frames rendered")
        eng.close()
        return
    lines = ["magnitude overlay frames of one study: device (host arrays in, transfers included), held study, host (numpy twin); host uint8 frames out; "
             f"float16 flow and echo, {a.frames} frames ({a.frames - 2} rendered), velocity, rv mask, colormap hot"]
    for name, (H, W) in SIZES.items():
        st, _ = make_study(a.frames + H + W, a.frames, H, W)
        n = st.nframes
        small, _ = make_study(1, 6, 64, 64)
        A.magnitude_overlay(small, "velocity", "rv")                                            # warm-up of all three
        A.magnitude_overlay(small, "velocity", "rv", engine=eng)
        held = A.HeldStudy.from_study(eng, st)
        dev = A.magnitude_overlay(st, "velocity", "rv", engine=eng)
        hld = A.magnitude_overlay(held, "velocity", "rv", engine=eng)
        host = A.magnitude_overlay(st, "velocity", "rv")
        equal = bool(np.array_equal(dev, host) and np.array_equal(hld, host))
        td, th, tt = [], [], []
        for _ in range(a.reps):
            t = time.perf_counter(); d = A.magnitude_overlay(st, "velocity", "rv", engine=eng); td.append(time.perf_counter() - t)
            t = time.perf_counter(); k = A.magnitude_overlay(held, "velocity", "rv", engine=eng); th.append(time.perf_counter() - t)
            t = time.perf_counter(); w = A.magnitude_overlay(st, "velocity", "rv"); tt.append(time.perf_counter() - t)
            equal = equal and bool(np.array_equal(d, w) and np.array_equal(k, w))
            del d, k, w
        up = a.frames * H * W * (4 + 2) + n * H * W * 2
        lines.append(f"  {a.frames}x{name}: device {med(td)}  held {med(th)}  host {med(tt)}  speed-up {np.median(tt) / np.median(td):6.1f}x / "
                     f"{np.median(tt) / np.median(th):6.1f}x  bit-equal {equal}  (median of {a.reps}; {up / 1e6:.0f} MB uploaded by the device way, "
                     f"{n * H * W * 3 / 1e6:.0f} MB of frames downloaded by both)")
        eng.release_study()
    eng.close()
    emit(lines, a.out)


if __name__ == "__main__":
    main()
