#!/usr/bin/env python3
"""The rad/long overlay frames of one 65-frame study (visualize_radlong's per-pixel part, the video writer left out), at 512x512 and
600x800, float16 flow and echo as the study file holds them, AV centroids given: the numpy twin on the host against the device, on
the same box, host arrays in and host frames out, transfers included.  Two figures per size:
  whole   analysis.radlong_overlay(ds, 'velocity'): the param field and the rad/long projection, then the frames
  frames  the rendering alone: analysis.overlay_host on host planes against DenseFlow.radlong_overlay on the resident planes
Checks bit-equality first, then alternates host and device after a warm-up and takes the median.  Prints a text report; `--out FILE`
appends it to FILE as well.
    python tools/overlay_bench.py [--reps 5] [--out FILE]
`--profile-call SIZE` (512x512 | 600x800) makes only warmed device calls of the rendering at that size, for a kernel trace in a run of
its own; `--trace-summary DIR` then reads that run's kernel statistics and prints (and appends to `--out`) each kernel's time against
its compulsory bytes and the 8.0 TB/s HBM peak:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/overlay_bench.py --profile-call 600x800
    python tools/overlay_bench.py --profile-call 600x800 --trace-summary <dir> [--out FILE]
profiles/r10_overlay.txt is the three reports of one session, one after the other."""
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


def make_study(seed, N, H, W):
    """speckle flow (float16) that is quiet in frame 0, an rv disc that drifts, a float16 echo of 256 grey levels"""
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
    n = N - 2
    cent = [(H / 3 + 0.1 * f, W / 2 - 0.1 * f) for f in range(n)]
    return T.FlowStudy(flow, {"rv": rv, "av": rv}, 50.0, echo=echo), cent


def med(ts):
    return f"{np.median(ts) * 1e3:8.1f} ms ({min(ts) * 1e3:.1f}-{max(ts) * 1e3:.1f})"


HBM_PEAK = 8.0e12
# compulsory bytes per pixel of the study (n * H * W) and what they are
KERNELS = (("k_ov_compose", 10, "2 B indices + 2 B echo in (each read by both of a pixel's slots: 8 B requested), 6 B out"),
           ("k_ov_index", 18, "16 B of planes in, 2 B of indices out"),
           ("k_ov_echo", 2, "2 B of echo in"),
           ("k_ov_half", 0, "frame 0 of one plane only"))


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
    px = (frames - 2) * H * W
    calls = 1 + reps
    avg = {}
    for name, _, _ in KERNELS:
        hit = [r for r in rows if name in r["Name"]]
        if len(hit) != 1 or int(hit[0]["Calls"]) != calls:
            raise SystemExit(f"{files[0]}: expected one row of {calls} calls for {name}, got {hit}")
        avg[name] = float(hit[0]["AverageNs"]) * 1e-9
    total = sum(avg.values())
    lines = [f"kernel trace, {frames}x{size}: {calls} calls of DenseFlow.radlong_overlay (1 warm-up + {reps}) on resident planes, {px} pixels per call, "
             f"kernel time {total * 1e6:.0f} us per call (the call itself: see 'frames' above; the rest is the two copies over PCIe)"]
    for name, bpp, what in KERNELS:
        if bpp:
            bw = bpp * px / avg[name]
            lines.append(f"  {name:<13}{avg[name] * 1e6:8.1f} us  {bpp:2d} B per pixel compulsory ({what}): {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_PEAK:4.1f} % of the 8.0 TB/s HBM peak")
        else:
            lines.append(f"  {name:<13}{avg[name] * 1e6:8.1f} us  {what}")
    bw = 24 * px / total
    lines.append(f"  the rendering as a whole: {total * 1e6:.0f} us for the 24 B per pixel it cannot avoid (16 B of planes + 2 B of echo in, 6 B out) = "
                 f"{bw / 1e12:.2f} TB/s = {100 * bw / HBM_PEAK:.1f} % of peak; with the 2-byte index scratch written and read back and the echo read twice it moves 30 B per pixel")
    for r in sorted(rows, key=lambda r: -float(r["Percentage"]))[:8]:
        lines.append(f"    {r['Name'][:58]:<58} calls {int(r['Calls']):3d}  avg {float(r['AverageNs']) / 1e3:8.1f} us  {float(r['Percentage']):5.2f} %")
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
    lr, ll = A.colormap_lut("bwr"), A.colormap_lut("BrBG")
    eng = T.DenseFlow(device_id=0)
    if a.profile_call:
        H, W = SIZES[a.profile_call]
        st, cent = make_study(a.frames + H + W, a.frames, H, W)
        n = st.nframes
        eng.radlong_project_param(st.flow, st.get_mask("rv"), 0, 1 / 50.0, False, n, cent)
        for _ in range(1 + a.reps):
            eng.radlong_overlay(st.echo, lr, ll)
        px = n * H * W
        print(f"{a.profile_call}: {1 + a.reps} calls of DenseFlow.radlong_overlay (1 warm-up + {a.reps}), {px} pixels per call; compulsory bytes per call: "
              f"k_ov_index {16 * px} in + {2 * px} out, k_ov_echo {2 * px} in, k_ov_compose {4 * px} in + {6 * px} out; "
              f"the rendering as one pass would need {18 * px} in + {6 * px} out")
        eng.close()
        return
    lines = ["radlong overlay frames of one study, host (numpy twin) vs device, host arrays in, host uint8 frames out, transfers included; "
             f"float16 flow and echo, {a.frames} frames ({a.frames - 2} used), colormaps bwr / BrBG"]
    for name, (H, W) in SIZES.items():
        st, cent = make_study(a.frames + H + W, a.frames, H, W)
        n = st.nframes
        small, scent = make_study(1, 6, 64, 64)
        A.radlong_overlay(small, "velocity", centroids=scent)                                   # warm-up of both
        dev = A.radlong_overlay(st, "velocity", centroids=cent, engine=eng)
        host = A.radlong_overlay(st, "velocity", centroids=cent)
        equal = bool(np.array_equal(dev, host))
        rad, lon = A.calculate_comp_magnitude(A.param_field(st.flow, st.get_mask("rv"), "velocity", st.frame_rate, n), cent)
        wh, wd, fh, fd = [], [], [], []
        for _ in range(a.reps):
            t = time.perf_counter(); h = A.radlong_overlay(st, "velocity", centroids=cent); wh.append(time.perf_counter() - t)
            t = time.perf_counter(); d = A.radlong_overlay(st, "velocity", centroids=cent, engine=eng); wd.append(time.perf_counter() - t)
            equal = equal and bool(np.array_equal(h, d))
            t = time.perf_counter(); h2, _ = A.overlay_host(rad, lon, st.echo, lr, ll); fh.append(time.perf_counter() - t)
            t = time.perf_counter(); d2, _ = eng.radlong_overlay(st.echo, lr, ll); fd.append(time.perf_counter() - t)   # host-synchronous
            equal = equal and bool(np.array_equal(h2, d2)) and bool(np.array_equal(h2, h))
            del h, d, h2, d2
        lines.append(f"  {a.frames}x{name} whole : host {med(wh)}  device {med(wd)}  speed-up {np.median(wh) / np.median(wd):6.1f}x  bit-equal {equal}  (median of {a.reps})")
        lines.append(f"  {a.frames}x{name} frames: host {med(fh)}  device {med(fd)}  speed-up {np.median(fh) / np.median(fd):6.1f}x  "
                     f"({n * H * W * 6 / 1e6:.0f} MB of frames downloaded, {n * H * W * 2 / 1e6:.0f} MB of echo uploaded per call)")
    eng.close()
    emit(lines, a.out)


if __name__ == "__main__":
    main()
