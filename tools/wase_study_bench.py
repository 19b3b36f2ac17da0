#!/usr/bin/env python3
"""A bkgd_comp="WASE" study end to end, three ways, interleaved in one process on one GPU (DualTVL1, scale = 0.04 * 50, a seeded bkgd mask
of density 0.3):
  (a) the path before the one-call forms, written out: calc_study, wase_compensate(scale=), np.concatenate of the last flow -- and, for
      the float16 comparison, the writer's .astype(np.float16) on top (a16);
  (b) calc_study_wase(pad_last=True): float32, the flows never leave the device between the solve and the compensation;
  (c) calc_study_wase_payload: the same with float16 flows and the echo.
Before anything is timed (a), (b) and (c) must agree in bits.  Each form gets one warm-up, then `--reps` timed rounds a, b, c, a, b, c, ...;
printed are the median and min-max of the host clock around each synchronous call, and the device time of the reduction plus k_wase_out
of the new call (HIP events inside the library).
usage: python3 tools/wase_study_bench.py [--frames 65] [--sizes 512x512,600x800] [--reps 5]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE = 0.04 * 50


def parent_path(eng, rgb, mask):
    flows = eng.calc_study(rgb)
    flows, _ = eng.wase_compensate(flows, mask, scale=SCALE)
    return np.concatenate([flows, flows[-1:]], axis=0)


def same_bits(a, b):
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return f"{np.median(ts):8.1f} ms ({ts.min():.1f}-{ts.max():.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from tee_optical_flow_amd.synth import speckle_sequence
    import tee_optical_flow_amd as T
    eng = T.DenseFlow()
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        N = a.frames
        rgb = np.ascontiguousarray(np.repeat(speckle_sequence(3, N, H, W)[..., None], 3, axis=3))
        mask = np.random.default_rng(13).random((N, H, W, 2)) < 0.3
        mask[0] = False
        forms = {
            "a   calc_study + wase_compensate + concatenate (float32)": lambda: parent_path(eng, rgb, mask),
            "a16 ... + astype(float16)": lambda: parent_path(eng, rgb, mask).astype(np.float16),
            "b   calc_study_wase(pad_last=True) (float32)": lambda: eng.calc_study_wase(rgb, mask, scale=SCALE, pad_last=True)[0],
            "c   calc_study_wase_payload (float16 + echo)": lambda: eng.calc_study_wase_payload(rgb, mask, scale=SCALE)[0],
        }
        first = {k: f() for k, f in forms.items()}                                  # warm-up of every form, and the agreement
        ka, ka16, kb, kc = forms
        if not (same_bits(first[ka], first[kb]) and same_bits(first[ka16], first[kc]) and np.isfinite(first[kb]).all()):
            print(f"{N} frames {H}x{W}: the forms DISAGREE in bits, nothing timed")
            eng.close()
            return 1
        del first
        wall = {k: [] for k in forms}
        dev = []
        for _ in range(a.reps):
            for k, f in forms.items():
                t0 = time.perf_counter()
                f()
                wall[k].append(time.perf_counter() - t0)
                if k == kb:
                    dev.append(eng.counter("wase_study_kernel_us") * 1e-6)
        print(f"{N} frames {H}x{W}, DualTVL1, scale {SCALE}, mask density 0.3; (a)=(b) and (a16)=(c) in bits; median of {a.reps} (min-max), one warm-up each")
        for k in forms:
            print(f"  {k:58s} {stats(wall[k])}")
        ma, mb, ma16, mc = (float(np.median(wall[k])) for k in (ka, kb, ka16, kc))
        print(f"  b / a = {mb / ma:.3f}   c / a16 = {mc / ma16:.3f}   device time of the reduction + k_wase_out in (b): {stats(dev)}")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
