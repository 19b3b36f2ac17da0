#!/usr/bin/env python3
"""A study solved as a chain (DenseFlow's chain=True, tf_chain_next: every pair starts from the flow before it) against the same study
solved as a batch, interleaved in one process on one GPU (DualTVL1 at its default parameters, calc_study_payload with scale = 0.04 * 50):
  (p) calc_study_payload(rgb): all N-1 pairs in lock-step;
  (c) calc_study_payload(rgb, chain=True): N-1 single-pair solves, one after the other, on the device;
  (3) three chained studies: submit_study_payload(chain=True) x 3 then the three waits (one lane each), against three calls of (c).
The yardstick is (p) of the same run; no threshold.  Each form gets one warm-up, then `--reps` timed rounds p, c, 3-together, 3-in-turn;
printed are the median and min-max of the host clock, and the executed inner iterations per pair (last_iters()) of (p) and (c).
usage: python3 tools/chain_bench.py [--frames 65] [--sizes 512x512,600x800] [--reps 5]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE = 0.04 * 50


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
    inner = {}

    def plain(rgb):
        eng.setUseInitialFlow(False)
        out = eng.calc_study_payload(rgb, scale=SCALE)[0]
        inner["p"] = eng.last_iters()[..., 0].sum(axis=(1, 2))
        return out

    def chained(rgb, record=False):
        eng.setUseInitialFlow(True)
        out = eng.calc_study_payload(rgb, scale=SCALE, chain=True)[0]
        if record:
            inner["c"] = eng.last_iters()[..., 0].sum(axis=(1, 2))
        return out

    def together(studies):
        eng.setUseInitialFlow(True)
        tickets = [eng.submit_study_payload(s, scale=SCALE, chain=True) for s in studies]
        return [eng.wait(t)[0] for t in tickets]

    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        N = a.frames
        studies = [np.ascontiguousarray(np.repeat(speckle_sequence(3 + i, N, H, W)[..., None], 3, axis=3)) for i in range(3)]
        rgb = studies[0]
        forms = {
            "p  calc_study_payload": lambda: plain(rgb),
            "c  calc_study_payload(chain=True)": lambda: chained(rgb, record=True),
            "3  three chained studies submitted together": lambda: together(studies),
            "3s three chained studies one after another": lambda: [chained(s) for s in studies],
        }
        first = {k: f() for k, f in forms.items()}                                  # warm-up of every form, and the agreement
        kp, kc, k3, k3s = forms
        d = first[kc].astype(np.float32) - first[kp].astype(np.float32)
        if not (np.array_equal(first[kc][0], first[kp][0]) and all(np.array_equal(x, y) for x, y in zip(first[k3], first[k3s]))):
            print(f"{N} frames {H}x{W}: pair 0 of the chain is not the plain solve, or submitted chains differ from waited ones: nothing timed")
            eng.close()
            return 1
        epe = np.sqrt((d[1:N - 1] ** 2).sum(-1)).mean() / SCALE
        del first, d
        wall = {k: [] for k in forms}
        for _ in range(a.reps):
            for k, f in forms.items():
                t0 = time.perf_counter()
                f()
                wall[k].append(time.perf_counter() - t0)
        print(f"{N} frames {H}x{W}, DualTVL1, scale {SCALE}; pair 0 equal in bits, pairs 1.. differ by {epe:.4f} px mean (float16 payloads); "
              f"median of {a.reps} (min-max), one warm-up each")
        for k in forms:
            print(f"  {k:48s} {stats(wall[k])}")
        mp, mc, m3, m3s = (float(np.median(wall[k])) for k in (kp, kc, k3, k3s))
        print(f"  c / p = {mc / mp:.2f}   per chained pair {mc * 1e3 / (N - 1):.2f} ms   together / one after another = {m3 / m3s:.2f}")
        print(f"  executed inner iterations per pair, pairs 1..{N - 2}: plain mean {inner['p'][1:].mean():.1f}, chained mean {inner['c'][1:].mean():.1f} "
              f"(sum {int(inner['p'][1:].sum())} against {int(inner['c'][1:].sum())})")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
