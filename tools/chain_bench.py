#!/usr/bin/env python3
"""A study solved as a chain (DenseFlow's chain=True, tf_chain_next: every pair starts from the flow before it) against the same study
solved as a batch, interleaved in one process on one GPU (DualTVL1 at its default parameters, calc_study_payload with scale = 0.04 * 50):
  (p) calc_study_payload(rgb): all N-1 pairs in lock-step;
  (c) calc_study_payload(rgb, chain=True): N-1 single-pair solves, one after the other, on the device;
  (3) three chained studies: submit_study_payload(chain=True) x 3 then the three waits (one lane each), against three calls of (c).
The yardstick is (p) of the same run; no threshold.  Each form gets one warm-up, then `--reps` timed rounds p, c, 3-together, 3-in-turn;
printed are the median and min-max of the host clock, and the executed inner iterations per pair (last_iters()) of (p) and (c).
usage: python3 tools/chain_bench.py [--frames 65] [--sizes 512x512,600x800] [--reps 5]

--lockstep: S = 2, 4, 8 studies of one frame size as chains in lock-step (calc_study_chains_payload, tf_calc_chains_rgb: step k solves pair
k of every study as one batch) against the two forms there were before, interleaved in one process, one warm-up of each form, then
`--reps` timed rounds 1, 2, 3; the warm-up's results must be equal in bits between the three forms, else nothing is timed:
  (1) one lock-step call of the S studies;
  (2) S calls of calc_study_payload(chain=True), one after another;
  (3) the same S studies submitted together, submit_study_payload(chain=True) x S then the waits (one lane each, three lanes).
No threshold: printed are the median and min-max of the host clock and the ratios (1)/(2) and (1)/(3).  The lines, with a header that
says what was run, when and (`--note`) where, also go to `--out` (default profiles/r19_chains_lockstep.txt, overwritten: the tool
writes the whole file).
usage: python3 tools/chain_bench.py --lockstep [--frames 65] [--sizes 512x512,600x800] [--reps 5] [--chains 2,4,8] [--out FILE] [--note TEXT]"""
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


def lockstep(a):
    from tee_optical_flow_amd.synth import speckle_sequence
    import tee_optical_flow_amd as T
    counts = [int(v) for v in a.chains.split(",")]
    eng = T.DenseFlow()
    eng.setUseInitialFlow(True)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    # the file's header: what was run, when and (--note) where; everything in the file is written here
    say("# S studies of one frame size solved as chains in lock-step (tf_calc_chains_rgb, DenseFlow.calc_study_chains_payload: step k solves")
    say("# pair k of every study as one batch) against the two forms there were before.  Written by tools/chain_bench.py --lockstep, "
        f"{time.strftime('%Y-%m-%d')}" + (f"; {a.note}" if a.note else "") + ".")
    say(f"# {a.frames} frames per study, DualTVL1 at its default parameters, float16 payloads with echo, scale = 0.04 * 50; the three forms")
    say(f"# interleaved in one process, median of {a.reps} (min-max) after one warm-up each, whose flows must be equal in bits between the forms.")
    say("#   (1) one lock-step call of the S studies;")
    say("#   (2) S calls of calc_study_payload(chain=True), one after another;")
    say("#   (3) the same S studies submitted together, submit_study_payload(chain=True) x S then the waits (three lanes).")
    say("# No threshold is set.  The copy-out of (1) is in order on the solve stream, its uploads and conditioning are study after study.")

    def together(studies):
        tickets = [eng.submit_study_payload(s, scale=SCALE, chain=True) for s in studies]
        return [eng.wait(t)[0] for t in tickets]

    rc = 0
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        N = a.frames
        every = [np.ascontiguousarray(np.repeat(speckle_sequence(3 + i, N, H, W)[..., None], 3, axis=3)) for i in range(max(counts))]
        for S in counts:
            studies = every[:S]
            forms = {
                "1  one lock-step call": lambda: [f for f, _ in eng.calc_study_chains_payload(studies, scale=SCALE)],
                f"2  {S} chained calls one after another": lambda: [eng.calc_study_payload(s, scale=SCALE, chain=True)[0] for s in studies],
                f"3  {S} chained studies submitted together": lambda: together(studies),
            }
            first = {k: f() for k, f in forms.items()}                              # warm-up of every form, and the agreement
            k1, k2, k3 = forms
            if not all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(first[k1], first[k2], first[k3])):
                say(f"{S} studies of {N} frames {H}x{W}: the three forms' flows differ: nothing timed")
                rc = 1
                continue
            del first
            wall = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, f in forms.items():
                    t0 = time.perf_counter()
                    f()
                    wall[k].append(time.perf_counter() - t0)
            say(f"{S} studies of {N} frames {H}x{W}, DualTVL1, scale {SCALE}, float16 payloads with echo; the three forms' flows equal in bits; "
                f"median of {a.reps} (min-max), one warm-up each")
            for k in forms:
                say(f"  {k:48s} {stats(wall[k])}")
            m1, m2, m3 = (float(np.median(wall[k])) for k in (k1, k2, k3))
            say(f"  (1) / (2) = {m1 / m2:.2f}   (1) / (3) = {m1 / m3:.2f}   per pair: (1) {m1 * 1e3 / (S * (N - 1)):.2f} ms, (2) {m2 * 1e3 / (S * (N - 1)):.2f} ms, "
                f"(3) {m3 * 1e3 / (S * (N - 1)):.2f} ms")
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65)
    ap.add_argument("--sizes", default="512x512,600x800")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lockstep", action="store_true", help="time S studies as chains in lock-step against the two forms there were before")
    ap.add_argument("--chains", default="2,4,8", help="--lockstep: the numbers of studies S")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_chains_lockstep.txt"),
                    help="--lockstep: the file that gets the printed lines, header included (it is overwritten)")
    ap.add_argument("--note", default="", help="--lockstep: where this was run, for the file's header, e.g. 'one MI355X, 16 CPUs for the command'")
    a = ap.parse_args()
    if a.lockstep:
        return lockstep(a)
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
