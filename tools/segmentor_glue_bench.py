#!/usr/bin/env python3
"""The frame glue around the SAM segmentor (evaluate_1_slice of the reference, calculate_optical_flow.py:47-88) on the host against
the device path (DenseFlow.segmentor_input / segmentor_classmap, what predict_movie(engine=) takes when the model sits on the engine's
GPU), for a study of 65 frames at 512x512 and at 600x800.  The model is a stand-in on the GPU whose three sub-modules do no arithmetic
(the encoder hands its input on, the decoder hands out fixed logits [1,3,256,256]), so what is timed is the glue: both resizes, the
normalised tensor, its upload, the argmax and its way back -- transfers included, the two paths alternating after one warm-up call,
the median of --reps calls, with bit-equality of the class maps.  Then the same with clean_mask(engine=) behind it, which is
predict_movie as the study driver calls it, and the device time of the two calls (HIP events on the stream around them, against a
plain copy of the same bytes) for the kernels' share.
    python tools/segmentor_glue_bench.py [--reps 5]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"512x512": (65, 512, 512), "600x800": (65, 600, 800)}


def study(N, H, W):
    from tee_optical_flow_amd.synth import speckle_sequence
    g = speckle_sequence(N + H + W, N, H, W)
    rng = np.random.default_rng(N + H)
    out = np.empty((N, H, W, 3), np.uint8)
    for c in range(3):
        out[..., c] = np.clip(g.astype(np.int16) + rng.integers(-12, 13, g.shape, dtype=np.int16), 0, 255)
    return out


def stand_in(torch, device):
    class Enc(torch.nn.Module):
        def forward(self, x):
            return x

    class Prompt(torch.nn.Module):
        def forward(self, points=None, boxes=None, masks=None):
            return None, None

        def get_dense_pe(self):
            return None

    class Dec(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(1)
            yy, xx = torch.meshgrid(torch.arange(256), torch.arange(256), indexing="ij")
            lg = torch.rand((1, 3, 256, 256), generator=g) * 0.2
            lg[0, 1] += ((yy - 100) ** 2 + (xx - 90) ** 2 < 60 ** 2).float()            # two blobs and a background: masks worth cleaning
            lg[0, 2] += ((yy - 170) ** 2 + (xx - 180) ** 2 < 40 ** 2).float()
            lg[0, 0] += 0.5
            self.logits = lg.to(device)

        def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output):
            return self.logits, None

    class Sam:
        def __init__(self):
            self.image_encoder, self.prompt_encoder, self.mask_decoder = Enc(), Prompt(), Dec()
            self._p = torch.zeros(1, device=device)

        def parameters(self):
            return iter((self._p,))
    return Sam()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_segmentor_glue.txt"))
    a = ap.parse_args()
    import torch
    import tee_optical_flow_amd as T
    from tee_optical_flow_amd import masks
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    eng = T.DenseFlow(device_id=0)
    dev = torch.device("cuda", 0)
    sam = stand_in(torch, dev)

    def glue_host(fr):
        return np.stack([masks.evaluate_1_slice(f, sam) for f in fr])

    def glue_device(fr):
        return masks._predict_classmaps_device(fr, sam, eng, a.chunk)

    def timed(fn, *args):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn(*args)
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t) * 1e3

    def row(name, th, td, N, equal):
        mh, md = np.median(th), np.median(td)
        say(f"  {name}: host {mh:8.1f} ms ({min(th):.1f}-{max(th):.1f}; {mh / N:.2f} ms per frame)  device {md:7.1f} ms "
            f"({min(td):.1f}-{max(td):.1f}; {md / N:.2f} ms per frame)  speed-up {mh / md:5.1f}x  bit-equal {equal}  (median of {len(th)})")

    say(f"segmentor frame glue, 65-frame studies to 1024x1024 and back, stand-in model on the GPU without arithmetic, chunk {a.chunk}; "
        f"host = evaluate_1_slice per frame (PIL, CPU torch, upload, argmax, .cpu(), PIL), device = tf_segmentor_input + tf_segmentor_classmap")
    for name, (N, H, W) in SIZES.items():
        fr = study(N, H, W)
        glue_host(fr[:2]), glue_device(fr)                                               # warm-up of both
        th, td, equal = [], [], True
        for _ in range(a.reps):
            h, t = timed(glue_host, fr); th.append(t)
            d, t = timed(glue_device, fr); td.append(t)
            equal = equal and h.dtype == d.dtype and np.array_equal(h, d)
        row(f"{name} class maps      ", th, td, N, equal)
        # predict_movie as the driver calls it: the glue, then clean_mask on the engine (the same call behind either glue)
        host_pm = lambda: masks.clean_mask(glue_host(fr), "RVIO_2class", engine=eng)     # noqa: E731  (predict_movie before the device glue)
        dev_pm = lambda: masks.predict_movie(fr, sam, mode="RVIO_2class", engine=eng, chunk=a.chunk)   # noqa: E731
        host_pm(), dev_pm()
        th, td, equal = [], [], True
        for _ in range(a.reps):
            h, t = timed(host_pm); th.append(t)
            d, t = timed(dev_pm); td.append(t)
            equal = equal and list(h) == list(d) and all(np.array_equal(h[k], d[k]) for k in h)
        row(f"{name} predict_movie   ", th, td, N, equal)
        # the device's share: events around the calls of one chunk, against a pinned copy of the same bytes
        n = min(a.chunk, N)
        x = eng.segmentor_input(fr[:n])
        logits = sam.mask_decoder.logits.repeat(n, 1, 1, 1).contiguous()
        pin_in = torch.from_numpy(fr[:n].copy()).pin_memory()
        dst_in = torch.empty_like(pin_in, device=dev)
        dmap = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
        pin_map = torch.empty((n, H, W), dtype=torch.uint8).pin_memory()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        spans = {"input": [], "input_copy": [], "classmap": [], "classmap_copy": []}
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            ev[0].record(); eng.segmentor_input(fr[:n], out=x); ev[1].record()
            ev[2].record(); dst_in.copy_(pin_in, non_blocking=True); ev[3].record()
            ev[4].record(); eng.segmentor_classmap(logits, (H, W)); ev[5].record()
            ev[6].record(); pin_map.copy_(dmap, non_blocking=True); ev[7].record()
            torch.cuda.synchronize()
            for k, i in (("input", 0), ("input_copy", 2), ("classmap", 4), ("classmap_copy", 6)):
                spans[k].append(ev[i].elapsed_time(ev[i + 1]))
        m = {k: float(np.median(v[1:])) for k, v in spans.items()}
        chunks = -(-N // a.chunk)
        say(f"  {name} device time per chunk of {n} frames (events on the stream): segmentor_input {m['input']:.2f} ms of which a plain upload "
            f"of the frames is {m['input_copy']:.2f} ms (kernel ~{m['input'] - m['input_copy']:.2f} ms for {n * 12} MiB written); "
            f"segmentor_classmap {m['classmap']:.2f} ms of which a plain download of the maps is {m['classmap_copy']:.2f} ms; "
            f"kernels ~{max(m['input'] - m['input_copy'], 0) + max(m['classmap'] - m['classmap_copy'], 0):.2f} ms per chunk, "
            f"~{(max(m['input'] - m['input_copy'], 0) + max(m['classmap'] - m['classmap_copy'], 0)) * chunks:.1f} ms per study, "
            f"{(max(m['input'] - m['input_copy'], 0) + max(m['classmap'] - m['classmap_copy'], 0)) * chunks / np.median(td) * 100:.1f} % of the device path's predict_movie")
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
