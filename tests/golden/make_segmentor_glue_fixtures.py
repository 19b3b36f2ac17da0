"""Writes tests/golden/segmentor_glue.npz: what PIL and torch on the CPU make of small frames and logits on the two sides of the
segmentor call in evaluate_1_slice (tee_optical_flow_amd/masks.py) -- the expected values of the device glue (DenseFlow.segmentor_input,
DenseFlow.segmentor_classmap) and of its numpy twins.  PIL and torch on the CPU only; run from the repository root:
    python tests/golden/make_segmentor_glue_fixtures.py
Per input case  in_<name>_frames uint8 [4,H,W,3] (random bytes, all 255, all 0, a 1-pixel checkerboard) and in_<name>_resized uint8
[4,oh,ow,3] = Image.resize((ow, oh), BILINEAR).  The float tensor is not stored: it is segmentor_lut()[c][resized].
Per class-map case  cm_<name>_logits float32 [n,C,h,w] and cm_<name>_map uint8 [n,H,W] = argmax(dim=1) -> uint8 -> Image.resize((W, H),
NEAREST), the reference's own steps."""
import os

import numpy as np
import torch
from PIL import Image

INPUT_CASES = [("upscale", 37, 53, 64, 64), ("downscale", 96, 80, 64, 64), ("hidentity", 50, 64, 64, 64), ("tiny", 1, 7, 16, 16),
               ("scalar", 33, 31, 30, 30)]
# name, n, C, h, w, H, W, kind
CLASSMAP_CASES = [("one_class", 2, 1, 16, 16, 9, 21, "random"), ("to_one_pixel", 2, 3, 4, 4, 1, 1, "random"),
                  ("wide", 2, 9, 64, 64, 25, 100, "ties"), ("odd", 3, 3, 64, 64, 37, 53, "special"),
                  ("all_equal", 1, 3, 16, 16, 40, 24, "equal"), ("many", 1, 256, 8, 8, 13, 5, "ties")]


def frames_for(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), np.full((H, W, 3), 255, np.uint8), np.zeros((H, W, 3), np.uint8), board])


def logits_for(rng, kind, n, C, h, w):
    if kind == "equal":
        return np.full((n, C, h, w), 0.25, np.float32)
    if kind == "random":
        return rng.standard_normal((n, C, h, w)).astype(np.float32)
    a = (rng.integers(-3, 4, (n, C, h, w)) / 4.0).astype(np.float32)          # few values: exact ties at most pixels
    if kind == "special":
        a[0, 1, ::5, ::3] = np.inf
        a[0, 0, ::7, ::2] = -np.inf
        a[0, 2, 1::5, 1::3] = np.inf
        a[0, 1, 1::5, 1::3] = np.inf                                           # a tie of infinities
        a[1, 2, ::4, ::4] = np.nan
        a[1, 0, ::8, ::4] = np.nan                                             # two NaNs at one pixel: the first wins
        a[2, 1, 3::6, :] = np.nan
        a[2, :, 5, 5] = -np.inf                                                # every class -inf
    return a


def main():
    rng = np.random.default_rng(20261018)
    out = {}
    for name, H, W, oh, ow in INPUT_CASES:
        fr = frames_for(rng, H, W)
        out[f"in_{name}_frames"] = fr
        out[f"in_{name}_resized"] = np.stack([np.asarray(Image.fromarray(f).convert("RGB").resize((ow, oh), Image.BILINEAR)) for f in fr])
    for name, n, C, h, w, H, W, kind in CLASSMAP_CASES:
        lg = logits_for(rng, kind, n, C, h, w)
        pred = torch.from_numpy(lg).argmax(dim=1).cpu().float()
        out[f"cm_{name}_logits"] = lg
        out[f"cm_{name}_map"] = np.stack([np.asarray(Image.fromarray(pred[i].numpy().astype(np.uint8), "L").resize((W, H), resample=Image.NEAREST))
                                          for i in range(n)])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "segmentor_glue.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
