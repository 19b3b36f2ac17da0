"""Writes tests/golden/jpeg_corpus.npz: JPEG Baseline streams made by Pillow's encoder (libjpeg-turbo) and the SHA-256 of Pillow's two
decodes of each -- np.asarray(Image.open(s)) (RGB, or grey) and, after im.draft("YCbCr", None), the stream's own components upsampled
with no colour transform -- so that the tests need no PIL.  Needs Pillow built on libjpeg-turbo; run from the repository's root:

    python tests/golden/make_jpeg_corpus.py

Sizes 1x1 ... 80x200; 4:4:4, 4:2:2, 4:2:0 and grey; quality 5 ... 100; optimised tables; restart intervals of 1 MCU, one MCU row, a
value that does not divide the MCU count, one at least the MCU count, and one that gives more than 8 intervals."""
import hashlib
import io
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (2, 1), (7, 9), (8, 8), (16, 16), (17, 23), (33, 7), (31, 31), (9, 130), (48, 64)]
BIG = (80, 200)
SAMPLINGS = {"444": 0, "422": 1, "420": 2, "grey": None}
MCU = {"444": (8, 8), "422": (8, 16), "420": (16, 16), "grey": (8, 8)}     # rows, columns


def content(kind, H, W, ch, rng):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        a = rng.integers(0, 256, (H, W, ch))
    elif kind == "gradient":
        a = np.stack([(x * 255 // max(W - 1, 1) + c * 60) % 256 if c % 2 == 0 else y * 255 // max(H - 1, 1) for c in range(ch)], -1)
    else:                                                                  # smooth: a few low-frequency waves and a little noise
        a = np.stack([127 + 90 * np.sin(x / (5.0 + c) + c) * np.cos(y / (7.0 - c)) for c in range(ch)], -1) + rng.normal(0, 3, (H, W, ch))
    return np.clip(a, 0, 255).astype(np.uint8)


def restart_blocks(how, H, W, sampling):
    mh, mw = MCU[sampling]
    mcux, mcuy = -(-W // mw), -(-H // mh)
    n = mcux * mcuy
    return {"none": 0, "one": 1, "row": mcux, "odd": next(r for r in range(2, n + 3) if n % r), "all": n + 5,
            "many": max(1, n // 11)}[how]


def encode(a, sampling, quality, ri, optimize):
    im = Image.fromarray(a[..., 0], "L") if sampling == "grey" else Image.fromarray(a, "RGB")
    kw = {} if sampling == "grey" else {"subsampling": SAMPLINGS[sampling]}
    bio = io.BytesIO()
    im.save(bio, "JPEG", quality=quality, optimize=optimize, restart_marker_blocks=ri, **kw)
    return bio.getvalue()


def digests(s, sampling):
    rgb = np.asarray(Image.open(io.BytesIO(s)))
    im = Image.open(io.BytesIO(s))
    if sampling != "grey":
        im.draft("YCbCr", None)
    own = np.asarray(im)
    return hashlib.sha256(np.ascontiguousarray(own).tobytes()).hexdigest(), hashlib.sha256(np.ascontiguousarray(rgb).tobytes()).hexdigest()


def main():
    assert features.check_feature("libjpeg_turbo"), "the yardstick is libjpeg-turbo as Pillow drives it"
    rng = np.random.default_rng(2950)
    kinds, quals, hows = ["noise", "gradient", "smooth"], [5, 50, 90, 100], ["none", "one", "row", "odd", "all", "many"]
    cases, k = [], 0
    for H, W in SIZES:
        for sampling in SAMPLINGS:
            for rep in range(3):                                           # three draws per size and sampling, the knobs rotating
                kind, q, how = kinds[k % 3], quals[(k // 3 + rep) % 4], hows[(k + 2 * rep) % 6]
                k += 1
                cases.append((f"enc_{H}x{W}_{sampling}_{kind}_q{q}_{how}", H, W, sampling, kind, q, how, rep != 1))
    for i, (sampling, how, q) in enumerate([("420", "many", 90), ("422", "row", 50), ("444", "odd", 90), ("grey", "one", 100)]):
        cases.append((f"enc_{BIG[0]}x{BIG[1]}_{sampling}_smooth_q{q}_{how}", BIG[0], BIG[1], sampling, "smooth", q, how, True))
    for sampling in SAMPLINGS:                                             # every interval rule on one shape per sampling
        for how in hows:
            cases.append((f"enc_ri_40x56_{sampling}_{how}", 40, 56, sampling, "smooth", 75, how, True))
    names, streams, meta, sha_own, sha_rgb = [], [], [], [], []
    for name, H, W, sampling, kind, q, how, optimize in cases:
        a = content(kind, H, W, 1 if sampling == "grey" else 3, rng)
        s = encode(a, sampling, q, restart_blocks(how, H, W, sampling), optimize)
        o, r = digests(s, sampling)
        names.append(name); streams.append(s); meta.append((H, W, 1 if sampling == "grey" else 3)); sha_own.append(o); sha_rgb.append(r)
    lens = np.array([len(s) for s in streams], np.uint32)
    off = np.zeros(len(streams), np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    path = os.path.join(HERE, "jpeg_corpus.npz")
    np.savez_compressed(path, blob=np.frombuffer(b"".join(streams), np.uint8), off=off, len=lens, shape=np.array(meta, np.int32),
                        names=np.array(names), sha_own=np.array(sha_own), sha_rgb=np.array(sha_rgb))
    print(f"{len(streams)} streams, {int(lens.sum())} bytes of JPEG, {os.path.getsize(path)} bytes on disk")


if __name__ == "__main__":
    main()
