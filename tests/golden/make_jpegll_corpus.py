"""Writes tests/golden/jpegll_corpus.npz: JPEG Lossless streams (SOF3, predictor 1) made by frames.jpegll_encode_frame, with the SHA-256
of the encoded array and of Pillow's decode of the stream (libjpeg-turbo 3 decodes SOF3) -- so that the tests need no PIL.  A valid
lossless stream has one decoding, so the two digests of a case are equal; both are recorded, as made.  Needs Pillow built on
libjpeg-turbo; run from the repository's root:

    python tests/golden/make_jpegll_corpus.py

W in {1, 2, 63, 64, 65, 127, 129, 200} (a 64-lane scan round and its carry), H in {1, 2, 3, 17, 80}, 1 and 3 samples; noise, constant
frames, ramps, 0/255 checkerboards and sector-masked speckle; restart intervals of none, 1, 2, 3 (H no multiple), H and H + 2 rows."""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tee_optical_flow_amd import frames as F  # noqa: E402
from tests.jpegll_cases import K3, LONG, NINE, image  # noqa: E402

WIDTHS, HEIGHTS = [1, 2, 63, 64, 65, 127, 129, 200], [1, 2, 3, 17, 80]
KINDS, HOWS = ["noise", "const", "ramp", "checker", "speckle"], ["none", "one", "two", "three", "all", "above"]


def restart_rows(how, H):
    if how == "three" and (H % 3 == 0 or H < 3):
        how = "two"
    return {"none": 0, "one": 1, "two": 2, "three": 3, "all": H, "above": H + 2}[how]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    assert features.check_feature("libjpeg_turbo"), "the yardstick is libjpeg-turbo as Pillow drives it"
    rng = np.random.default_rng(3070)
    cases, k = [], 0
    for H in HEIGHTS:
        for W in WIDTHS:
            for samples in (1, 3):
                kind, how = KINDS[k % 5], HOWS[(k // 5 + k) % 6]
                tables = [None, [K3, NINE], [LONG]][k % 3]                 # the encoder's default; two tables; 16-bit codes
                k += 1
                cases.append((f"enc_{H}x{W}x{samples}_{kind}_{how}", H, W, samples, kind, how, tables))
    for samples in (1, 3):                                                 # every interval rule on one shape
        for how in HOWS:
            cases.append((f"enc_ri_17x65x{samples}_{how}", 17, 65, samples, "speckle", how, None))
    names, streams, meta, sha_array, sha_pillow = [], [], [], [], []
    for name, H, W, samples, kind, how, tables in cases:
        a = image(kind, H, W, samples, rng)
        a = a[..., 0] if samples == 1 else a
        s = F.jpegll_encode_frame(a, restart_rows(how, H), tables)
        im = Image.open(io.BytesIO(s))
        assert im.mode == ("L" if samples == 1 else "RGB"), (name, im.mode)
        got = np.asarray(im)
        assert np.array_equal(got, a), name
        names.append(name); streams.append(s); meta.append((H, W, samples)); sha_array.append(sha(a)); sha_pillow.append(sha(got))
    lens = np.array([len(s) for s in streams], np.uint32)
    off = np.zeros(len(streams), np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    path = os.path.join(HERE, "jpegll_corpus.npz")
    np.savez_compressed(path, blob=np.frombuffer(b"".join(streams), np.uint8), off=off, len=lens, shape=np.array(meta, np.int32),
                        names=np.array(names), sha_array=np.array(sha_array), sha_pillow=np.array(sha_pillow))
    print(f"{len(streams)} streams, {int(lens.sum())} bytes of JPEG, {os.path.getsize(path)} bytes on disk")


if __name__ == "__main__":
    main()
