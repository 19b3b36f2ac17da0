"""The segmentor glue's CPU statement (tee_optical_flow_amd/masks.py: pil_resize_bilinear, pil_nearest_index, segmentor_lut) against
PIL and torch themselves, the C++ tables the device path gathers with (csrc/pil_resample_tables.h) against the Python twins, the
fixture tests/golden/segmentor_glue.npz, the choice between predict_movie's host and device path, and the two entry points' argument
checks, which return before any GPU work.  Every comparison is np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tee_optical_flow_amd import masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "segmentor_glue.npz")

# (H, W) -> (out_h, out_w)
BILINEAR_SIZES = [((37, 53), (64, 64)), ((64, 64), (64, 64)), ((512, 512), (1024, 1024)), ((600, 800), (1024, 1024)),
                  ((1080, 1920), (1024, 1024)), ((1, 7), (16, 16)), ((434, 636), (1024, 1024)), ((1200, 1030), (1024, 1024)),
                  ((1024, 700), (1024, 1024))]
TABLE_BILINEAR = [(1, 16), (7, 16), (37, 64), (96, 64), (512, 1024), (800, 1024), (1920, 1024), (1024, 1024)]
TABLE_NEAREST = [(256, 1), (256, 37), (256, 512), (256, 600), (256, 800)]


def glue_fixture():
    """{'in': {name: (frames, resized)}, 'cm': {name: (logits, class map)}} of tests/golden/segmentor_glue.npz"""
    z = np.load(GOLD)
    out = {"in": {}, "cm": {}}
    for k in z.files:
        kind, rest = k.split("_", 1)
        name, what = rest.rsplit("_", 1)
        out[kind].setdefault(name, {})[what] = z[k]
    return {"in": {n: (d["frames"], d["resized"]) for n, d in out["in"].items()},
            "cm": {n: (d["logits"], d["map"]) for n, d in out["cm"].items()}}


def twin_classmap(logits, size):
    """numpy statement of DenseFlow.segmentor_classmap: np.argmax (first of equal maxima, NaN is the maximum and the first NaN wins, as
    torch's on the CPU) and a gather with the twin indices"""
    logits = np.asarray(logits, np.float32)
    iy, ix = masks.pil_nearest_index(logits.shape[2], size[0]), masks.pil_nearest_index(logits.shape[3], size[1])
    return np.argmax(logits, axis=1).astype(np.uint8)[:, iy][:, :, ix]


class FakeSam:
    """SAM-shaped stand-in (tests/test_study_driver_cpu.py's, with a device to sit on): comparisons and constants only, so torch on
    the GPU and on the CPU agree bit for bit"""

    def __init__(self, device="cpu"):
        import torch
        self.device = torch.device(device)

        class Enc(torch.nn.Module):
            def forward(self, x):
                return x

        class Prompt(torch.nn.Module):
            def forward(self, points=None, boxes=None, masks=None):
                return None, None

            def get_dense_pe(self):
                return None

        class Dec(torch.nn.Module):
            def forward(self, image_embeddings, image_pe, sparse_prompt_embeddings, dense_prompt_embeddings, multimask_output):
                x = image_embeddings[:, 0]                              # [1,1024,1024]
                c1 = (x > 0.2).float()
                c2 = torch.zeros_like(x)
                c2[:, 300:700, 300:700] = 2.0
                logits = torch.stack([torch.full_like(x, 0.5), c1, c2], dim=1)
                return logits, None

        self.image_encoder, self.prompt_encoder, self.mask_decoder = Enc(), Prompt(), Dec()
        self._p = torch.zeros(1, device=self.device)

    def parameters(self):
        return iter((self._p,)) if self.device.type != "cpu" else iter(())


@pytest.mark.parametrize("src,dst", BILINEAR_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_bilinear_twin_equals_pil(src, dst):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(src[0] * 7 + src[1])
    img = rng.integers(0, 256, src + (3,), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), Image.BILINEAR))
    got = masks.pil_resize_bilinear(img, dst)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    g1 = masks.pil_resize_bilinear(img[..., 1], dst)                    # one channel: mode "L" runs the same passes
    assert np.array_equal(g1, np.asarray(Image.fromarray(img[..., 1]).resize((dst[1], dst[0]), Image.BILINEAR)))


@pytest.mark.parametrize("n_in", [7, 64, 256])
def test_nearest_twin_equals_pil(n_in):
    Image = pytest.importorskip("PIL.Image")
    ramp = np.arange(n_in, dtype=np.uint8)                              # (n_in <= 256: a pixel's value is its index)
    col = Image.fromarray(np.ascontiguousarray(ramp[:, None]), "L")
    row = Image.fromarray(np.ascontiguousarray(ramp[None, :]), "L")
    for n_out in range(1, 601):
        idx = masks.pil_nearest_index(n_in, n_out)
        assert idx.dtype == np.int32 and idx.shape == (n_out,) and idx.min() >= 0 and idx.max() <= n_in - 1
        if n_out == n_in:                                               # (resize returns a copy)
            assert np.array_equal(idx, np.arange(n_in))
        assert np.array_equal(np.asarray(row.resize((n_out, 1), Image.NEAREST))[0], idx.astype(np.uint8)), n_out
        assert np.array_equal(np.asarray(col.resize((1, n_out), Image.NEAREST))[:, 0], idx.astype(np.uint8)), n_out


def test_lut_is_the_tensor_evaluate_1_slice_hands_the_model():
    torch = pytest.importorskip("torch")
    pytest.importorskip("PIL.Image")
    seen = []

    class Spy(FakeSam):
        def __init__(self):
            super().__init__()
            enc = self.image_encoder

            class Enc(torch.nn.Module):
                def forward(self, x):
                    seen.append(x.clone())
                    return enc(x)
            self.image_encoder = Enc()
    lut = masks.segmentor_lut()
    assert lut.dtype == np.float32 and lut.shape == (3, 256) and lut.flags.c_contiguous
    # a 1024 x 1024 frame is not resized: byte b of channel c sits at row (b + 7 c) % 256
    frame = np.empty((1024, 1024, 3), np.uint8)
    for c in range(3):
        frame[..., c] = ((np.arange(1024) + 7 * c) % 256).astype(np.uint8)[:, None]
    masks.evaluate_1_slice(frame, Spy())
    x = seen[0].numpy()
    assert x.shape == (1, 3, 1024, 1024) and x.dtype == np.float32
    for c in range(3):
        assert np.array_equal(x[0, c], lut[c][frame[..., c]])
        rows = {int(frame[r, 0, c]): r for r in range(256)}
        assert all(x[0, c, rows[b], 5] == lut[c, b] for b in range(256))
    # and through a resize: the tensor is the LUT of the twin's bytes
    rng = np.random.default_rng(4)
    small = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    masks.evaluate_1_slice(small, Spy())
    r = masks.pil_resize_bilinear(small, (1024, 1024))
    assert np.array_equal(seen[1].numpy()[0], np.stack([lut[c][r[..., c]] for c in range(3)]))


def test_cpp_tables_equal_the_python_twins(tmp_path):
    """the stand-alone table program, built with the address and undefined-behaviour sanitizers (their runtimes linked into the
    program itself): every bound, coefficient and index"""
    exe = tmp_path / "vrt"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_resample_tables.cpp"), "-o", str(exe)])
    args = [s for p in TABLE_BILINEAR for s in ("b", str(p[0]), str(p[1]))] + [s for p in TABLE_NEAREST for s in ("n", str(p[0]), str(p[1]))]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.splitlines()
    at = 0
    for n_in, n_out in TABLE_BILINEAR:
        ksize, bounds, coeff = masks.pil_bilinear_coeffs(n_in, n_out)
        assert lines[at] == f"bilinear {n_in} {n_out} {ksize}"
        got = np.array([ln.split() for ln in lines[at + 1:at + 1 + n_out]], dtype=np.int64)
        assert got.shape == (n_out, 2 + ksize)
        assert np.array_equal(got[:, :2], bounds) and np.array_equal(got[:, 2:], coeff), (n_in, n_out)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all() and (bounds[:, 1] <= ksize).all()
        at += 1 + n_out
    for n_in, n_out in TABLE_NEAREST:
        assert lines[at] == f"nearest {n_in} {n_out}"
        assert np.array_equal(np.array(lines[at + 1].split(), dtype=np.int64), masks.pil_nearest_index(n_in, n_out)), (n_in, n_out)
        at += 2
    assert at == len(lines)
    assert subprocess.run([str(exe), "b", "0", "4"]).returncode == 2


def test_an_axis_that_keeps_its_length_has_the_single_coefficient_one():
    ksize, bounds, coeff = masks.pil_bilinear_coeffs(64, 64)
    assert ksize == 3 and np.array_equal(bounds[:, 0], np.arange(64)) and (coeff[:, 0] == 1 << 22).all() and not coeff[:, 1:].any()


def test_twins_equal_the_fixture():
    fx = glue_fixture()
    assert set(fx["in"]) == {"upscale", "downscale", "hidentity", "tiny", "scalar"}
    for name, (frames, resized) in fx["in"].items():
        assert frames.dtype == resized.dtype == np.uint8 and frames.shape[0] == resized.shape[0] == 4
        assert max(resized.shape[1:3]) <= 64
        assert (frames[1] == 255).all() and not frames[2].any() and set(np.unique(frames[3])) <= {0, 255}
        for f, r in zip(frames, resized):
            assert np.array_equal(masks.pil_resize_bilinear(f, r.shape[:2]), r), name
    assert {lg.shape[1] for lg, _ in fx["cm"].values()} == {1, 3, 9, 256}
    for name, (logits, cmap) in fx["cm"].items():
        assert logits.dtype == np.float32 and cmap.dtype == np.uint8
        assert np.array_equal(twin_classmap(logits, cmap.shape[1:]), cmap), name
    assert not fx["cm"]["all_equal"][1].any()
    assert np.isnan(fx["cm"]["odd"][0]).any() and np.isinf(fx["cm"]["odd"][0]).any()
    assert os.path.getsize(GOLD) < 256 << 10


def test_fixture_is_what_pil_and_torch_compute():
    Image = pytest.importorskip("PIL.Image")
    torch = pytest.importorskip("torch")
    fx = glue_fixture()
    for name, (frames, resized) in fx["in"].items():
        oh, ow = resized.shape[1:3]
        for f, r in zip(frames, resized):
            assert np.array_equal(np.asarray(Image.fromarray(f).convert("RGB").resize((ow, oh), Image.BILINEAR)), r), name
    for name, (logits, cmap) in fx["cm"].items():
        pred = torch.from_numpy(logits).argmax(dim=1).float().numpy().astype(np.uint8)
        H, W = cmap.shape[1:]
        for p, m in zip(pred, cmap):
            assert np.array_equal(np.asarray(Image.fromarray(p, "L").resize((W, H), resample=Image.NEAREST)), m), name


def test_predict_movie_takes_the_host_path_unless_engine_frames_and_model_fit():
    pytest.importorskip("torch")
    pytest.importorskip("PIL.Image")
    from tee_optical_flow_amd.synth import speckle_sequence
    calls = []

    class Spy:
        device_id = 0

        def segmentor_input(self, *a, **k):
            calls.append("input")
            raise AssertionError("the device path was taken")

        def segmentor_classmap(self, *a, **k):
            calls.append("classmap")
            raise AssertionError("the device path was taken")

    class NoGlue:
        device_id = 0
    nparr = np.repeat(speckle_sequence(3, 3, 32, 40)[..., None], 3, axis=3)
    sam = FakeSam()
    want = masks.predict_movie(nparr, sam, mode="RVIO_2class")
    for eng in (Spy(), NoGlue()):                                       # a CPU model: the host path, whatever the engine can do
        got = masks.predict_movie(nparr, sam, mode="RVIO_2class", engine=eng)
        assert list(got) == list(want) and all(np.array_equal(got[k], want[k]) for k in want)
    assert calls == []


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from tee_optical_flow_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(64)            # never dereferenced: every check comes before the handle is used
    h = C.addressof(fake)
    rgb = np.zeros((2, 4, 4, 3), np.uint8)
    lut = masks.segmentor_lut()
    dummy = C.create_string_buffer(64)           # stands for device memory: never touched either
    good = dict(h=h, rgb=rgb.ctypes.data, N=2, H=4, W=4, oh=8, ow=8, lut=lut.ctypes.data, out=C.addressof(dummy))

    def inp(**kw):
        a = {**good, **kw}
        return L.tf_segmentor_input(a["h"], a["rgb"], a["N"], a["H"], a["W"], a["oh"], a["ow"], a["lut"], a["out"], None)
    for bad in (dict(h=None), dict(rgb=None), dict(lut=None), dict(out=None), dict(N=0), dict(H=0), dict(W=-1), dict(oh=0), dict(ow=0)):
        assert inp(**bad) == _lib.TF_ERR_INVALID_ARG, bad
    assert inp(H=65536, W=65536) == _lib.TF_ERR_UNSUPPORTED and inp(oh=46341, ow=46341) == _lib.TF_ERR_UNSUPPORTED
    cmap = np.full((2, 4, 4), 7, np.uint8)
    goodc = dict(h=h, lg=C.addressof(dummy), N=2, C=3, hh=4, ww=4, H=4, W=4, out=cmap.ctypes.data)

    def cls(**kw):
        a = {**goodc, **kw}
        return L.tf_segmentor_classmap(a["h"], a["lg"], a["N"], a["C"], a["hh"], a["ww"], a["H"], a["W"], a["out"], None)
    for bad in (dict(h=None), dict(lg=None), dict(out=None), dict(N=0), dict(C=0), dict(hh=0), dict(ww=0), dict(H=0), dict(W=-3)):
        assert cls(**bad) == _lib.TF_ERR_INVALID_ARG, bad
    assert cls(C=257) == _lib.TF_ERR_UNSUPPORTED and cls(C=256, hh=65536, ww=65536) == _lib.TF_ERR_UNSUPPORTED
    assert cls(H=46341, W=46341) == _lib.TF_ERR_UNSUPPORTED
    assert (cmap == 7).all()
