"""JPEG Baseline without a GPU: the independent reference decoder of tests/jpeg_cases.py against the recorded digests of Pillow's decodes
(and against Pillow itself where it imports), the numpy twin (frames.jpeg_decode_frame) against the reference decoder on the whole corpus,
statuses included, the core under the sanitizers (tests/csrc/verify_jpeg.cpp: a stand-alone program with exact-size buffers), the colour
function, and the library's argument refusals."""
import io
import os
import subprocess

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F

from tests import jpeg_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_decoder_gives_the_recorded_pillow_digests():
    cases, shas = JC.golden()
    want = JC.expected()
    assert len(cases) >= 140
    for c in cases:
        arr, status = want[c.name]
        assert status == 0 and JC.sha(arr) == shas[c.name][0], c.name
        if c.samples == 3 and c.H * c.W <= 48 * 64:                        # (the per-pixel colour loop: the small ones)
            assert JC.sha(JC.reference_rgb(arr)) == shas[c.name][1], c.name
        elif c.samples == 3:
            assert JC.sha(F.ycc_to_rgb_libjpeg(arr)) == shas[c.name][1], c.name
        else:
            assert shas[c.name][0] == shas[c.name][1]


def test_the_golden_corpus_covers_what_it_promises():
    cases, _ = JC.golden()
    names = [c.name for c in cases]
    for sampling in ("444", "422", "420", "grey"):
        for how in ("none", "one", "row", "odd", "all", "many"):
            assert f"enc_ri_40x56_{sampling}_{how}" in names
    assert {(c.H, c.W) for c in cases} >= {(1, 1), (2, 1), (7, 9), (8, 8), (16, 16), (17, 23), (33, 7), (31, 31), (9, 130), (80, 200)}
    assert os.path.getsize(JC.GOLDEN) < 400 * 1024
    many = next(c for c in cases if c.name == "enc_ri_40x56_444_many")
    assert many.buf.count(b"\xff\xd7") >= 1                                # more than 8 intervals: the numbering has wrapped


def test_reference_decoder_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    for c in JC.golden()[0]:
        im = Image.open(io.BytesIO(c.buf))
        if c.samples == 3:
            im.draft("YCbCr", None)
        assert np.array_equal(np.asarray(im), JC.expected()[c.name][0]), c.name


def test_twin_agrees_with_the_reference_decoder_on_the_whole_corpus():
    want, seen = JC.expected(), {0: 0, 1: 0, 2: 0, 3: 0}
    for c in JC.corpus():
        arr, status = want[c.name]
        got, got_status = F.jpeg_decode_frame(c.buf, c.H, c.W, c.samples)
        assert got_status == status, (c.name, got_status, status)
        assert got.shape == ((c.H, c.W) if c.samples == 1 else (c.H, c.W, c.samples)) and got.dtype == np.uint8
        assert np.array_equal(got, arr) if status == 0 else not got.any(), c.name
        seen[status] += 1
    assert all(seen.values()), seen
    assert len({c.name for c in JC.corpus()}) == len(JC.corpus())           # no two cases share a name


def test_the_corpus_says_what_its_names_promise():
    want = JC.expected()
    for name, (_, status) in want.items():
        if name.startswith(("enc_", "hand_")):
            assert status == 0, name
        elif name.startswith("bad_"):
            assert status == 1, name
        elif name.startswith("refused_"):
            assert status == 2, name
        elif name.startswith("data_"):
            assert status == 3, name
    cuts = [want[n][1] for n in want if n.startswith("cut_after_")]
    assert cuts[0] == 1 and 3 in cuts and cuts[-1] == 0 and cuts == sorted(cuts, key=lambda s: (s == 0, s))   # header, data, only EOI missing
    first = want["hand_sixteen_bit_codes"][0]
    for pad in (1, 15, 16, JC.T - 1, JC.T + 16):                            # the stage walk's pixels do not depend on the COM segment
        got, status = JC.reference_decode(JC.stage_stream(pad), 16, 16, 1)
        assert status == 0 and np.array_equal(got, first), pad
    assert F.jpeg_decode_frame(JC.stage_stream(JC.T + 3), 16, 16, 1)[1] == 0
    with pytest.raises(ValueError):
        F.jpeg_decode_frame(b"", 0, 3, 1)
    with pytest.raises(ValueError):
        F.jpeg_decode_frame(b"", 3, 3, 2)


def test_wrapping_arithmetic_is_the_same_in_every_decoder():
    """DC at +-2047 steps of 255 passes 2^31 in the IDCT: the project fixes signed 32-bit there"""
    c = next(c for c in JC.corpus() if c.name == "hand_dc_plus_2047_q255")
    arr, status = JC.expected()[c.name]
    assert status == 0 and arr.min() < arr.max()
    assert np.array_equal(F.jpeg_decode_frame(c.buf, c.H, c.W, 1)[0], arr)


def test_ycc_to_rgb_libjpeg():
    ycc = np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128], [76, 85, 255], [255, 0, 0], [0, 255, 255], [29, 255, 107]], np.uint8)
    assert np.array_equal(F.ycc_to_rgb_libjpeg(ycc), JC.reference_rgb(ycc))
    assert F.ycc_to_rgb_libjpeg(ycc)[2].tolist() == [128, 128, 128]
    rnd = np.random.default_rng(5).integers(0, 256, (4000, 3), dtype=np.uint8)
    assert np.array_equal(F.ycc_to_rgb_libjpeg(rnd), JC.reference_rgb(rnd))
    with pytest.raises(ValueError):
        F.ycc_to_rgb_libjpeg(np.zeros((2, 2), np.uint8))


# ---- the core under the sanitizers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verify_jpeg(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jpeg") / "verify_jpeg"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_jpeg.cpp"), "-o", str(exe)])
    return str(exe)


def test_core_decodes_the_whole_corpus_under_the_sanitizers(verify_jpeg, tmp_path):
    path = tmp_path / "corpus.bin"
    stage = [JC.Case(f"stage_{pad}", JC.stage_stream(pad), 16, 16, 1) for pad in (0, 1, 15, 16, 17, JC.T - 2, JC.T, JC.T + 16)]
    want = {**JC.expected(), **{c.name: JC.reference_decode(c.buf, c.H, c.W, c.samples) for c in stage}}
    cases = JC.corpus() + tuple(stage)
    JC.write_corpus(path, cases, want)
    r = subprocess.run([verify_jpeg, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.strip() == f"{len(cases)} cases ok"


def test_core_colour_function_under_the_sanitizers(verify_jpeg, tmp_path):
    g = np.arange(0, 256, 5, dtype=np.uint8)
    ycc = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    ycc = np.concatenate([ycc, np.random.default_rng(9).integers(0, 256, (50000, 3), dtype=np.uint8)])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    ycc.tofile(fin)
    r = subprocess.run([verify_jpeg, "color", str(fin), str(fout), str(len(ycc))], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert np.array_equal(np.fromfile(fout, np.uint8).reshape(-1, 3), F.ycc_to_rgb_libjpeg(ycc))


# ---- the library's entry points (no GPU needed: a null handle is refused before anything else) ------------------------------------------
def test_library_exports_and_refuses_without_a_handle():
    from tee_optical_flow_amd.dense_flow import DenseFlow
    assert {"tf_jpeg_decode", "tf_hold_frames_jpeg", "tf_jpeg_stage_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.tf_jpeg_stage_bytes() == _lib.JPEG_STAGE_BYTES == JC.T and JC.T % 16 == 0
    blob, off, ln = F.jpeg_record([JC.stage_stream(0)])
    out, status = np.full(256, 7, np.uint8), np.full(1, -7, np.int32)
    assert L.tf_jpeg_decode(None, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, 16, 16, 1, out.ctypes.data, status.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_hold_frames_jpeg(None, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, 16, 16, 1, 1, 0, 0, status.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert (out == 7).all() and status[0] == -7 and L.tf_abi_version() == 2
    for name in ("jpeg_decode", "hold_frames_jpeg"):
        assert callable(getattr(DenseFlow, name))
    assert F.JPEG_BASELINE_TRANSFER_SYNTAX == "1.2.840.10008.1.2.4.50" and len(F.JPEG_STATUS_TEXT) == 4
    assert _lib.JPEG_COLORS == {"none": 0, "libjpeg": 1}


# ---- dicom_jpeg_frames ---------------------------------------------------------------------------------------------------------------------
def _item(data):
    return b"\xfe\xff\x00\xe0" + len(data).to_bytes(4, "little") + data


END = b"\xfe\xff\xdd\xe0\x00\x00\x00\x00"


def _dataset(streams, H, W, samples, uid=F.JPEG_BASELINE_TRANSFER_SYNTAX, bits=8, photometric="YBR_FULL_422", **more):
    from types import SimpleNamespace
    even = [s + b"\x00" * (len(s) & 1) for s in streams]                    # (a fragment has even length: PS3.5 A.4; the pad follows EOI)
    return SimpleNamespace(file_meta=SimpleNamespace(TransferSyntaxUID=uid), PixelData=_item(b"") + b"".join(_item(e) for e in even) + END,
                           Rows=H, Columns=W, SamplesPerPixel=samples, BitsAllocated=bits, PhotometricInterpretation=photometric, **more)


def test_dicom_jpeg_frames_on_stub_datasets():
    from tee_optical_flow_amd import pipeline as P
    from tee_optical_flow_amd.exceptions import ConfigurationError, DICOMReadError
    cases = [c for c in JC.golden()[0] if (c.H, c.W, c.samples) == (48, 64, 3)][:3]
    want = np.stack([JC.expected()[c.name][0] for c in cases])
    got = P.dicom_jpeg_frames(_dataset([c.buf for c in cases], 48, 64, 3, NumberOfFrames="3"))       # (NumberOfFrames is an IS: a string)
    assert isinstance(got, P.JpegFrames) and isinstance(got, P.RleFrames) and got.shape == (3, 48, 64) and got.samples == 3
    assert got.photometric == "YBR_FULL_422" and got.color == "libjpeg" and got.blob.dtype == np.uint8 and got.off.dtype == np.uint64
    assert np.array_equal(got.decode(), want)                              # PIL where it imports, else the twin: the same components
    assert P._jpeg_form(got, None) == ("YBR_FULL", "libjpeg", None) and P._jpeg_form(got, "RGB") == ("RGB", "none", None)
    host, ph = P._jpeg_host(got, None)
    assert ph is None and np.array_equal(host, F.ycc_to_rgb_libjpeg(want))
    dicom = P.dicom_jpeg_frames(_dataset([c.buf for c in cases], 48, 64, 3, NumberOfFrames=3, photometric="YBR_FULL"), jpeg_color="dicom")
    assert P._jpeg_form(dicom, None) == ("YBR_FULL", "none", None)
    host, ph = P._jpeg_host(dicom, None)
    assert ph == "YBR_FULL" and np.array_equal(host, want)
    grey = next(c for c in JC.golden()[0] if (c.H, c.W, c.samples) == (48, 64, 1))
    one = P.dicom_jpeg_frames(_dataset([grey.buf], 48, 64, 1, photometric="MONOCHROME2"))             # no NumberOfFrames: one frame
    assert one.shape == (1, 48, 64) and np.array_equal(one.decode()[0], JC.expected()[grey.name][0])
    assert P._jpeg_form(one, None)[0] is None                              # (a grey stack of one frame stays grey)
    two = P.dicom_jpeg_frames(_dataset([grey.buf, grey.buf], 48, 64, 1, photometric="MONOCHROME2", NumberOfFrames=2))
    assert P._jpeg_form(two, None) == ("GRAY", "none", None)
    assert P._jpeg_form(got, "PALETTE COLOR")[2] is not None and P._jpeg_form(two, "RGB")[2] is not None
    # refused: 16-bit samples, another transfer syntax, no file_meta -- read through pixel_array as ever
    assert P.dicom_jpeg_frames(_dataset([c.buf for c in cases], 48, 64, 3, bits=16, NumberOfFrames=3)) is None
    assert "BitsAllocated = 16" in P._jpeg_refusal(_dataset([], 1, 1, 3, bits=16))
    assert "SamplesPerPixel = 4" in P._jpeg_refusal(_dataset([], 1, 1, 4))
    assert P.dicom_jpeg_frames(_dataset([c.buf for c in cases], 48, 64, 3, uid=F.RLE_TRANSFER_SYNTAX, NumberOfFrames=3)) is None
    assert P.dicom_rle_frames(_dataset([c.buf for c in cases], 48, 64, 3, NumberOfFrames=3)) is None
    assert P.dicom_jpeg_frames(SimpleNamespaceless()) is None
    with pytest.raises(ValueError):                                        # three fragments for two frames and no offset table
        P.dicom_jpeg_frames(_dataset([c.buf for c in cases], 48, 64, 3, NumberOfFrames=2))
    with pytest.raises(ConfigurationError):
        P.dicom_jpeg_frames(_dataset([], 1, 1, 3), jpeg_color="adobe")
    bad = P.JpegFrames(got.blob[:-40].copy(), got.off, np.array([got.len[0], got.len[1], got.len[2] - 40], np.uint32), (3, 48, 64), 3)
    with pytest.raises(DICOMReadError, match="frame 2 did not decode: status 3"):
        bad.decode()


class SimpleNamespaceless:
    Rows, Columns = 1, 1


def test_a_refused_dataset_is_logged_once(caplog):
    from tee_optical_flow_amd import pipeline as P
    P._jpeg_fallbacks.clear()
    ds = _dataset([], 1, 1, 3, bits=16)
    with caplog.at_level("WARNING", logger=P.logger.name):
        assert P._stored_jpeg(ds, "x.dcm") is None and P._stored_jpeg(ds, "y.dcm") is None
        assert P._stored_jpeg(_dataset([], 1, 1, 3, uid="1.2.840.10008.1.2.1"), "z.dcm") is None
    assert [r.getMessage() for r in caplog.records].count(
        "JPEG Baseline pixel data not decoded on the device, the host decodes it instead: JPEG Baseline pixel data with BitsAllocated = 16: "
        "only 8-bit samples are decoded from the stored bytes") == 1 and len(caplog.records) == 1
    P._jpeg_fallbacks.clear()


def test_npz_study_may_carry_jpeg_in_nparrs_place(tmp_path):
    from tee_optical_flow_amd import pipeline as P
    from tee_optical_flow_amd.exceptions import DICOMReadError
    cases = [c for c in JC.golden()[0] if (c.H, c.W, c.samples) == (48, 64, 3)][:4]
    want = np.stack([JC.expected()[c.name][0] for c in cases])
    blob, off, ln = F.jpeg_record([c.buf for c in cases])
    path = str(tmp_path / "s.npz")
    np.savez(path, jpeg_blob=blob, jpeg_off=off, jpeg_len=ln, rows=48, cols=64, samples=3, photometric="YBR_FULL_422", pixel_spacing=0.05, frame_rate=40.0)
    stored = P.read_study_stored(path)
    assert isinstance(stored[0], P.JpegFrames) and stored[1] == "YBR_FULL_422" and stored[0].shape == (4, 48, 64) and stored[0].color == "libjpeg"
    arr, md, pid, hr = P.read_study(path)                                  # frames="host": the host decodes, libjpeg's colours
    assert np.array_equal(arr, F.ycc_to_rgb_libjpeg(want)) and md["pixel_spacing"] == 0.05
    np.savez(path, jpeg_blob=blob, jpeg_off=off, jpeg_len=ln, rows=48, cols=64, samples=3, photometric="YBR_FULL", jpeg_color="dicom")
    assert np.array_equal(P.read_study(path)[0], F.ybr_full_to_rgb(want))
    np.savez(path, jpeg_blob=blob, jpeg_off=off, jpeg_len=ln, rows=48, cols=64)
    with pytest.raises(DICOMReadError, match="samples"):
        P.read_study_stored(path)
    np.savez(path, jpeg_blob=blob[:100], jpeg_off=off, jpeg_len=ln, rows=48, cols=64, samples=3)
    with pytest.raises(DICOMReadError, match="inside jpeg_blob"):
        P.read_study(path)
