"""JPEG Lossless (SOF3, predictor 1) without a GPU: the independent reference decoder of tests/jpegll_cases.py against the encoded arrays
and the recorded digests (and against Pillow itself where it imports and takes the stream), the numpy twin (frames.jpegll_decode_frame)
against the reference decoder on the whole corpus, statuses included, the core under the sanitizers (tests/csrc/verify_jpegll.cpp: a
stand-alone program with exact-size buffers), the encoder's round trip, dicom_jpegll_frames on stub datasets, .npz studies, and the
library's argument refusals."""
import io
import os
import subprocess

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F

from tests import jpegll_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_decoder_gives_the_encoded_arrays_and_the_recorded_digests():
    cases, shas = LC.golden()
    want = LC.expected()
    assert len(cases) >= 90
    for c in cases:
        arr, status = want[c.name]
        assert status == 0 and LC.sha(arr) == shas[c.name][0] == shas[c.name][1], c.name
    rng = np.random.default_rng(1)                                          # ... and arrays it has never seen, through the hand-written builder
    for H, W, C, rows in ((1, 1, 1, 0), (3, 65, 3, 1), (9, 5, 1, 4)):
        a = LC.image("noise", H, W, C, rng)
        a = a[..., 0] if C == 1 else a
        got, status = LC.reference_decode(LC.build(H, W, C, LC.diffs_of(a, rows), rows=rows), H, W, C)
        assert status == 0 and np.array_equal(got, a)


def test_the_golden_corpus_covers_what_it_promises():
    cases, _ = LC.golden()
    names = {c.name for c in cases}
    assert {(c.H, c.W, c.samples) for c in cases} >= {(H, W, s) for H in (1, 2, 3, 17, 80) for W in (1, 2, 63, 64, 65, 127, 129, 200) for s in (1, 3)}
    for samples in (1, 3):
        for how in ("none", "one", "two", "three", "all", "above"):
            assert f"enc_ri_17x65x{samples}_{how}" in names
    for kind in ("noise", "const", "ramp", "checker", "speckle"):
        assert any(f"_{kind}_" in n for n in names), kind
    assert os.path.getsize(LC.GOLDEN) < 400 * 1024
    many = next(c for c in cases if c.name == "enc_ri_17x65x3_one")
    assert many.buf.count(b"\xff\xd7") >= 2 and b"\xff\xdd\x00\x04\x00\x41" in many.buf      # 17 intervals of 65 samples: the numbering has wrapped
    seen = set()
    for c in cases:
        seen |= LC.categories(c)
    assert seen == set(range(9)), seen                                     # every category 8-bit samples can give
    checker = next(c for c in cases if "_checker_" in c.name and c.W > 2)
    assert LC.categories(checker) >= {8}                                   # differences of +-255
    const = next(c for c in cases if "_const_" in c.name and c.samples == 1)
    assert LC.categories(const) == {0}


def test_reference_decoder_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    tried = 0
    for c in LC.golden()[0]:
        try:
            im = Image.open(io.BytesIO(c.buf))
            got = np.asarray(im)
        except Exception:                                                  # a Pillow whose libjpeg does not decode SOF3
            continue
        tried += 1
        assert im.mode == ("L" if c.samples == 1 else "RGB") and np.array_equal(got, LC.expected()[c.name][0]), c.name
    if not tried:
        pytest.skip("this Pillow takes no SOF3 stream")


def test_twin_agrees_with_the_reference_decoder_on_the_whole_corpus():
    want, seen = LC.expected(), {0: 0, 1: 0, 2: 0, 3: 0}
    for c in LC.corpus():
        arr, status = want[c.name]
        got, got_status = F.jpegll_decode_frame(c.buf, c.H, c.W, c.samples)
        assert got_status == status, (c.name, got_status, status)
        assert got.shape == ((c.H, c.W) if c.samples == 1 else (c.H, c.W, c.samples)) and got.dtype == np.uint8
        assert np.array_equal(got, arr) if status == 0 else not got.any(), c.name
        seen[status] += 1
    assert all(seen.values()), seen
    assert len({c.name for c in LC.corpus()}) == len(LC.corpus())           # no two cases share a name


def test_the_corpus_says_what_its_names_promise():
    want = LC.expected()
    for name, (_, status) in want.items():
        if name.startswith(("enc_", "hand_")):
            assert status == 0, name
        elif name.startswith("bad_"):
            assert status == 1, name
        elif name.startswith("refused_"):
            assert status == 2, name
        elif name.startswith("data_"):
            assert status == 3, name
    for line in ("bad_sof3_twice", "bad_size", "bad_components", "bad_dht_class_1", "bad_dri_not_a_multiple_of_w", "bad_undefined_table", "refused_sof_c0",
                 "refused_dac", "refused_dnl", "refused_precision_12", "refused_sampling_2x1", "refused_predictor_0", "refused_predictor_7",
                 "refused_point_transform", "refused_se", "refused_ah", "refused_scan_of_two", "data_no_code", "data_category_17", "data_category_16",
                 "data_interval_ends_early", "data_missing_rst", "data_extra_rst", "data_wrong_rst_number", "data_sample_256", "data_sample_minus_1"):
        assert line in want, line                                          # one or more per line of the status table
    cuts = [want[n][1] for n in want if n.startswith("cut_after_")]
    assert cuts[0] == 1 and 3 in cuts and cuts[-1] == 0 and cuts == sorted(cuts, key=lambda s: (s == 0, s))   # header, data, only EOI missing
    first = want["hand_sixteen_bit_codes"][0]
    assert np.array_equal(first, LC._stage_image())
    for pad in (1, 15, 16, LC.T - 1, LC.T + 16):                            # the stage walk's pixels do not depend on the COM segment
        got, status = LC.reference_decode(LC.stage_stream(pad), 4, 24, 1)
        assert status == 0 and np.array_equal(got, first), pad
    s0 = LC.stage_stream(0)
    assert s0.count(b"\xff\x00") >= 8 and s0.count(b"\xff\xd0") == 1 and max(LC.LONG[0][15:]) == 2       # stuffed bytes, restarts, 16-bit codes
    assert F.jpegll_decode_frame(LC.stage_stream(LC.T + 3), 4, 24, 1)[1] == 0
    with pytest.raises(ValueError):
        F.jpegll_decode_frame(b"", 0, 3, 1)
    with pytest.raises(ValueError):
        F.jpegll_decode_frame(b"", 3, 3, 2)


def test_a_sample_that_wraps_is_a_status_not_a_masked_value():
    """255 + 1 and 0 - 1: a decoder that masks to 8 bits returns 0 and 255; sums are kept modulo 2^16 in full and the range check judges"""
    want = LC.expected()
    for name in ("data_sample_256", "data_sample_minus_1", "data_category_9", "data_category_15", "data_category_16",
                 "data_category_16_twice_is_still_outside", "data_first_column_outside", "data_last_sample_outside"):
        c = next(c for c in LC.corpus() if c.name == name)
        assert want[name][1] == 3 and F.jpegll_decode_frame(c.buf, c.H, c.W, c.samples)[1] == 3, name


# ---- the encoder ----------------------------------------------------------------------------------------------------------------------------
def test_encoder_round_trips_and_is_what_the_corpus_holds():
    rng = np.random.default_rng(8)
    for H, W, C, rows, tables in ((1, 1, 1, 0, None), (5, 9, 3, 2, [LC.K3, LC.NINE, LC.LONG]), (7, 130, 1, 1, LC.FLAT5), (4, 3, 3, 9, [LC.LONG])):
        a = rng.integers(0, 256, (H, W) if C == 1 else (H, W, C), dtype=np.uint8)
        buf = F.jpegll_encode_frame(a, rows, tables)
        assert buf[:4] == b"\xff\xd8\xff\xc3" and buf[-2:] == b"\xff\xd9"
        for decode in (F.jpegll_decode_frame, LC.reference_decode):
            got, status = decode(buf, H, W, C)
            assert status == 0 and np.array_equal(got, a), (H, W, C, decode.__name__)
        if tables is None or not isinstance(tables, list) or len(tables) == 1:  # (one table: the very bytes the hand-written builder writes)
            assert buf == LC.build(H, W, C, LC.diffs_of(a, rows), tables=[F.JPEGLL_DEFAULT_TABLE] if tables is None else (tables if isinstance(tables, list) else [tables]),
                                   rows=rows)
    assert F.JPEGLL_DEFAULT_TABLE == (list(LC.K3[0]), list(LC.K3[1]))
    blob, off, ln = F.jpegll_record([b"abc", b"de"])
    assert blob.tobytes() == b"abcde" and off.tolist() == [0, 3] and ln.tolist() == [3, 2] and F.jpegll_record is F.rle_record
    for bad in (np.zeros((2, 2), np.uint16), np.zeros((2, 2, 2), np.uint8), np.zeros((0, 2), np.uint8)):
        with pytest.raises(ValueError):
            F.jpegll_encode_frame(bad)
    with pytest.raises(ValueError):
        F.jpegll_encode_frame(np.zeros((400, 200), np.uint8), 400)          # 80000 samples do not fit DRI
    with pytest.raises(ValueError):
        F.jpegll_encode_frame(np.zeros((2, 2), np.uint8), tables=LC.flat_table(range(5), 3))


# ---- the core under the sanitizers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verify_jpegll(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jpegll") / "verify_jpegll"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_jpegll.cpp"), "-o", str(exe)])
    return str(exe)


def test_core_decodes_the_whole_corpus_under_the_sanitizers(verify_jpegll, tmp_path):
    path = tmp_path / "corpus.bin"
    stage = [LC.Case(f"stage_{pad}", LC.stage_stream(pad), 4, 24, 1) for pad in (0, 1, 15, 16, 17, LC.T - 2, LC.T, LC.T + 16)]
    want = {**LC.expected(), **{c.name: LC.reference_decode(c.buf, c.H, c.W, c.samples) for c in stage}}
    cases = LC.corpus() + tuple(stage)
    LC.write_corpus(path, cases, want)
    r = subprocess.run([verify_jpegll, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.strip() == f"{len(cases)} cases ok"


# ---- the library's entry points (no GPU needed: a null handle is refused before anything else) ------------------------------------------
def test_library_exports_and_refuses_without_a_handle():
    from tee_optical_flow_amd.dense_flow import DenseFlow
    assert {"tf_jpegll_decode", "tf_hold_frames_jpegll"} <= set(_lib.EXPORTED_SYMBOLS)
    L = _lib.load()
    assert L.tf_jpeg_stage_bytes() == LC.T
    blob, off, ln = F.jpegll_record([LC.stage_stream(0)])
    out, status = np.full(96, 7, np.uint8), np.full(1, -7, np.int32)
    assert L.tf_jpegll_decode(None, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, 4, 24, 1, out.ctypes.data, status.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert L.tf_hold_frames_jpegll(None, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, 1, 4, 24, 1, 1, 0, status.ctypes.data) == _lib.TF_ERR_INVALID_ARG
    assert (out == 7).all() and status[0] == -7 and L.tf_abi_version() == 2
    for name in ("jpeg_lossless_decode", "hold_frames_jpeg_lossless"):
        assert callable(getattr(DenseFlow, name))
    assert F.JPEG_LOSSLESS_TRANSFER_SYNTAXES == ("1.2.840.10008.1.2.4.70", "1.2.840.10008.1.2.4.57")


# ---- dicom_jpegll_frames ---------------------------------------------------------------------------------------------------------------------
def _item(data):
    return b"\xfe\xff\x00\xe0" + len(data).to_bytes(4, "little") + data


END = b"\xfe\xff\xdd\xe0\x00\x00\x00\x00"


def _dataset(streams, H, W, samples, uid=F.JPEG_LOSSLESS_TRANSFER_SYNTAXES[0], bits=8, photometric="RGB", **more):
    from types import SimpleNamespace
    even = [s + b"\x00" * (len(s) & 1) for s in streams]                    # (a fragment has even length: PS3.5 A.4; the pad follows EOI)
    return SimpleNamespace(file_meta=SimpleNamespace(TransferSyntaxUID=uid), PixelData=_item(b"") + b"".join(_item(e) for e in even) + END,
                           Rows=H, Columns=W, SamplesPerPixel=samples, BitsAllocated=bits, PhotometricInterpretation=photometric, **more)


class NoFileMeta:
    Rows, Columns = 1, 1


def test_dicom_jpegll_frames_on_stub_datasets():
    from tee_optical_flow_amd import pipeline as P
    from tee_optical_flow_amd.exceptions import DICOMReadError
    cases = [c for c in LC.golden()[0] if (c.H, c.W, c.samples) == (17, 65, 3)][:3]
    want = np.stack([LC.expected()[c.name][0] for c in cases])
    for uid in F.JPEG_LOSSLESS_TRANSFER_SYNTAXES:                           # both transfer syntaxes
        got = P.dicom_jpegll_frames(_dataset([c.buf for c in cases], 17, 65, 3, uid=uid, NumberOfFrames="3"))    # (NumberOfFrames is an IS: a string)
        assert isinstance(got, P.JpegLosslessFrames) and isinstance(got, P.RleFrames) and not isinstance(got, P.JpegFrames)
        assert got.shape == (3, 17, 65) and got.samples == 3 and got.photometric == "RGB" and got.blob.dtype == np.uint8 and got.off.dtype == np.uint64
        assert np.array_equal(got.decode(), want)                          # PIL where it imports and takes the stream, else the twin
        assert P._rle_form(got, "RGB") == ("RGB", None) and P._rle_form(got, "YBR_FULL") == ("YBR_FULL", None)
    grey = next(c for c in LC.golden()[0] if (c.H, c.W, c.samples) == (17, 65, 1))
    one = P.dicom_jpegll_frames(_dataset([grey.buf], 17, 65, 1, photometric="MONOCHROME2"))               # no NumberOfFrames: one frame
    assert one.shape == (1, 17, 65) and np.array_equal(one.decode()[0], LC.expected()[grey.name][0])
    two = P.dicom_jpegll_frames(_dataset([grey.buf, grey.buf], 17, 65, 1, photometric="MONOCHROME2", NumberOfFrames=2))
    assert P._rle_form(two, "MONOCHROME2") == ("GRAY", None) and P._rle_form(one, "MONOCHROME2")[0] is None
    # refused: 16-bit samples, another transfer syntax, no file_meta -- read through pixel_array as ever
    assert P.dicom_jpegll_frames(_dataset([c.buf for c in cases], 17, 65, 3, bits=16, NumberOfFrames=3)) is None
    assert "BitsAllocated = 16" in P._jpegll_refusal(_dataset([], 1, 1, 3, bits=16))
    assert "SamplesPerPixel = 4" in P._jpegll_refusal(_dataset([], 1, 1, 4))
    for uid in (F.JPEG_BASELINE_TRANSFER_SYNTAX, F.RLE_TRANSFER_SYNTAX, "1.2.840.10008.1.2.1", "1.2.840.10008.1.2.4.80"):
        assert P.dicom_jpegll_frames(_dataset([c.buf for c in cases], 17, 65, 3, uid=uid, NumberOfFrames=3)) is None
    assert P.dicom_jpeg_frames(_dataset([c.buf for c in cases], 17, 65, 3, NumberOfFrames=3)) is None
    assert P.dicom_rle_frames(_dataset([c.buf for c in cases], 17, 65, 3, NumberOfFrames=3)) is None
    assert P.dicom_jpegll_frames(NoFileMeta()) is None
    with pytest.raises(ValueError):                                        # three fragments for two frames and no offset table
        P.dicom_jpegll_frames(_dataset([c.buf for c in cases], 17, 65, 3, NumberOfFrames=2))
    bad = P.JpegLosslessFrames(got.blob[:-40].copy(), got.off, np.array([got.len[0], got.len[1], got.len[2] - 40], np.uint32), (3, 17, 65), 3)
    with pytest.raises(DICOMReadError, match="JPEG Lossless frame 2 did not decode: status 3"):
        bad.decode()


def test_a_refused_dataset_is_logged_once(caplog):
    from tee_optical_flow_amd import pipeline as P
    P._jpegll_fallbacks.clear()
    ds = _dataset([], 1, 1, 3, bits=16)
    with caplog.at_level("WARNING", logger=P.logger.name):
        assert P._stored_jpegll(ds, "x.dcm") is None and P._stored_jpegll(ds, "y.dcm") is None
        assert P._stored_jpegll(_dataset([], 1, 1, 3, uid="1.2.840.10008.1.2.1"), "z.dcm") is None
    assert [r.getMessage() for r in caplog.records].count(
        "JPEG Lossless pixel data not decoded on the device, the host decodes it instead: JPEG Lossless pixel data with BitsAllocated = 16: "
        "only 8-bit samples are decoded from the stored bytes") == 1 and len(caplog.records) == 1
    assert not P._jpeg_fallbacks                                           # (its own set and wording: the Baseline one is untouched)
    P._jpegll_fallbacks.clear()


def test_npz_study_may_carry_jpeg_lossless_in_nparrs_place(tmp_path):
    from tee_optical_flow_amd import pipeline as P
    from tee_optical_flow_amd.exceptions import DICOMReadError
    cases = [c for c in LC.golden()[0] if (c.H, c.W, c.samples) == (17, 65, 3)][:4]
    want = np.stack([LC.expected()[c.name][0] for c in cases])
    blob, off, ln = F.jpegll_record([c.buf for c in cases])
    path = str(tmp_path / "s.npz")
    np.savez(path, jpegll_blob=blob, jpegll_off=off, jpegll_len=ln, rows=17, cols=65, samples=3, photometric="YBR_FULL", pixel_spacing=0.05, frame_rate=40.0)
    stored = P.read_study_stored(path)
    assert isinstance(stored[0], P.JpegLosslessFrames) and stored[1] == "YBR_FULL" and stored[0].shape == (4, 17, 65) and stored[0].photometric == "YBR_FULL"
    arr, md, pid, hr = P.read_study(path)                                  # frames="host": the host decodes and converts as for any stored array
    assert np.array_equal(arr, F.ybr_full_to_rgb(want)) and md["pixel_spacing"] == 0.05
    np.savez(path, jpegll_blob=blob, jpegll_off=off, jpegll_len=ln, rows=17, cols=65, samples=3)
    assert np.array_equal(P.read_study(path)[0], want)
    np.savez(path, jpegll_blob=blob, jpegll_off=off, jpegll_len=ln, rows=17, cols=65)
    with pytest.raises(DICOMReadError, match="samples"):
        P.read_study_stored(path)
    np.savez(path, jpegll_blob=blob[:100], jpegll_off=off, jpegll_len=ln, rows=17, cols=65, samples=3)
    with pytest.raises(DICOMReadError, match="inside jpegll_blob"):
        P.read_study(path)
