"""JPEG Lossless on the device (tf_jpegll_decode, tf_hold_frames_jpegll; DenseFlow.jpeg_lossless_decode, hold_frames_jpeg_lossless):
k_jpeg_marks and the three k_jpegll_* kernels over the whole corpus of tests/jpegll_cases.py against its independent reference decoder,
what hold_frames_jpeg_lossless holds against frames.ingest_host of the decoded frames, the walk of a stream across the stage boundary,
restart intervals, scratch batches, mixed good and bad frames, and a study call on the token -- np.array_equal, no tolerance anywhere.
No case provokes a fault: a malformed stream is an input the bounds-checked decoder refuses, and tests/test_jpegll_cpu.py runs the same
core over the same corpus under the sanitizers.  PIL is not needed."""
import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests import jpegll_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import tee_optical_flow_amd as T
    e = T.DenseFlow(device_id=0)
    yield e
    e.close()


def _by_shape(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c.H, c.W, c.samples), []).append(c)
    return groups


def _check(eng, cases, what):
    want = LC.expected()
    c0 = cases[0]
    out, status = eng.jpeg_lossless_decode(F.jpegll_record([c.buf for c in cases]), c0.H, c0.W, c0.samples)
    for i, c in enumerate(cases):
        arr, st = want[c.name]
        assert status[i] == st, (what, c.name, int(status[i]), st)
        assert np.array_equal(out[i], arr), (what, c.name)                 # (a frame that fails: zeros, as the reference gives)


def test_whole_corpus_batched_by_shape(eng):
    for shape, cases in _by_shape(LC.corpus()).items():
        _check(eng, cases, shape)
    assert eng.counter("jpegll_bytes") > 0 and eng.counter("jpegll_entropy_us") >= 0 and eng.counter("jpegll_restore_us") >= 0


def test_every_fifth_case_frame_by_frame(eng):
    for c in LC.corpus()[::5]:
        _check(eng, [c], "alone")


def test_stream_walks_across_the_stage_boundary(eng):
    """a COM segment of 0 ... T + 16 bytes in front: the stuffed FF bytes, the RSTn markers and the 16-bit codes of the stream sit on
    every offset of the stage boundary; the pixels do not change.  One call, every stream at its own alignment in the blob."""
    want = LC._stage_image()
    out, status = eng.jpeg_lossless_decode(F.jpegll_record([LC.stage_stream(pad) for pad in range(LC.T + 17)]), 4, 24, 1)
    assert not status.any()
    assert all(np.array_equal(o, want) for o in out)


def test_forty_intervals_equal_the_stream_without_dri(eng):
    rng = np.random.default_rng(40)
    img = rng.integers(0, 256, (40, 70, 3), dtype=np.uint8)
    a = LC.build(40, 70, 3, LC.diffs_of(img, 1), rows=1, fill=2)
    b = LC.build(40, 70, 3, LC.diffs_of(img))
    assert a.count(b"\xff\xd0") == 5 and a.count(b"\xff\xd7") == 4          # 39 markers: the numbering wraps four times
    out, status = eng.jpeg_lossless_decode(F.jpegll_record([a, b]), 40, 70, 3)
    assert not status.any() and np.array_equal(out[0], out[1]) and np.array_equal(out[0], img)


def test_seventy_frames_in_three_or_more_scratch_batches(eng):
    rng = np.random.default_rng(70)
    imgs = rng.integers(0, 256, (70, 17, 23, 3), dtype=np.uint8)
    frames = [F.jpegll_encode_frame(imgs[i], i % 5) for i in range(70)]
    whole, status = eng.jpeg_lossless_decode(F.jpegll_record(frames), 17, 23, 3)
    assert not status.any() and np.array_equal(whole, imgs)
    before = eng.counter("jpegll_batches")
    eng.set_tuning("jpeg_batch_kib", 69)                                   # a frame's differences take 17 * 23 * 3 * 2 B = 2346 B: 30 frames a batch
    try:
        cut, status = eng.jpeg_lossless_decode(F.jpegll_record(frames), 17, 23, 3)
        assert eng.counter("jpegll_batches") - before == 3
        eng.set_tuning("jpeg_batch_kib", 1)                                # less than one frame: a frame a batch
        single, status1 = eng.jpeg_lossless_decode(F.jpegll_record(frames[:9]), 17, 23, 3)
        assert eng.counter("jpegll_batches") - before == 12
    finally:
        eng.set_tuning("jpeg_batch_kib", 0)
    assert not status.any() and not status1.any()
    assert np.array_equal(cut, imgs) and np.array_equal(single, imgs[:9])


@pytest.mark.parametrize("flip", [False, True])
def test_hold_frames_jpeg_lossless_equals_hold_frames_of_the_decoded_frames(eng, flip):
    want = LC.expected()
    for (H, W, samples), cases in _by_shape([c for c in LC.corpus() if want[c.name][1] == 0]).items():
        cases = cases[:6]
        decoded = np.stack([want[c.name][0] for c in cases])
        rec = F.jpegll_record([c.buf for c in cases])
        for form in (("GRAY",) if samples == 1 else ("RGB", "YBR_FULL")):
            tok = eng.hold_frames_jpeg_lossless(rec, H, W, samples, form=form, flip=flip)
            assert tok.shape == (len(cases), H, W, 3)
            got = eng.download_frames()
            assert np.array_equal(got, F.ingest_host(decoded, form, flip)), (H, W, form, flip)
            if (H, W) in ((17, 65), (80, 200), (1, 1)):                    # ... and the device's own hold_frames of the decoded array
                eng.hold_frames(decoded, form, flip=flip)
                assert np.array_equal(eng.download_frames(), got), (H, W, form, flip)


def test_mixed_good_and_bad_frames(eng):
    want = LC.expected()
    cases = [c for c in LC.corpus() if (c.H, c.W, c.samples) == (4, 6, 1)]
    assert {want[c.name][1] for c in cases} == {0, 1, 2, 3}
    rec = F.jpegll_record([c.buf for c in cases])
    out, status = eng.jpeg_lossless_decode(rec, 4, 6, 1)
    assert status.tolist() == [want[c.name][1] for c in cases]
    for i, c in enumerate(cases):
        assert np.array_equal(out[i], want[c.name][0]), c.name             # good outputs valid, bad ones untouched (the zeros they were)
    # the C call with an output full of a sentinel: a bad frame's slot is not written, by zeros or anything else
    blob, off, ln = (np.ascontiguousarray(a) for a in rec)
    raw, st = np.full((len(cases), 4, 6), 0xA5, np.uint8), np.full(len(cases), -7, np.int32)
    rc = eng._L.tf_jpegll_decode(eng._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, len(cases), 4, 6, 1, raw.ctypes.data, st.ctypes.data)
    assert rc == _lib.TF_ERR_INVALID_ARG and st.tolist() == status.tolist()
    for i, c in enumerate(cases):
        assert np.array_equal(raw[i], want[c.name][0]) if st[i] == 0 else (raw[i] == 0xA5).all(), c.name
    good = next(c for c in cases if c.name == "hand_good")
    tok = eng.hold_frames_jpeg_lossless(F.jpegll_record([good.buf] * 3), 4, 6, 1, form="GRAY")
    held, gen = eng.download_frames(), eng._held_frames_shape()[3]
    with pytest.raises(OpticalFlowCalculationError, match=r"frame \d+ did not decode: status [123]"):
        eng.hold_frames_jpeg_lossless(rec, 4, 6, 1, form="GRAY")
    wraps = next(c for c in cases if c.name == "data_sample_256")           # the range check alone fails this one, in k_jpegll_rows
    with pytest.raises(OpticalFlowCalculationError, match=r"frame 1 did not decode: status 3"):
        eng.hold_frames_jpeg_lossless(F.jpegll_record([good.buf, wraps.buf, good.buf]), 4, 6, 1, form="GRAY")
    assert eng._held_frames_shape() == (3, 4, 6, gen) and np.array_equal(eng.download_frames(), held)
    assert tok.checked(eng, eng._held_frames_shape(), 1) is tok             # the token is still good
    with pytest.raises(OpticalFlowCalculationError):
        eng.hold_frames_jpeg_lossless(F.jpegll_record([good.buf]), 4, 6, 1, form="RGB")          # samples against the form
    with pytest.raises(OpticalFlowCalculationError):
        eng.jpeg_lossless_decode(F.jpegll_record([good.buf]), 4, 70000, 1)
    assert eng._held_frames_shape() == (3, 4, 6, gen)
    # the library's own refusals, behind the wrapper's: (N, H, W, samples, form) -> TF_ERR_INVALID_ARG before any GPU work
    b1, o1, l1 = (np.ascontiguousarray(a) for a in F.jpegll_record([good.buf]))
    st1, out1 = np.full(1, -7, np.int32), np.full(4 * 6, 0xA5, np.uint8)
    uploaded = eng.counter("frames_upload_bytes")
    hold = lambda N, H, W, samples, form, p=b1.ctypes.data: eng._L.tf_hold_frames_jpegll(eng._h, p, o1.ctypes.data, l1.ctypes.data, N, H, W, samples, form, 0,
                                                                                     st1.ctypes.data)
    for args in ((1, 4, 6, 1, 3), (1, 4, 6, 1, -1), (1, 4, 6, 1, 0), (1, 4, 6, 3, 1), (1, 4, 6, 2, 2), (0, 4, 6, 1, 1), (1, 0, 6, 1, 1), (1, 4, 0, 1, 1),
                 (1, 65536, 6, 1, 1), (1, 4, 65536, 1, 1)):
        assert hold(*args) == _lib.TF_ERR_INVALID_ARG, args
    assert hold(1, 4, 6, 1, 1, p=None) == _lib.TF_ERR_INVALID_ARG
    dec = lambda N, H, W, samples, out=out1.ctypes.data, stp=st1.ctypes.data: eng._L.tf_jpegll_decode(eng._h, b1.ctypes.data, o1.ctypes.data, l1.ctypes.data, N, H, W,
                                                                                                 samples, out, stp)
    for args in ((1, 4, 6, 2), (0, 4, 6, 1), (1, 65536, 6, 1), (1, 4, 65536, 1), (1, 4, 6, 1, None), (1, 4, 6, 1, out1.ctypes.data, None)):
        assert dec(*args) == _lib.TF_ERR_INVALID_ARG, args
    assert st1[0] == -7 and (out1 == 0xA5).all() and eng.counter("frames_upload_bytes") == uploaded
    assert eng._held_frames_shape() == (3, 4, 6, gen) and np.array_equal(eng.download_frames(), held)


def test_upload_counter_grows_by_the_compressed_span(eng):
    c = next(c for c in LC.golden()[0] if c.name == "enc_ri_17x65x3_two")
    before = eng.counter("frames_upload_bytes")
    eng.hold_frames_jpeg_lossless(F.jpegll_record([c.buf, c.buf]), 17, 65, 3, form="RGB")
    assert eng.counter("frames_upload_bytes") - before == 2 * len(c.buf)
    assert eng.counter("jpegll_bytes") == 2 * len(c.buf) + 2 * 17 * 65 * 3


def test_study_payload_from_the_token_equals_the_one_from_hold_frames(eng):
    rng = np.random.default_rng(12)
    base = LC.image("speckle", 48, 64, 3, rng)
    decoded = np.stack([np.roll(base, 2 * i, axis=1) for i in range(4)])     # four 48 x 64 frames that drift: something to solve
    frames = [F.jpegll_encode_frame(f, 8 * (i % 2)) for i, f in enumerate(decoded)]
    tok = eng.hold_frames_jpeg_lossless(F.jpegll_record(frames), 48, 64, 3, form="RGB")
    got = eng.calc_study_payload(tok, 1.0)
    tok2 = eng.hold_frames(decoded, "RGB")
    want = eng.calc_study_payload(tok2, 1.0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    eng.release_frames()


def test_baseline_decoder_still_refuses_an_sof3_stream(eng):
    c = next(c for c in LC.corpus() if c.name == "hand_good")
    out, status = eng.jpeg_decode(F.jpeg_record([c.buf]), 4, 6, 1)
    assert status.tolist() == [2] and not out.any()
    assert F.jpeg_decode_frame(c.buf, 4, 6, 1)[1] == 2
    out, status = eng.jpeg_lossless_decode(F.jpegll_record([c.buf]), 4, 6, 1)   # ... which the new entry point decodes
    assert status.tolist() == [0] and np.array_equal(out[0], LC.expected()[c.name][0])
