"""JPEG Baseline on the device (tf_jpeg_decode, tf_hold_frames_jpeg; DenseFlow.jpeg_decode, hold_frames_jpeg): the four k_jpeg_* kernels
over the whole corpus of tests/jpeg_cases.py against its independent reference decoder, what hold_frames_jpeg holds against
frames.ingest_host of the decoded frames and against the recorded digests of Pillow's RGB, the walk of a stream across the stage
boundary, restart intervals, scratch batches, mixed good and bad frames, and a study call on the token -- np.array_equal, no tolerance
anywhere.  No case provokes a fault: a malformed stream is an input the bounds-checked decoder refuses, and tests/test_jpeg_cpu.py runs
the same core over the same corpus under the sanitizers.  PIL is not needed."""
import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests import jpeg_cases as JC

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
    want = JC.expected()
    c0 = cases[0]
    out, status = eng.jpeg_decode(F.jpeg_record([c.buf for c in cases]), c0.H, c0.W, c0.samples)
    for i, c in enumerate(cases):
        arr, st = want[c.name]
        assert status[i] == st, (what, c.name, int(status[i]), st)
        assert np.array_equal(out[i], arr), (what, c.name)                 # (a frame that fails: zeros, as the reference gives)


def test_whole_corpus_batched_by_shape(eng):
    for shape, cases in _by_shape(JC.corpus()).items():
        _check(eng, cases, shape)
    assert eng.counter("jpeg_bytes") > 0 and eng.counter("jpeg_entropy_us") >= 0


def test_every_fifth_case_frame_by_frame(eng):
    for c in JC.corpus()[::5]:
        _check(eng, [c], "alone")


def test_stream_walks_across_the_stage_boundary(eng):
    """a COM segment of 0 ... T + 16 bytes in front: the stuffed FF bytes, the RSTn markers and the 16-bit codes of the stream sit on
    every offset of the stage boundary; the pixels do not change.  One call, every stream at its own alignment in the blob."""
    want, st = JC.reference_decode(JC.stage_stream(0), 16, 16, 1)
    assert st == 0
    out, status = eng.jpeg_decode(F.jpeg_record([JC.stage_stream(pad) for pad in range(JC.T + 17)]), 16, 16, 1)
    assert not status.any()
    assert all(np.array_equal(o, want) for o in out)


def test_forty_intervals_equal_the_stream_without_dri(eng):
    rng = np.random.default_rng(40)
    blocks = JC._blocks(rng, 40)
    a = JC.encode(16, 160, blocks, ri=1, fill=2)
    b = JC.encode(16, 160, blocks)
    assert a.count(b"\xff\xd0") + a.count(b"\xff\xd7") >= 9
    out, status = eng.jpeg_decode(F.jpeg_record([a, b]), 16, 160, 1)
    assert not status.any() and np.array_equal(out[0], out[1])
    assert np.array_equal(out[0], JC.reference_decode(b, 16, 160, 1)[0])


def test_seventy_frames_in_three_or_more_scratch_batches(eng):
    rng = np.random.default_rng(70)
    frames = [JC.encode(64, 64, JC._blocks(rng, 16 * 6), sampling=((2, 2), (1, 1), (1, 1)), ri=(i % 5)) for i in range(70)]
    want = np.stack([JC.reference_decode(f, 64, 64, 3)[0] for f in frames[::7]])
    whole, status = eng.jpeg_decode(F.jpeg_record(frames), 64, 64, 3)
    assert not status.any()
    before = eng.counter("jpeg_batches")
    eng.set_tuning("jpeg_batch_kib", 30 * 24)                              # a frame's coefficients take 64 * 64 * 3 * 2 B = 24 KiB: 30 frames a batch
    try:
        cut, status = eng.jpeg_decode(F.jpeg_record(frames), 64, 64, 3)
        assert eng.counter("jpeg_batches") - before == 3
        eng.set_tuning("jpeg_batch_kib", 1)                                # less than one frame: a frame a batch
        single, status1 = eng.jpeg_decode(F.jpeg_record(frames[:9]), 64, 64, 3)
    finally:
        eng.set_tuning("jpeg_batch_kib", 0)
    assert not status.any() and not status1.any()
    assert np.array_equal(cut, whole) and np.array_equal(single, whole[:9]) and np.array_equal(whole[::7], want)


@pytest.mark.parametrize("flip", [False, True])
def test_hold_frames_jpeg_equals_ingest_of_the_decoded_frames(eng, flip):
    want = JC.expected()
    for (H, W, samples), cases in _by_shape([c for c in JC.corpus() if want[c.name][1] == 0]).items():
        cases = cases[:6]
        decoded = np.stack([want[c.name][0] for c in cases])
        rec = F.jpeg_record([c.buf for c in cases])
        for form in (("GRAY",) if samples == 1 else ("RGB", "YBR_FULL")):
            tok = eng.hold_frames_jpeg(rec, H, W, samples, form=form, flip=flip)
            assert tok.shape == (len(cases), H, W, 3)
            assert np.array_equal(eng.download_frames(), F.ingest_host(decoded, form, flip)), (H, W, form, flip)
        if samples == 3:
            eng.hold_frames_jpeg(rec, H, W, 3, form="YBR_FULL", color="libjpeg", flip=flip)
            assert np.array_equal(eng.download_frames(), F.ingest_host(F.ycc_to_rgb_libjpeg(decoded), "RGB", flip)), (H, W, flip)


def test_hold_with_libjpeg_colour_gives_the_recorded_rgb(eng):
    cases, shas = JC.golden()
    for c in [c for c in cases if c.samples == 3][::3]:
        eng.hold_frames_jpeg(F.jpeg_record([c.buf]), c.H, c.W, 3, form="YBR_FULL", color="libjpeg")
        assert JC.sha(eng.download_frames()[0]) == shas[c.name][1], c.name
    for c in [c for c in cases if c.samples == 1][::5]:
        eng.hold_frames_jpeg(F.jpeg_record([c.buf]), c.H, c.W, 1, form="GRAY")
        assert JC.sha(eng.download_frames()[0][..., 0]) == shas[c.name][1], c.name


def test_mixed_good_and_bad_frames(eng):
    want = JC.expected()
    cases = [c for c in JC.corpus() if (c.H, c.W, c.samples) == (8, 16, 1)]
    assert {want[c.name][1] for c in cases} == {0, 1, 2, 3}
    rec = F.jpeg_record([c.buf for c in cases])
    out, status = eng.jpeg_decode(rec, 8, 16, 1)
    assert status.tolist() == [want[c.name][1] for c in cases]
    for i, c in enumerate(cases):
        assert np.array_equal(out[i], want[c.name][0]), c.name             # good outputs valid, bad ones untouched (the zeros they were)
    # the C call with an output full of a sentinel: a bad frame's slot is not written, by zeros or anything else
    blob, off, ln = (np.ascontiguousarray(a) for a in rec)
    if blob.size == 0:
        blob = np.zeros(1, np.uint8)
    raw, st = np.full((len(cases), 8, 16), 0xA5, np.uint8), np.full(len(cases), -7, np.int32)
    rc = eng._L.tf_jpeg_decode(eng._h, blob.ctypes.data, off.ctypes.data, ln.ctypes.data, len(cases), 8, 16, 1, raw.ctypes.data, st.ctypes.data)
    assert rc == _lib.TF_ERR_INVALID_ARG and st.tolist() == status.tolist()
    for i, c in enumerate(cases):
        assert np.array_equal(raw[i], want[c.name][0]) if st[i] == 0 else (raw[i] == 0xA5).all(), c.name
    good = next(c for c in cases if want[c.name][1] == 0)
    tok = eng.hold_frames_jpeg(F.jpeg_record([good.buf] * 3), 8, 16, 1, form="GRAY")
    held, gen = eng.download_frames(), eng._held_frames_shape()[3]
    with pytest.raises(OpticalFlowCalculationError, match=r"frame \d+ did not decode: status [123]"):
        eng.hold_frames_jpeg(rec, 8, 16, 1, form="GRAY")
    assert eng._held_frames_shape() == (3, 8, 16, gen) and np.array_equal(eng.download_frames(), held)
    assert tok.checked(eng, eng._held_frames_shape(), 1) is tok             # the token is still good
    with pytest.raises(OpticalFlowCalculationError):
        eng.hold_frames_jpeg(F.jpeg_record([good.buf]), 8, 16, 1, form="RGB")          # samples against the form
    with pytest.raises(OpticalFlowCalculationError):
        eng.hold_frames_jpeg(F.jpeg_record([good.buf]), 8, 16, 1, form="GRAY", color="libjpeg")
    with pytest.raises(OpticalFlowCalculationError):
        eng.jpeg_decode(F.jpeg_record([good.buf]), 8, 70000, 1)
    assert eng._held_frames_shape() == (3, 8, 16, gen)
    # the library's own refusals, behind the wrapper's: (N, H, W, samples, form, color) -> TF_ERR_INVALID_ARG before any GPU work
    b1, o1, l1 = (np.ascontiguousarray(a) for a in F.jpeg_record([good.buf]))
    st1, out1 = np.full(1, -7, np.int32), np.full(8 * 16, 0xA5, np.uint8)
    uploaded = eng.counter("frames_upload_bytes")
    hold = lambda N, H, W, samples, form, color, p=b1.ctypes.data: eng._L.tf_hold_frames_jpeg(eng._h, p, o1.ctypes.data, l1.ctypes.data, N, H, W, samples, form, color,
                                                                                         0, st1.ctypes.data)
    for args in ((1, 8, 16, 1, 3, 0), (1, 8, 16, 1, -1, 0), (1, 8, 16, 1, 1, 2), (1, 8, 16, 1, 1, -1), (1, 8, 16, 1, 1, 1), (1, 8, 16, 3, 0, 1),
                 (1, 8, 16, 1, 0, 0), (1, 8, 16, 3, 1, 0), (1, 8, 16, 2, 2, 0), (0, 8, 16, 1, 1, 0), (1, 0, 16, 1, 1, 0), (1, 8, 0, 1, 1, 0),
                 (1, 65536, 16, 1, 1, 0), (1, 8, 65536, 1, 1, 0)):
        assert hold(*args) == _lib.TF_ERR_INVALID_ARG, args
    assert hold(1, 8, 16, 1, 1, 0, p=None) == _lib.TF_ERR_INVALID_ARG
    dec = lambda N, H, W, samples, out=out1.ctypes.data, stp=st1.ctypes.data: eng._L.tf_jpeg_decode(eng._h, b1.ctypes.data, o1.ctypes.data, l1.ctypes.data, N, H, W,
                                                                                               samples, out, stp)
    for args in ((1, 8, 16, 2), (0, 8, 16, 1), (1, 65536, 16, 1), (1, 8, 65536, 1), (1, 8, 16, 1, None), (1, 8, 16, 1, out1.ctypes.data, None)):
        assert dec(*args) == _lib.TF_ERR_INVALID_ARG, args
    assert st1[0] == -7 and (out1 == 0xA5).all() and eng.counter("frames_upload_bytes") == uploaded
    assert eng._held_frames_shape() == (3, 8, 16, gen) and np.array_equal(eng.download_frames(), held)


def test_upload_counter_grows_by_the_compressed_span(eng):
    c = next(c for c in JC.golden()[0] if c.name.startswith("enc_48x64_420"))
    before = eng.counter("frames_upload_bytes")
    eng.hold_frames_jpeg(F.jpeg_record([c.buf, c.buf]), 48, 64, 3, form="YBR_FULL", color="libjpeg")
    assert eng.counter("frames_upload_bytes") - before == 2 * len(c.buf)
    assert eng.counter("jpeg_bytes") == 2 * len(c.buf) + 2 * 48 * 64 * 3


def test_study_payload_from_the_token_equals_the_one_from_hold_frames(eng):
    rng = np.random.default_rng(12)
    base = JC._blocks(rng, 6 * 8 * 3, amp=30, density=0.5)
    frames = []
    for i in range(4):                                                      # four 48 x 64 frames that drift: something to solve
        frames.append(JC.encode(48, 64, [[b[0] + 3 * i] + b[1:] for b in base], sampling=((1, 1),) * 3, q=[6] * 64))
    decoded = np.stack([JC.reference_decode(f, 48, 64, 3)[0] for f in frames])
    tok = eng.hold_frames_jpeg(F.jpeg_record(frames), 48, 64, 3, form="YBR_FULL", color="libjpeg")
    got = eng.calc_study_payload(tok, 1.0)
    tok2 = eng.hold_frames(F.ycc_to_rgb_libjpeg(decoded), "RGB")
    want = eng.calc_study_payload(tok2, 1.0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    eng.release_frames()
