"""The split entropy decode of JPEG Lossless on the device (k_jpegll_spec, k_jpegll_sync, k_jpegll_scan, k_jpegll_emit and the serial
fallback k_jpegll_entropy_rest behind tf_set_tuning "jpegll_split" = 2): the whole corpus of tests/jpegll_cases.py and the aimed streams of
tests/jpegll_sync_cases.py against the independent reference decoder and against the serial path ("jpegll_split" = 1), the counters,
the fallback, scratch batches with good and bad frames mixed, and the hold path -- np.array_equal, no tolerance anywhere.  No case
provokes a fault: a malformed stream is an input the bounds-checked decoder answers with a status, and tests/test_jpegll_sync_cpu.py
runs the same core over the same streams under the sanitizers.  Frames are at most 80 x 200."""
import contextlib

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F
from tee_optical_flow_amd.exceptions import OpticalFlowCalculationError

from tests import jpegll_cases as LC
from tests import jpegll_sync_cases as SC

pytestmark = pytest.mark.gpu

R = _lib.JPEGLL_SYNC_ROUNDS


@pytest.fixture(scope="module")
def eng():
    import tee_optical_flow_amd as T
    e = T.DenseFlow(device_id=0)
    yield e
    e.close()


@contextlib.contextmanager
def split(eng, mode, rounds=None):
    eng.set_tuning("jpegll_split", mode)
    if rounds is not None:
        eng.set_tuning("jpegll_sync_rounds", rounds)
    try:
        yield
    finally:
        eng.set_tuning("jpegll_split", 0)
        eng.set_tuning("jpegll_sync_rounds", R)


def _by_shape(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c.H, c.W, c.samples), []).append(c)
    return groups


def _decode(eng, cases):
    c0 = cases[0]
    return eng.jpeg_lossless_decode(F.jpegll_record([c.buf for c in cases]), c0.H, c0.W, c0.samples)


def _check(eng, cases, want, what):
    """the cases in one call down the split path: the reference's arrays and statuses, and the serial path's"""
    with split(eng, 2):
        out, status = _decode(eng, cases)
    with split(eng, 1):
        out1, status1 = _decode(eng, cases)
    for i, c in enumerate(cases):
        arr, st = want[c.name]
        assert status[i] == st == status1[i], (what, c.name, int(status[i]), st, int(status1[i]))
        assert np.array_equal(out[i], arr) and np.array_equal(out1[i], arr), (what, c.name)


def test_whole_corpus_batched_by_shape_and_every_fifth_case_alone(eng):
    want = LC.expected()
    before = eng.counter("jpegll_split_intervals")
    for shape, cases in _by_shape(LC.corpus()).items():
        _check(eng, cases, want, shape)
    assert eng.counter("jpegll_split_intervals") > before
    for c in LC.corpus()[::5]:
        _check(eng, [c], want, "alone")


def test_every_malformed_stream_gets_the_serial_path_s_status(eng):
    want = LC.expected()
    bad = [c for c in LC.corpus() if want[c.name][1] != 0]
    assert len(bad) == 159
    for shape, cases in _by_shape(bad).items():
        with split(eng, 2):
            out, status = _decode(eng, cases)
        with split(eng, 1):
            out1, status1 = _decode(eng, cases)
        assert status.tolist() == status1.tolist() == [want[c.name][1] for c in cases], shape
        assert not out.any() and not out1.any()


def test_bit_offset_walk_and_stuffing_at_a_cut(eng):
    want = SC.expected()
    straddle, behind = SC.stuffing_cases()
    for shape, cases in _by_shape(SC.bit_offset_walk() + straddle + behind).items():
        _check(eng, cases, want, shape)
    for c in SC.small_cases() + SC.end_cases():
        _check(eng, [c], want, c.name)


def test_three_two_and_one_code_on_three_components(eng):
    want = SC.expected()
    _check(eng, list(SC.table_cases()), want, "tables")
    for c in SC.table_cases():
        _check(eng, [c], want, c.name)


def test_differing_tables_over_several_blocks_of_pieces(eng):
    """the phase is part of the state and guessed 0, so the truth travels a block of pieces a round: the default rounds fall back, enough
    rounds serve, and the automatic rule keeps such frames on the serial kernel whatever their length"""
    want = SC.expected()
    same = next(c for c in SC.plain_cases() if c.name == "plain_noise_3")
    for c in SC.big_table_cases():
        _check(eng, [c], want, c.name)
        for rounds, falls in ((R, 1), (16, 0)):
            before = eng.counter("jpegll_serial_fallbacks")
            with split(eng, 2, rounds=rounds):
                out, status = _decode(eng, [c])
            assert status.tolist() == [0] and np.array_equal(out[0], want[c.name][0]), (c.name, rounds)
            assert eng.counter("jpegll_serial_fallbacks") - before == falls, (c.name, rounds)
    _check(eng, list(SC.big_table_cases()) + [same], want, "one batch, the phase in some states only")
    with split(eng, 0):
        assert len(same.buf) > 16384 and all(len(c.buf) > 16384 for c in SC.big_table_cases())
        before = eng.counter("jpegll_split_intervals")
        out, status = _decode(eng, list(SC.big_table_cases()))
        assert not status.any() and eng.counter("jpegll_split_intervals") == before and eng.counter("jpegll_sync_rounds") == 0
        out, status = _decode(eng, list(SC.big_table_cases()) + [same])
        assert not status.any() and eng.counter("jpegll_split_intervals") - before == 1
        for i, c in enumerate(list(SC.big_table_cases()) + [same]):
            assert np.array_equal(out[i], want[c.name][0]), c.name


def test_noise_and_speckle_converge_within_the_default_rounds(eng):
    want = SC.expected()
    for c in SC.plain_cases():
        split_before, fb_before = eng.counter("jpegll_split_intervals"), eng.counter("jpegll_serial_fallbacks")
        with split(eng, 2):
            out, status = _decode(eng, [c])
            assert eng.counter("jpegll_sync_rounds") == R                   # the rounds launched in the last call: one batch
        assert status.tolist() == [0] and np.array_equal(out[0], want[c.name][0]), c.name
        assert eng.counter("jpegll_split_intervals") - split_before == 1 and eng.counter("jpegll_serial_fallbacks") == fb_before, c.name
    with split(eng, 1):
        _decode(eng, [SC.plain_cases()[0]])
        assert eng.counter("jpegll_sync_rounds") == 0                       # the serial path launches none


def test_fallback_with_no_round_and_on_streams_that_do_not_synchronise(eng):
    want = SC.expected()
    cases = list(SC.plain_cases()) + list(SC.restart_cases())
    intervals = {"restart_12_rows": 5, "restart_7_rows_grey": 9, "restart_40_intervals": 40}
    for c in cases:                                                        # no round: every interval of more than one piece falls back
        nint = intervals.get(c.name, 1)
        before = eng.counter("jpegll_serial_fallbacks")
        with split(eng, 2, rounds=0):
            out, status = _decode(eng, [c])
            assert eng.counter("jpegll_sync_rounds") == 0
        assert status.tolist() == [0] and np.array_equal(out[0], want[c.name][0]), c.name
        assert eng.counter("jpegll_serial_fallbacks") - before == nint, c.name   # (every interval of these streams has more than one piece)
    checker, ramp, big = SC.stubborn_cases()
    for c, falls in ((checker, 0), (ramp, 0), (big, 1)):                   # the default rounds: exact whichever path served
        before = eng.counter("jpegll_serial_fallbacks")
        with split(eng, 2):
            out, status = _decode(eng, [c])
        assert status.tolist() == [0] and np.array_equal(out[0], want[c.name][0]), c.name
        assert eng.counter("jpegll_serial_fallbacks") - before == falls, c.name
    for rounds, falls in ((1, 2), (2, 0)):                                  # the small checkerboard and the ramp are one block of pieces each: round 1 carries
        before = eng.counter("jpegll_serial_fallbacks")                    # the truth through it, round 2 finds nothing to change
        with split(eng, 2, rounds=rounds):
            out, status = _decode(eng, [checker, ramp])
        assert not status.any() and np.array_equal(out[0], want[checker.name][0]) and np.array_equal(out[1], want[ramp.name][0])
        assert eng.counter("jpegll_serial_fallbacks") - before == falls, rounds


def test_seventy_frames_in_three_or_more_scratch_batches_good_and_bad_mixed(eng):
    rng = np.random.default_rng(71)
    imgs = rng.integers(0, 256, (70, 17, 23, 3), dtype=np.uint8)
    frames = [F.jpegll_encode_frame(imgs[i], i % 5) for i in range(70)]
    bad = {7: frames[7][:len(frames[7]) // 2] + b"\xff\xd9", 33: b"\xff\xd8\x00", 34: frames[34].replace(b"\xff\xc3", b"\xff\xc1", 1),
           69: frames[69][:-40] + b"\xff\xd9"}
    mixed = [bad.get(i, f) for i, f in enumerate(frames)]
    with split(eng, 1):
        want_out, want_status = eng.jpeg_lossless_decode(F.jpegll_record(mixed), 17, 23, 3)
    assert want_status.tolist() == [{7: 3, 33: 1, 34: 2, 69: 3}.get(i, 0) for i in range(70)]
    before = eng.counter("jpegll_batches")
    eng.set_tuning("jpeg_batch_kib", 69)
    try:
        with split(eng, 2):
            out, status = eng.jpeg_lossless_decode(F.jpegll_record(mixed), 17, 23, 3)
            whole, whole_status = eng.jpeg_lossless_decode(F.jpegll_record(frames), 17, 23, 3)
    finally:
        eng.set_tuning("jpeg_batch_kib", 0)
    assert eng.counter("jpegll_batches") - before >= 6                      # three or more batches a call: the per-piece scratch counts too
    assert status.tolist() == want_status.tolist() and np.array_equal(out, want_out)
    assert not whole_status.any() and np.array_equal(whole, imgs)
    for i in range(70):
        assert np.array_equal(out[i], imgs[i]) if i not in bad else not out[i].any(), i


@pytest.mark.parametrize("flip", [False, True])
def test_hold_path_down_the_split_decode(eng, flip):
    want = SC.expected()
    cases = [c for c in SC.plain_cases() if c.samples == 3] + [SC.stubborn_cases()[2]]
    decoded = np.stack([want[c.name][0] for c in cases])
    with split(eng, 2):
        tok = eng.hold_frames_jpeg_lossless(F.jpegll_record([c.buf for c in cases]), 80, 200, 3, form="RGB", flip=flip)
        got = eng.download_frames()
        assert tok.shape == (len(cases), 80, 200, 3) and np.array_equal(got, F.ingest_host(decoded, "RGB", flip))
        eng.hold_frames(decoded, "RGB", flip=flip)
        assert np.array_equal(eng.download_frames(), got)
        grey = [c for c in SC.plain_cases() if c.samples == 1]
        tok = eng.hold_frames_jpeg_lossless(F.jpegll_record([c.buf for c in grey]), 80, 200, 1, form="GRAY", flip=flip)
        held, gen = eng.download_frames(), eng._held_frames_shape()[3]
        assert np.array_equal(held, F.ingest_host(np.stack([want[c.name][0] for c in grey]), "GRAY", flip))
        early = SC.end_cases()[1]                                          # a failed hold leaves the held frames, generation and tokens intact
        good = SC.end_cases()[0]
        with pytest.raises(OpticalFlowCalculationError, match=r"frame 1 did not decode: status 3"):
            eng.hold_frames_jpeg_lossless(F.jpegll_record([good.buf, early.buf, good.buf]), 4, 60, 1, form="GRAY", flip=flip)
        assert eng._held_frames_shape() == (len(grey), 80, 200, gen) and np.array_equal(eng.download_frames(), held)
        assert tok.checked(eng, eng._held_frames_shape(), 1) is tok
    eng.release_frames()


def test_restart_intervals_of_several_rows_and_forty_intervals(eng):
    want = SC.expected()
    twelve, seven, forty, none = SC.restart_cases()
    for c in (twelve, seven):
        _check(eng, [c], want, c.name)
    _check(eng, [forty, none], want, "forty")
    assert np.array_equal(want[forty.name][0], want[none.name][0])
    before = eng.counter("jpegll_split_intervals")
    with split(eng, 2):
        _decode(eng, [forty, none])
    assert eng.counter("jpegll_split_intervals") - before == 41


def test_the_automatic_rule_keeps_short_intervals_on_the_serial_path(eng):
    """"jpegll_split" = 0: intervals of a row of a small frame are far below any threshold worth measuring, so the call launches what it
    launched before there was a split path"""
    forty = SC.restart_cases()[2]
    before = eng.counter("jpegll_split_intervals")
    with split(eng, 0):
        out, status = _decode(eng, [forty])
        assert eng.counter("jpegll_split_intervals") == before and eng.counter("jpegll_sync_rounds") == 0
    assert status.tolist() == [0] and np.array_equal(out[0], SC.expected()[forty.name][0])
    with pytest.raises(OpticalFlowCalculationError):
        eng.set_tuning("jpegll_split", 3)
