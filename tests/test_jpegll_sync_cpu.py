"""The split entropy decode of JPEG Lossless without a GPU: csrc/teeflow_jpegll_sync_core.h run the way the kernels run it by a
stand-alone program under the sanitizers (tests/csrc/verify_jpegll_sync.cpp, exact-size buffers) over the whole corpus of
tests/jpegll_cases.py and the streams of tests/jpegll_sync_cases.py, against the independent reference decoder, with rounds enough to
converge and with none; and the properties that make those streams worth running on the GPU, asserted here so that
tests/test_gpu_jpegll_sync.py cannot quietly miss its targets."""
import os
import subprocess

import numpy as np
import pytest

from tee_optical_flow_amd import _lib
from tee_optical_flow_amd import frames as F

from tests import jpegll_cases as LC
from tests import jpegll_sync_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256                                                                # piece slots a thread block hands exits through within one round (tfsync::BLOCK)


@pytest.fixture(scope="module")
def verify_sync(tmp_path_factory):
    exe = tmp_path_factory.mktemp("jpegll_sync") / "verify_jpegll_sync"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_jpegll_sync.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def runs(verify_sync, tmp_path_factory):
    """{R: {case name: (status, intervals, most pieces of an interval, last round that changed a piece, fallbacks)}} of the program over
    everything, which also checked every status and output against the reference decoder"""
    path = tmp_path_factory.mktemp("jpegll_sync_corpus") / "corpus.bin"
    cases = LC.corpus() + SC.cases()
    LC.write_corpus(path, cases, {**LC.expected(), **SC.expected()})
    out = {}
    for R in (1 << 20, SC.R, 0):
        r = subprocess.run([verify_sync, str(path), str(R)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == f"{len(cases)} cases ok" and len(lines) == len(cases) + 1
        out[R] = {c.name: tuple(int(v) for v in ln.split()[1:]) for c, ln in zip(cases, lines)}
    return out


def test_split_decode_equals_the_reference_on_everything_under_the_sanitizers(runs):
    """the committed corpus (92 encoder-made streams), the hand-made streams, every malformed one and the streams of jpegll_sync_cases:
    arrays and statuses, converged and with no round at all"""
    want = {**LC.expected(), **SC.expected()}
    assert len(LC.golden()[0]) == 92 and sum(1 for c in LC.corpus() if want[c.name][1] != 0) == 159
    for R, rows in runs.items():
        assert len(rows) == len(LC.corpus()) + len(SC.cases())
        for name, (status, nint, pieces, last, fallbacks) in rows.items():
            assert status == want[name][1], (R, name)
            if R == 0 and status == 0:                                     # no round: every interval of more than one piece fell back
                assert fallbacks <= nint and (fallbacks > 0) == (pieces > 1), (name, fallbacks, nint, pieces)
            if R == 1 << 20:
                assert fallbacks == 0 and last < R, name


def test_library_export_and_the_cases_file_agree():
    assert "tf_jpegll_segment_bytes" in _lib.EXPORTED_SYMBOLS
    assert _lib.load().tf_jpegll_segment_bytes() == _lib.JPEGLL_SEGMENT_BYTES == SC.S
    assert _lib.JPEGLL_SYNC_ROUNDS == SC.R


def test_bit_offset_walk_puts_a_symbol_boundary_on_every_bit_around_the_first_cut(runs):
    walk = SC.bit_offset_walk()
    assert [c.name for c in walk] == [f"walk_{k}" for k in range(8 * SC.S + 1)]
    code0 = LC._codes(LC.LONG)[0]
    assert code0[1] == 1                                                   # LONG's code for category 0 is one bit
    for k, c in enumerate(walk):
        arr, status = SC.expected()[c.name]
        assert status == 0 and (arr[0, :k] == 128).all() and (k == 0 or arr[0, k] != 128)
        data = c.buf[SC.scan_offset(c.buf):-2]
        bits = "".join(f"{b:08b}" for b in data.replace(b"\xff\x00", b"\xff"))
        assert bits[:k] == str(code0[0]) * k and SC.pieces(c.buf) >= 3     # symbol k starts at bit k; cuts at bits 256 and 512 have data behind them
        assert runs[1 << 20][c.name][0] == 0


def test_the_search_finds_stuffing_at_a_cut_of_both_kinds():
    straddle, behind = SC.stuffing_cases()
    assert len(straddle) == 3 and len(behind) == 3
    for c in straddle:
        o = SC.scan_offset(c.buf)
        hit = SC.stuffing_at_cuts(c.buf)[0]
        assert hit and all(c.buf[o + cut - 1] == 0xFF and c.buf[o + cut] == 0 and cut % SC.S == 0 for cut in hit)
    for c in behind:
        o = SC.scan_offset(c.buf)
        hit = SC.stuffing_at_cuts(c.buf)[1]
        assert hit and all(c.buf[o + cut - 2:o + cut] == b"\xff\x00" and cut % SC.S == 0 for cut in hit)
    assert all(SC.expected()[c.name][1] == 0 for c in straddle + behind)


def test_table_cases_name_three_two_and_one_code(runs):
    three, two, one = SC.table_cases()
    sel = lambda c: [c.buf[c.buf.index(b"\xff\xda") + 6 + 2 * i] >> 4 for i in range(3)]
    assert sel(three) == [0, 1, 2] and sel(two) == [0, 1, 1] and sel(one) == [0, 1, 0]
    assert one.buf.count(bytes([0xFF, 0xC4])) == 2                          # two ids, one code: compared by bits and vals, the phase is no part of a state
    for c in (three, two, one):
        assert SC.expected()[c.name][1] == 0 and SC.pieces(c.buf) > 2 * SC.R
    # where the tables differ the phase is guessed 0 and a wrong phase does not correct itself: the truth has to arrive
    assert runs[1 << 20][one.name][3] <= runs[1 << 20][three.name][3]


def test_big_table_cases_span_several_blocks_and_need_a_round_a_block(runs):
    three, two = SC.big_table_cases()
    sel = lambda c: [c.buf[c.buf.index(b"\xff\xda") + 6 + 2 * i] >> 4 for i in range(3)]
    assert sel(three) == [0, 1, 2] and sel(two) == [0, 1, 1]
    same = next(c for c in SC.plain_cases() if c.name == "plain_noise_3")   # the same kind of image under one code
    for c in (three, two):
        assert SC.expected()[c.name][1] == 0 and SC.pieces(c.buf) > (SC.R + 1) * BLOCK
        status, nint, pieces, last, fallbacks = runs[1 << 20][c.name]
        assert fallbacks == 0 and last > SC.R and last >= pieces // BLOCK   # a wrong phase does not correct itself: a round a block
        assert runs[SC.R][c.name][4] == 1 and runs[0][c.name][4] == 1       # the default rounds do not suffice: the serial core serves, exactly
    assert SC.pieces(same.buf) > 4 * BLOCK and runs[1 << 20][same.name][3] <= 4


def test_stubborn_streams_do_not_converge_within_the_default_rounds(runs):
    checker, ramp, big = SC.stubborn_cases()
    for c in (checker, ramp, big):
        assert SC.expected()[c.name][1] == 0 and SC.pieces(c.buf) > 2 * SC.R
    # a block hands the truth through all its pieces in one round, so a stream that never synchronises needs a round per block:
    # the big checkerboard has more blocks than the default rounds and falls back, the small one is served
    assert SC.pieces(big.buf) > (SC.R + 1) * BLOCK
    assert runs[SC.R][big.name][4] == 1 and runs[1 << 20][big.name][3] > SC.R and runs[1 << 20][big.name][4] == 0
    assert runs[SC.R][checker.name][4] == 0 and runs[SC.R][ramp.name][4] == 0
    for c in SC.plain_cases():                                             # noise and speckle, 1 and 3 samples: served with rounds to spare
        assert runs[SC.R][c.name][4] == 0 and runs[1 << 20][c.name][3] * 2 <= SC.R, (c.name, runs[1 << 20][c.name])


def test_smallest_shapes_and_the_data_s_end(runs):
    small = {c.name: c for c in SC.small_cases()}
    assert set(small) == {"small_1x1", "small_one_piece", "small_one_piece_and_a_byte", "small_last_piece_of_one_byte"}
    assert SC.entropy_bytes(small["small_one_piece"].buf) == SC.S and SC.entropy_bytes(small["small_one_piece_and_a_byte"].buf) == SC.S + 1
    assert SC.entropy_bytes(small["small_last_piece_of_one_byte"].buf) == 2 * SC.S + 1
    assert [runs[0][n][2] for n in ("small_1x1", "small_one_piece", "small_one_piece_and_a_byte", "small_last_piece_of_one_byte")] == [1, 1, 2, 3]
    good, early, tail = SC.end_cases()
    want = SC.expected()
    assert want[good.name][1] == 0 and want[early.name][1] == 3 and want[tail.name][1] == 0
    assert len(early.buf) == len(good.buf) - 1 and SC.pieces(early.buf) > 2
    # cut one byte more and the data ends before the last sample's code: still status 3; the garbage is no code of its table
    assert F.jpegll_decode_frame(early.buf, 4, 60, 1)[1] == 3
    assert tail.buf.endswith(b"\xff\x00" * 40 + b"\xff\xd9") and max(LC._codes(LC.SHORT)[s][0] for s in range(9)) < 0b1111
    assert np.array_equal(want[tail.name][0], want[good.name][0])


def test_restart_cases_hold_a_few_long_intervals_and_forty(runs):
    twelve, seven, forty, none = SC.restart_cases()
    rows = runs[1 << 20]
    assert rows[twelve.name][1] == 5 and rows[seven.name][1] == 9 and rows[forty.name][1] == 40 and rows[none.name][1] == 1
    assert rows[twelve.name][2] > 2 * SC.R and rows[seven.name][2] > 2 * SC.R     # pieces of one interval
    want = SC.expected()
    assert np.array_equal(want[forty.name][0], want[none.name][0]) and forty.buf.count(b"\xff\xd0") == 5
