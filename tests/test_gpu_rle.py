"""DICOM RLE Lossless on the device (tf_rle_decode, tf_hold_frames_rle; DenseFlow.rle_decode, hold_frames_rle): k_rle_decode over the
whole corpus of tests/rle_cases.py against its independent decoder, what hold_frames_rle holds against frames.ingest_host of the
decoded frames, a study call and Otsu masks on the RLE token against the same calls on a hold_frames token, a failed call, the refusals
and the counters -- np.array_equal, no tolerance anywhere.  No case provokes a fault: a malformed stream is an input the bounds-checked
decoder refuses, and tests/test_rle_cpu.py runs the same core over the same corpus under the sanitizers.

The cases run in one child process (`python -m tests.rle_cases`: one engine, one call per shape over many small frames) under a time
limit; in it every case has a time limit of its own (rle_cases.CASE_SECONDS), so a kernel that did not end would end the child and
fail the cases from there on, not hold the suite."""
import json
import os
import subprocess
import sys

import pytest

from tests import rle_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def outcomes():
    r = subprocess.run([sys.executable, "-m", "tests.rle_cases"], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    done = {}
    for line in r.stdout.splitlines():                                   # a line a case: what was done before a child that died
        if line.startswith("{"):
            done.update(json.loads(line))
    return r.returncode, r.stderr[-3000:], done


@pytest.mark.parametrize("case", RC.GPU_CASES)
def test_rle_case(outcomes, case):
    rc, err, done = outcomes
    assert case in done, f"the child ended (exit status {rc}) before this case was done:\n{err}"
    seconds, outcome = done[case]
    print(f"{case}: {seconds} s")
    assert outcome == "ok", outcome


def test_the_child_ended_clean(outcomes):
    rc, err, done = outcomes
    assert rc == 0 and sorted(done) == sorted(RC.GPU_CASES), (rc, err)
