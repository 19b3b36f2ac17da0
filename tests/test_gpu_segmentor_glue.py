"""The SAM segmentor's frame glue on the device (tf_segmentor_input / tf_segmentor_classmap, DenseFlow.segmentor_input /
segmentor_classmap, predict_movie's engine path): bit-equal to what PIL and torch on the CPU compute (tests/golden/segmentor_glue.npz)
and to the numpy twins at study sizes, on both solver handles, beside a submitted study on the same engine, and through predict_movie.
No tolerance anywhere.  The cases are tests/segmentor_glue_cases.py; they exchange device pointers with torch, so they run in one
child process that imports torch before the library (one HIP runtime for both), once for the module, and every case is a test here."""
import json
import os
import subprocess
import sys

import pytest

from tests.segmentor_glue_cases import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results():
    r = subprocess.run([sys.executable, "-m", "tests.segmentor_glue_cases"], cwd=ROOT, capture_output=True, text=True,
                       env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_case(results, name):
    seconds, outcome = results[name]
    print(f"{name}: {seconds} s in the child process")
    assert outcome == "ok", outcome
    assert seconds < 10.0


def test_every_case_ran(results):
    assert sorted(results) == sorted(c[0] for c in CASES) and len(results) >= 50
