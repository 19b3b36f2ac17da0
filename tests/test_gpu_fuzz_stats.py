"""Randomised parity of the device statistics tail: tools/fuzz_stats.py draws the path, param, sizes, frame counts, mask density, data
family, nbins and percentiles, and compares histograms, percentiles, planes, counts and angle modes with numpy bit for bit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [1, 2])
def test_random_statistics_cases_match_numpy(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_stats.py"), "300", str(seed)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "300/300 cases identical" in r.stdout
