"""Randomised parity of the calls behind the tiled union-find labeller (tf_clean_masks, tf_otsu_masks, tf_av_centroids) with
scipy.ndimage: tools/fuzz_labelling.py draws the call, adversarial frames of 1 x 1 to 80 x 200, ids, min_size on a component's exact
size, mask values and channel counts, and compares every plane bit for bit and every area and centroid exactly; every fifth case also
frame by frame.  One seed of 300 cases, the interpreter's start, the draw and the scipy references included, took 1.8 s (seed 1) and
1.4 s (seed 2) of wall time on one MI355X box, measured once, 2026-10-21; the subprocess timeout is ten times that, rounded to 20 s: a
guard against hangs, not a performance bound."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [1, 2])
def test_random_labelling_cases_match_scipy(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_labelling.py"), "300", str(seed)], capture_output=True, text=True,
                       timeout=20)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "300/300 cases identical" in r.stdout
