"""Randomised parity of the device WASE compensation with numpy: tools/fuzz_wase.py draws the flow and frame counts, shapes near the
kernels' chunk, piece and scan-pass sizes, mask densities, zero fractions, the scale, the entry (host pointers or torch device
tensors) and a data family, and compares backgrounds and compensated flows with numpy bit for bit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 150


@pytest.mark.parametrize("seed", [1, 2])
def test_random_wase_cases_match_numpy(seed):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_wase.py"), str(CASES), str(seed)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{CASES}/{CASES} cases identical" in r.stdout
