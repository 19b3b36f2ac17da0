"""cv2.cartToPolar against this repository's restatement (analysis.cart_to_polar, the arithmetic teeflow_polar.hip.h runs), bit for bit,
wherever cv2 is importable: the one route from "parity unpinned" to "pinned" for the consumer's polar steps.
cv2 is never installed by the suite; without it the comparison skips with the reason, and a test proves the skip path."""
import importlib.util

import numpy as np
import pytest

from tee_optical_flow_amd import analysis as A


def cv2_probe():
    """(cv2 module or None, reason).  Never imports cv2 unless find_spec says it exists; never installs anything."""
    if importlib.util.find_spec("cv2") is None:
        return None, "cv2 is not importable here (importlib.util.find_spec('cv2') is None): cartToPolar parity stays unpinned"
    try:
        import cv2
    except Exception as e:                       # a broken wheel must not fail the suite
        return None, f"cv2 found but import failed: {e!r}"
    return cv2, f"cv2 {cv2.__version__}"


def test_probe_skips_cleanly_without_cv2(monkeypatch):
    real = importlib.util.find_spec
    monkeypatch.setattr(importlib.util, "find_spec", lambda name, *a, **k: None if name == "cv2" else real(name, *a, **k))
    mod, reason = cv2_probe()
    assert mod is None and "unpinned" in reason


def _inputs():
    rng = np.random.default_rng(17)
    x = rng.normal(0, 3, (64, 257)).astype(np.float32)
    y = rng.normal(0, 3, (64, 257)).astype(np.float32)
    x[0, :8] = [0, -0.0, 0, -0.0, -1, 1e-45, -1e-45, 4]
    y[0, :8] = [0, 0, -0.0, -0.0, -0.0, 0, -1e-45, -4]
    x[1] = np.abs(x[1])
    y[1] = 0                                      # the +x axis: angle 0, magnitude not
    x[2] = y[2]                                   # |x| = |y|
    return x, y


def test_cart_to_polar_vs_opencv():
    cv2, reason = cv2_probe()
    if cv2 is None:
        pytest.skip(reason)
    x, y = _inputs()
    mag, ang = cv2.cartToPolar(x, y)
    hm, ha = A.cart_to_polar(x, y)
    assert mag.dtype == ang.dtype == np.float32
    assert np.array_equal(mag.view(np.int32), hm.view(np.int32)), f"{reason}: magnitude differs at {int((mag != hm).sum())} elements"
    assert np.array_equal(ang.view(np.int32), ha.view(np.int32)), f"{reason}: angle differs at {int((ang != ha).sum())} elements"
