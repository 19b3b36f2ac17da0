"""pydicom's convert_color_space(arr, 'YBR_FULL', 'RGB') against this repository's restatement (frames.ybr_full_to_rgb, the arithmetic
k_ingest runs), over all 2^24 triples, wherever pydicom is importable: the one route from "parity unpinned" to "pinned" for the colour
conversion of frames="device" (DESIGN.md section 2).  pydicom is never installed by the suite; without it the comparison skips with the
reason, and a test proves the skip path."""
import importlib.util

import numpy as np
import pytest

from tee_optical_flow_amd import frames as F

from tests import frames_cases as FC


def pydicom_probe():
    """(convert_color_space or None, reason).  Never imports pydicom unless find_spec says it exists; never installs anything."""
    if importlib.util.find_spec("pydicom") is None:
        return None, "pydicom is not importable here (importlib.util.find_spec('pydicom') is None): YBR_FULL -> RGB parity stays unpinned"
    try:
        import pydicom
        from pydicom.pixel_data_handlers.util import convert_color_space
    except Exception as e:                       # a broken or reorganised install must not fail the suite
        return None, f"pydicom found but its converter did not import: {e!r}"
    return convert_color_space, f"pydicom {pydicom.__version__}"


def test_probe_skips_cleanly_without_pydicom(monkeypatch):
    real = importlib.util.find_spec
    monkeypatch.setattr(importlib.util, "find_spec", lambda name, *a, **k: None if name == "pydicom" else real(name, *a, **k))
    fn, reason = pydicom_probe()
    assert fn is None and "unpinned" in reason


def test_twin_equals_pydicom_over_the_cube():
    convert, reason = pydicom_probe()
    if convert is None:
        pytest.skip(reason)
    cube = FC.cube()
    want = np.asarray(convert(cube.copy(), "YBR_FULL", "RGB"))
    got = F.ybr_full_to_rgb(cube)
    n = int((got != want).any(-1).sum())
    print(f"{reason}: the twin differs from convert_color_space at {n} of 2^24 triples"
          + (f", by at most {int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max())} counts" if n else ""))
    assert want.dtype == np.uint8 and n == 0
