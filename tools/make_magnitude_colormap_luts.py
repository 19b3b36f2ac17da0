#!/usr/bin/env python
"""Writes tee_optical_flow_amd/colormap_luts_magnitude.json: the 256-entry RGB table (float64 [256,3]) of 'hot', the colormap of the
reference's single-component magnitude overlay, for use when matplotlib is not importable (analysis.magnitude_colormap_lut).  A second
file beside colormap_luts.json, in the same format and for the same reasons (tools/make_colormap_luts.py): matplotlib's own table,
read through its public interface, kept as text with every float64 written as the shortest decimal string that reads back as the
same bits.  The first file stays what it is: the four tables of the rad/long overlay.  tests/test_single_overlay_cpu.py checks this
file against the installed matplotlib.

    python tools/make_magnitude_colormap_luts.py
"""
import json
import os

import matplotlib
import numpy as np

NAMES = ("hot",)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tee_optical_flow_amd", "colormap_luts_magnitude.json")

luts = {}
for name in NAMES:
    cmap = matplotlib.colormaps[name]
    assert cmap.N == 256, (name, cmap.N)
    luts[name] = np.array(cmap(np.arange(256))[:, :3], np.float64)
with open(OUT, "w") as f:
    f.write('{"source": "matplotlib colormaps, 256 x RGB, float64", "luts": {\n')
    f.write(",\n".join(f'"{name}": [\n' + ",\n".join(json.dumps([float(v) for v in row]) for row in lut) + "]" for name, lut in luts.items()))
    f.write("}}\n")
with open(OUT) as f:
    back = json.load(f)["luts"]
assert all(np.array_equal(np.array(back[name], np.float64), luts[name]) for name in NAMES)
print(f"matplotlib {matplotlib.__version__}: wrote {os.path.normpath(OUT)} ({os.path.getsize(OUT)} bytes)")
