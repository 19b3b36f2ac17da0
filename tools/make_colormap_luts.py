#!/usr/bin/env python
"""Writes tee_optical_flow_amd/colormap_luts.json: the 256-entry RGB tables (float64 [256,3]) of the matplotlib colormaps the
rad/long overlay uses when matplotlib is not importable: bwr and BrBG (the reference's defaults), PiYG and viridis.  They are
matplotlib's own tables, read through its public interface (an integer array indexes a colormap's table directly), kept as text:
json writes a float64 with repr, the shortest decimal string that reads back as the same bits;
tests/test_overlay_cpu.py checks the file against the installed matplotlib.

Why text and not an .npz: the file ships inside the package, and this repository keeps binary files to the test vectors under
tests/golden/.  As text the four tables can be read and diffed in review (a matplotlib release that changed a table would show as
changed rows), the loader needs no numpy archive code path, and nothing is lost: the round trip is bit-exact and asserted below.

    python tools/make_colormap_luts.py
"""
import json
import os

import matplotlib
import numpy as np

NAMES = ("bwr", "BrBG", "PiYG", "viridis")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tee_optical_flow_amd", "colormap_luts.json")

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
