"""Writes tests/golden/deflate_digests.json: the length and SHA-256 of zlib.compress(raw, 9) for every case of tests/deflate_cases.py,
made with zlib 1.2.11 (the file records the version that made it).  Run from the repository root:
    python tests/golden/make_deflate_digests.py"""
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import deflate_cases as DC  # noqa: E402

if __name__ == "__main__":
    out = {"zlib": zlib.ZLIB_RUNTIME_VERSION, "cases": {c.name: DC.digest(zlib.compress(c.raw, 9)) for c in DC.cases()}}
    with open(DC.DIGESTS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out['cases'])} cases, zlib {out['zlib']}")
