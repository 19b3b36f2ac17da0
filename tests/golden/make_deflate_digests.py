"""Writes tests/golden/deflate_digests.json: the length and SHA-256 of zlib.compress(raw, 9) for every case of tests/deflate_cases.py,
and under "sweeps" one length and SHA-256 per sweep size over the streams of its chunks end to end, made with zlib 1.2.11 (the file
records the version that made it).  An entry that the file holds already must come out as it is: the corpus grows, it does not move.
Run from the repository root:
    python tests/golden/make_deflate_digests.py"""
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import deflate_cases as DC  # noqa: E402

if __name__ == "__main__":
    out = {"zlib": zlib.ZLIB_RUNTIME_VERSION, "cases": {c.name: DC.digest(zlib.compress(c.raw, 9)) for c in DC.cases()},
           "sweeps": {str(n): DC.sweep_digest([zlib.compress(c, 9) for c in DC.sweep(n)]) for n in DC.SWEEP_SIZES}}
    old = {}
    if os.path.exists(DC.DIGESTS):
        with open(DC.DIGESTS) as f:
            old = json.load(f)
    for key in ("cases", "sweeps"):
        moved = [k for k, v in old.get(key, {}).items() if out[key].get(k) != v]
        assert not moved, f"{key}: recorded digests would change or go: {moved[:10]}"
    with open(DC.DIGESTS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out['cases'])} cases ({len(out['cases']) - len(old.get('cases', {}))} new), {len(out['sweeps'])} sweeps, zlib {out['zlib']}")
