#!/usr/bin/env python3
"""Writes tests/golden/deepflow_ref64_measured.json: per case id of tests/deepflow_ref64_cases.py, the deviation of
oracle/deepflow_oracle.c from the float64 reference tests/deepflow_ref64.py, per output.

It runs the oracle and the reference only: no device code, no GPU.  Every tolerance of tests/test_deepflow_ref64_stages_cpu.py and
tests/test_gpu_deepflow_ref64.py is a fixed multiple of a number in this file (deepflow_ref64_cases.tol), so it is rewritten only when a
case is added or the reference or the oracle is changed on purpose -- never to make a device result pass."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from tests import deepflow_ref64_cases as K  # noqa: E402

O.build()
out = {cid: K.measure(O, cid) for cid in K.all_ids()}
with open(K.RECORD, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
for cid, m in out.items():
    print(cid, " ".join(f"{k}={v:.3g}" for k, v in m.items()))
