"""The stream batch that inflate and RLE share (csrc/teeflow_streams_core.h) without a GPU: its span walk and table builder under the
address and undefined-behaviour sanitizers (tests/csrc/verify_streams.cpp, a stand-alone program): empty batches, one stream, every
lo & 15, off + len at and one past the 63-bit limit, a length at and one past the cap, both column layouts."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_span_walk_and_table_builder_under_the_sanitizers(tmp_path):
    exe = tmp_path / "verify_streams"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tee_optical_flow_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "verify_streams.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    m = re.fullmatch(r"(\d+) checks ok", r.stdout.strip())
    assert m and int(m.group(1)) > 10000, r.stdout
