"""The decoder's host logic that needs no GPU (qatzip_amd/csrc/qzd_inflate_plan.h: seating by compressed size, the chain
walk, the cut plan of a piece-wise decode, the pinned mirror's layout), compiled into a stand-alone program under the
address and undefined-behaviour sanitizers and run.  The checks themselves are in tests/c/inflate_plan_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inflate_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "inflate_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "qatzip_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "inflate_plan_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "inflate_plan_test: ok" in r.stdout
