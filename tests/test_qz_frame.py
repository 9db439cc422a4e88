"""The host rules of the compress calls that need no GPU (qatzip_amd/csrc/qz_frame.h: the delivery rule, member framing,
the folds of the crc out-parameter, the bounds; qzd_slot_host.h: the slots of a round), compiled into a stand-alone program
under the address and undefined-behaviour sanitizers and run.  The checks themselves are in tests/c/qz_frame_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qz_frame_under_sanitizers(tmp_path):
    exe = str(tmp_path / "qz_frame_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "qatzip_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "qz_frame_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "qz_frame_test: ok" in r.stdout
