"""The host rules of the decompress calls that need no GPU (qatzip_amd/csrc/qz_unframe.h: the member header, sized gzip-ext
members, one member as one inflate segment, the LZ4 frame extent, the frame plan and its result check, the folds of the crc
out-parameter), compiled into a stand-alone program under the address and undefined-behaviour sanitizers and run.  The checks
themselves are in tests/c/qz_unframe_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_qz_unframe_under_sanitizers(tmp_path):
    exe = str(tmp_path / "qz_unframe_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "qatzip_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "qz_unframe_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "qz_unframe_test: ok" in r.stdout
