"""qzstd-amd (qatzip_amd/cli/qzstd_amd.c): a file to .zst through a zstd session, the output split into frames by the strict
reader and compared to the input; -d is not offered."""
import os
import subprocess

import pytest

import qatzip_amd.build as B
import zstd_format as Z
import zstd_ref
import zstd_sim as S


@pytest.mark.gpu
def test_file_to_zst(tmp_path):
    B.build()
    src = S.make_input("silesia", 300000, 17)
    p = tmp_path / "data.bin"
    p.write_bytes(src)
    r = subprocess.run([B.ZSTD_CLI, "-k", "-C", "32768", "-m", "4", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = (tmp_path / "data.bin.zst").read_bytes()
    frames = Z.decode_frames(out)
    assert len(frames) == 10 and [f["content_size"] for f in frames] == [32768] * 9 + [300000 - 9 * 32768]
    assert b"".join(f["data"] for f in frames) == src and p.exists()
    assert min(ml for f in frames if f["sequences"] for _, ml, _ in f["sequences"]) >= 4
    zstd_ref.check(out, src)
    # -o, and without -k the input goes
    q = tmp_path / "other.zst"
    r = subprocess.run([B.ZSTD_CLI, "-o", str(q), str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not p.exists() and Z.decode(q.read_bytes(), 65536) == src
    r = subprocess.run([B.ZSTD_CLI, "-C", "262144", str(q)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "refused" in r.stderr and q.exists()


def test_decompression_is_not_offered(tmp_path):
    """needs no device: -d answers before a session is made"""
    B.build()
    r = subprocess.run([B.ZSTD_CLI, "-d", str(tmp_path / "x.zst")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "zstd -d" in r.stderr
    r = subprocess.run([B.ZSTD_CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-C <bytes>" in r.stdout
