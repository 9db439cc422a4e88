"""qzstd-amd --decompress (qatzip_amd/cli/qzstd_amd.c): a file to .zst and back, a file of libzstd's committed frames back to
back, and the short -d, which keeps its old answer."""
import hashlib
import subprocess

import pytest

import qatzip_amd.build as B
import zstd_sim as S
import zstdd_sim as D

pytestmark = pytest.mark.gpu


def test_compress_then_decompress_gives_the_input_back(tmp_path):
    B.build()
    src = S.make_input("silesia", 300000, 17)
    p = tmp_path / "data.bin"
    p.write_bytes(src)
    r = subprocess.run([B.ZSTD_CLI, "-C", "32768", str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not p.exists(), r.stderr
    z = tmp_path / "data.bin.zst"
    r = subprocess.run([B.ZSTD_CLI, "--decompress", "-k", str(z)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and z.exists(), r.stderr
    assert p.read_bytes() == src
    # -o, and without -k the .zst goes
    q = tmp_path / "again"
    r = subprocess.run([B.ZSTD_CLI, "--decompress", "-o", str(q), str(z)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not z.exists() and q.read_bytes() == src, r.stderr
    # a cut file leaves no output behind
    c = tmp_path / "cut.zst"
    r = subprocess.run([B.ZSTD_CLI, "-k", "-o", str(c), str(q)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    c.write_bytes(c.read_bytes()[:-3])
    r = subprocess.run([B.ZSTD_CLI, "--decompress", "-k", str(c)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cut" in r.stderr and not (tmp_path / "cut").exists()
    # the short option keeps its old answer
    r = subprocess.run([B.ZSTD_CLI, "-d", str(c)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "zstd -d" in r.stderr and c.exists()


def test_a_file_of_libzstds_frames(tmp_path):
    """the seventeen frames of (a) back to back, a skippable frame among them"""
    B.build()
    idx = D.index()
    a = [e for e in idx["frames"] if e["group"] == "a"]
    skip = next(e for e in idx["frames"] if e["name"] == "c_skippable")
    z = tmp_path / "all.zst"
    z.write_bytes(b"".join(D.frame_bytes(e) for e in a[:9] + [skip] + a[9:]))
    want = hashlib.sha256()
    for e in a:
        want.update(S.make_input(e["recipe"]["kind"], e["recipe"]["n"], e["recipe"]["seed"]))
    r = subprocess.run([B.ZSTD_CLI, "--decompress", str(z)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not z.exists(), r.stderr
    out = (tmp_path / "all").read_bytes()
    assert len(out) == sum(e["content"] for e in a) and hashlib.sha256(out).hexdigest() == want.hexdigest()

