"""bench.py --dump-outputs: what the last timed step returned, as float32 / float64 .npy files that two runs (or two builds)
can be compared by.  Driven here with host arrays standing in for the device buffers - no GPU needed."""
import os
import subprocess
import sys
import zlib

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Buf:
    def __init__(self, a):
        self.a = a

    def download(self, n, offset=0):
        return self.a[offset:offset + n].copy()


class _Ctx:
    def crc32(self, d, n):
        return zlib.crc32(d.a[:n].tobytes())


def _dump(path, seed_data=7):
    g = np.random.default_rng(seed_data)
    comp = [_Buf(g.integers(0, 256, 3_000_000, dtype=np.uint8)), _Buf(g.integers(0, 256, 50_000, dtype=np.uint8))]
    back = _Buf(g.integers(0, 256, 5_000_000, dtype=np.uint8))
    bench.dump_outputs(str(path), _Ctx(), comp, [3_000_000, 40_000], [123, 456], back, 5_000_000)
    return comp, back


def test_dump_outputs_is_deterministic_and_small(tmp_path):
    comp, back = _dump(tmp_path / "a")
    _dump(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["compressed_crc32.npy", "compressed_len.npy", "compressed_sample.npy", "decompressed_crc32.npy",
                     "decompressed_sample.npy"]
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
        total += os.path.getsize(tmp_path / "a" / f)
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "compressed_len.npy").tolist() == [3_000_000, 40_000]
    assert np.load(tmp_path / "a" / "compressed_crc32.npy").tolist() == [zlib.crc32(comp[0].a.tobytes()),
                                                                         zlib.crc32(comp[1].a[:40_000].tobytes())]
    assert np.load(tmp_path / "a" / "decompressed_crc32.npy").tolist() == [123, 456]
    s = np.load(tmp_path / "a" / "decompressed_sample.npy")
    assert s.size == 32 * 65536 and s.min() >= 0 and s.max() <= 255        # 32 blocks of bytes, exact in float32
    blk = s[:65536].astype(np.uint8).tobytes()
    assert back.a.tobytes().find(blk) >= 0                                  # a block is a slice of the output


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
