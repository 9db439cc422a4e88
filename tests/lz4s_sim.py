"""The LZ4s kernel (qatzip_amd/csrc/qzk_lz4s.h) on the CPU SIMT emulator, and the inputs the LZ4s tests share: used by
tests/test_sim_lz4s.py, tests/test_gpu_lz4s.py and tests/golden/gen_lz4s.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import datagen
import lz4s_format

HERE = os.path.dirname(os.path.abspath(__file__))
SIMDIR = os.path.join(HERE, "sim")
ROOT = os.path.dirname(HERE)
SO = os.path.join(SIMDIR, "libqzsim_lz4s.so")

_S = None


def build_so():
    """g++ build of tests/sim/sim_lz4s.cpp, redone when a source is newer"""
    deps = [os.path.join(SIMDIR, f) for f in ("sim_lz4s.cpp", "hipsim.h")]
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function",
                               "-o", SO, os.path.join(SIMDIR, "sim_lz4s.cpp")])
    return SO


def _load():
    global _S
    if _S is None:
        S = C.CDLL(build_so())
        S.sim_lz4s.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                               C.POINTER(C.c_uint64), C.c_void_p]
        _S = S
    return _S


def compress(src, hw_buff_sz=65536, mini_match=3, waves=0):
    """-> (stream, per-block lengths).  The driver itself checks that no block passes its bound and that nothing is written
    behind it (rc -3)."""
    S = _load()
    n = len(src)
    nb = (n + hw_buff_sz - 1) // hw_buff_sz
    cap = lz4s_format.bound(n, hw_buff_sz) + 64
    out = C.create_string_buffer(cap)
    ol = C.c_uint64(0)
    lens = (C.c_uint32 * max(nb, 1))()
    rc = S.sim_lz4s(src, n, hw_buff_sz, mini_match, waves, out, cap, C.byref(ol), lens)
    assert rc == 0, "sim_lz4s rc=%d" % rc
    return out.raw[:ol.value], list(lens)[:nb]


def _rand(n, seed):
    return np.random.Generator(np.random.PCG64([seed, 99])).integers(0, 256, n).astype(np.uint8).tobytes()


def window_input(seed=5):
    """The layout the LZ4s issue words, kept for that wording only: 131072 bytes, 70000 random ones, then three 3000-byte
    copies of pieces of them - at 70000 of the first 3000 bytes (source 70000 back), at 73000 of what lies exactly 65535
    back, at 76000 of what lies exactly 65536 back - then random.  (Copies of the FIRST 3000 bytes at 65535 and 65536 back
    cannot lie behind 70000 random bytes, so the latter two are copies of other pieces.)  It does not test the window: by
    the time the copies arrive, the 4096-entry table has long lost their sources to the random bytes in between, so no
    far candidate is ever met.  far_input() below carries that check."""
    r = bytearray(_rand(131072, seed))
    r[70000:73000] = r[0:3000]
    r[73000:76000] = r[73000 - 65535:76000 - 65535]
    r[76000:79000] = r[76000 - 65536:79000 - 65536]
    return bytes(r)


def far_input(dist, seed=6):
    """131072 bytes: 3000 random ones, zeros, the 3000 again `dist` bytes behind their first copy, zeros.  The zeros leave the
    table entries of the 3000 alone, so their second copy meets candidates exactly `dist` back."""
    f = _rand(3000, seed)
    b = bytearray(131072)
    b[0:3000] = f
    b[dist:dist + 3000] = f
    return bytes(b)


def make_input(kind, n, seed):
    """datagen's kinds, and the built ones: "window", "far65535", "far65536" (n = 131072)"""
    if kind == "window":
        assert n == 131072
        return window_input(seed)
    if kind.startswith("far"):
        assert n == 131072
        return far_input(int(kind[3:]), seed)
    return datagen.gen_bytes(kind, n, seed)
