#!/usr/bin/env python3
"""Developer tool: randomized campaign on the CPU emulator for the LZ4-HC kernels (qzk_lz4hc.h: chains, parse, finish)
against liblz4 1.9.3 itself, byte for byte: calls of random kinds / sizes / levels 3-8 as one frame (one block, or linked
blocks), as hardware-path frames per chunk, in one round or in rounds of a few blocks; plus inputs that barely shrink
(random bytes with planted repeats), where liblz4's two overflow tests decide between a stored and a compressed block.
usage: sim_fuzz_lz4hc.py [seconds] [first seed]"""
import ctypes as C
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
import refcalls  # noqa: E402

assert refcalls.lz4_pinned(), "needs liblz4 1.9.3"
SIMDIR = os.path.join(ROOT, "tests", "sim")


def build():
    so = os.path.join(SIMDIR, "libqzsim_lz4hc.so")
    csrc = os.path.join(ROOT, "qatzip_amd", "csrc")
    deps = [os.path.join(SIMDIR, "sim_lz4hc.cpp"), os.path.join(SIMDIR, "hipsim.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-I", SIMDIR, "-Wno-unused-function",
                               "-o", so, os.path.join(SIMDIR, "sim_lz4hc.cpp")])
    return so


S = C.CDLL(os.environ.get("QZSIM_LZ4HC_SO") or build())
S.sim_lz4hc.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                        C.POINTER(C.c_uint64), C.c_void_p]


def sim(src, level, frame_sz, hw, batch):
    n = len(src)
    cap = n + 64 + 32 * (n // 65536 + n // frame_sz + 2)
    out = C.create_string_buffer(cap); ol = C.c_uint64(0)
    rc = S.sim_lz4hc(src, n, frame_sz, level, hw, batch, out, cap, C.byref(ol), None)
    assert rc == 0, rc
    return out.raw[:ol.value]


def xxh32_small(b):
    """XXH32 (seed 0) of fewer than sixteen bytes: a frame descriptor"""
    M = 0xffffffff
    h = (374761393 + len(b)) & M
    i = 0
    while i + 4 <= len(b):
        h = (h + int.from_bytes(b[i:i + 4], "little") * 3266489917) & M
        h = (((h << 17) | (h >> 15)) & M) * 668265263 & M
        i += 4
    while i < len(b):
        h = (h + b[i] * 374761393) & M
        h = (((h << 11) | (h >> 21)) & M) * 2654435761 & M
        i += 1
    h ^= h >> 15; h = h * 2246822519 & M; h ^= h >> 13; h = h * 3266489917 & M; h ^= h >> 16
    return h


def hw_frames(src, chunk, level):
    """what the hardware path's framing makes of the library's frames: FLG 0x4C in every chunk's header"""
    out = b""
    for o in range(0, len(src), chunk):
        f = bytearray(refcalls.lz4f_compress_frame(src[o:o + chunk], level))
        f[4] = 0x4C
        f[14] = (xxh32_small(bytes(f[4:14])) >> 8) & 0xff
        out += bytes(f)
    return out


def barely(rng, n):
    """random bytes with sparse planted repeats: blocks that land within a few bytes of n - 1"""
    b = bytearray(rng.randbytes(n))
    for _ in range(rng.randrange(0, max(2, n // 300))):
        ln = rng.randrange(5, 9)
        if n < 3 * ln:
            break
        a = rng.randrange(0, n - 2 * ln); d = rng.randrange(a + ln, n - ln)
        b[d:d + ln] = b[a:a + ln]
    return bytes(b)


budget = float(sys.argv[1]) if len(sys.argv) > 1 else 300
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
t0 = time.time(); n_ok = 0; nblk = 0; bad = []
while time.time() - t0 < budget:
    rng = random.Random(seed)
    level = rng.randrange(3, 9)
    mode = rng.choice(["one", "one", "one", "hw", "barely"])
    n = rng.choice([rng.randrange(0, 300), rng.randrange(300, 20000), rng.randrange(20000, 70000), rng.randrange(65000, 66000),
                    rng.randrange(70000, 280000)])
    if mode == "barely":
        src = barely(rng, min(n, 140000))
    else:
        kind = rng.choice(datagen.KINDS)
        if kind == "lzmix":
            n = min(n, 80000)
        src = datagen.gen_bytes(kind, n, 5000 + seed)
        if rng.random() < 0.3 and n > 64:
            cut = rng.randrange(1, n); src = (src[cut:] + src[:cut] + src)[:n]
        if rng.random() < 0.2 and n > 1000:
            at = rng.randrange(0, n - 500); per = bytes(rng.randrange(256) for _ in range(rng.choice([1, 2, 3, 5, 7, 8, 13, 300])))
            ln = rng.randrange(10, min(n - at, 40000)); src = src[:at] + (per * (ln // len(per) + 1))[:ln] + src[at + ln:]
    n = len(src)
    batch = rng.choice([0, 0, 1, 2, 3])
    if mode == "hw" and n:
        chunk = rng.choice([65536, 131072, 100000, 16384, 262144])
        got = sim(src, level, chunk, 1, batch); exp = hw_frames(src, chunk, level)
    else:
        got = sim(src, level, max(n, 1), 0, batch); exp = refcalls.lz4f_compress_frame(src, level)
    if got != exp:
        bad.append((seed, mode, level, n, batch)); print("MISMATCH", bad[-1], flush=True)
    else:
        n_ok += 1
    nblk += max(1, (n + 65535) // 65536)
    seed += 1
print("up to seed %d: %d calls ok (%d blocks), %d mismatches %s" % (seed - 1, n_ok, nblk, len(bad), bad))
