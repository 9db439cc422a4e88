#!/usr/bin/env python3
"""Developer tool: the zstd decoder (qzd_zstd_decompress_frames) on device-resident frames of this project's writer, its two
stages alone, and libzstd's ZSTD_decompress on 16 threads of the same box where libzstd loads.

The data is bench.py's: 128 MiB of datagen's `silesia`, tiled with a period that is no multiple of a chunk, compressed in
the same process by qzd_zstd_compress_frames (mini_match 3) at 64 KB and 128 KB chunks.  Per configuration one warm-up call,
then --calls timed ones; GB/s is OUTPUT bytes over the call's kernels, first to last, by HIP events (qzd_last_timing), the
best call.  Stage E alone is a call with QATZIP_AMD_ZSTDD_STAGES=1, E and X one with =3 (qzd_zstdd.hip): the launches are
serial on one stream, so stage X is the difference.  The decoded bytes of the full call are compared with the input.
usage: zstd_decode_bench.py [--mib 1024] [--calls 3]"""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
import zstd_ref  # noqa: E402
import qatzip_amd  # noqa: E402
from qatzip_amd._lib import zstd_bound  # noqa: E402

TILE_SKEW = 4099                    # as bench.py

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--calls", type=int, default=3)
args = ap.parse_args()
n = args.mib << 20
base = datagen.gen("silesia", min(128 << 20, n), 20250523)
ctx = qatzip_amd.Context(0)
d_src = ctx.alloc(n)
tile = len(base) - TILE_SKEW if n > len(base) else len(base)
for off in range(0, n, tile):
    d_src.upload(base[:min(tile, n - off)], off)
d_c = ctx.alloc(zstd_bound(n, 65536) + 4096)
d_out = ctx.alloc(n + 64)
print("%d MiB resident, silesia tiled so that no two chunks are equal; GB/s of output by HIP events, best of %d calls" % (args.mib, args.calls))


def run(what, segs, stages):
    if stages:
        os.environ["QATZIP_AMD_ZSTDD_STAGES"] = stages
    else:
        os.environ.pop("QATZIP_AMD_ZSTDD_STAGES", None)
    ms = []
    for k in range(args.calls + 1):
        res = ctx.zstd_decompress_frames(d_c, d_out, segs)
        if k:
            ms.append(ctx.timing()[3])
    os.environ.pop("QATZIP_AMD_ZSTDD_STAGES", None)
    print("%-52s %8.2f GB/s   (ms: %s)" % (what, n / (min(ms) * 1e-3) / 1e9, " / ".join("%.1f" % m for m in ms)), flush=True)
    return res, min(ms)


for hw in (65536, 131072):
    zn, lens = ctx.zstd_compress_frames(d_src, n, d_c, hw, 3, 1)
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]])
    segs = [(int(o), i * hw, int(ln), min(hw, n - i * hw)) for i, (o, ln) in enumerate(zip(offs, lens))]
    print("%d KB chunks: %d frames, %.1f MiB of zstd (ratio %.4f)" % (hw >> 10, len(segs), zn / 2**20, zn / n), flush=True)
    res, full = run("Kzd decode, stages E + X + checksum kernel", segs, None)
    assert all(int(r["status"]) == 0 and int(r["out_len"]) == s[3] and int(r["in_used"]) == s[2] for r, s in zip(res, segs))
    for off in range(0, n, 256 << 20):
        m = min(64 << 20, n - off)
        assert d_out.download(m, off).tobytes() == d_src.download(m, off).tobytes()
    print("    (the output equals the input on the first 64 MiB of every 256 MiB)")
    _, e = run("    stage E alone (the bit streams)", segs, "1")
    _, ex = run("    stages E and X", segs, "3")
    print("    stage X by difference: %.1f ms = %.2f GB/s; the checksum kernel's launches (no frame has one): %.1f ms" %
          (ex - e, n / ((ex - e) * 1e-3) / 1e9, full - ex), flush=True)
    if zstd_ref.available():
        L = zstd_ref.lib()
        stream = d_c.download(zn).tobytes()
        W = 16
        parts = [list(range(w, len(segs), W)) for w in range(W)]

        def work(ids):
            dst = C.create_string_buffer(hw)
            for i in ids:
                o, _, ln, cap = segs[i]
                r = L.ZSTD_decompress(dst, cap, stream[o:o + ln], ln)
                assert r == cap
        best = 1e9
        for _ in range(2):
            t = time.perf_counter()
            with ThreadPoolExecutor(W) as ex_:
                list(ex_.map(work, parts))
            best = min(best, time.perf_counter() - t)
        print("    libzstd %d ZSTD_decompress on %d threads (ctypes, one call a frame): %.2f GB/s" % (zstd_ref.version(), W, n / best / 1e9), flush=True)
    else:
        print("    libzstd does not load here: no CPU figure")
ctx.close()
