#!/usr/bin/env python3
"""Developer tool: the LZ4s kernel (K4s, qzd_lz4s_compress_blocks) on device-resident data, next to K4
(qzd_lz4_compress_frames) on the same buffer in the same process.

The data is bench.py's: 128 MiB of datagen's `silesia`, tiled with a period that is no multiple of a chunk, so no two chunks
are equal.  Per configuration one warm-up call, then --calls timed ones; GB/s is input bytes over the call's kernels, first
to last, by HIP events (qzd_last_timing), the best call; ratio is output bytes over input bytes.  A sample of blocks from
the start of the 64 KB stream is read back by the independent reader (tests/lz4s_format.py).
With --only KB:MM just that one K4s configuration runs (for a counter pass: one kernel shape per run).
usage: lz4s_bench.py [--mib 1024] [--calls 3] [--only 64:3]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
import lz4s_format  # noqa: E402
import qatzip_amd  # noqa: E402
from qatzip_amd._lib import lz4s_bound  # noqa: E402

TILE_SKEW = 4099                    # as bench.py

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--only", default=None)
args = ap.parse_args()
n = args.mib << 20
base = datagen.gen("silesia", min(128 << 20, n), 20250523)
ctx = qatzip_amd.Context(0)
d_src = ctx.alloc(n)
tile = len(base) - TILE_SKEW if n > len(base) else len(base)
for off in range(0, n, tile):
    d_src.upload(base[:min(tile, n - off)], off)
d_c = ctx.alloc(lz4s_bound(n, 1024) + 4096)
print("%d MiB resident, silesia tiled so that no two chunks are equal; GB/s by HIP events, best of %d calls" % (args.mib, args.calls))


def run(what, call):
    out = call()
    ms = []
    for _ in range(args.calls):
        assert call() == out
        ms.append(ctx.timing()[3])
    print("%-44s %8.2f GB/s   ratio %.4f   (ms: %s)" % (what, n / (min(ms) * 1e-3) / 1e9, out / n, " / ".join("%.1f" % m for m in ms)),
          flush=True)
    return out


if args.only:
    kb, mm = (int(x) for x in args.only.split(":"))
    run("K4s LZ4s  %3d KB chunks, mini_match %d" % (kb, mm), lambda: ctx.lz4s_compress_blocks(d_src, n, d_c, kb << 10, mm, 1)[0])
    ctx.close()
    sys.exit(0)
for mm in (3, 4):
    run("K4s LZ4s   64 KB chunks, mini_match %d" % mm, lambda: ctx.lz4s_compress_blocks(d_src, n, d_c, 65536, mm, 1)[0])
    if mm == 3:
        head = d_c.download(1 << 20).tobytes()
        pos, k = 0, 0
        src_head = d_src.download(8 * 65536).tobytes()
        while k < 8:
            size = int.from_bytes(head[pos:pos + 4], "little")
            data, _ = lz4s_format.decode_block(head[pos + 4:pos + 4 + size], 3)
            assert data == src_head[k * 65536:(k + 1) * 65536]
            pos += 4 + size; k += 1
        print("    (the first 8 blocks decode to their input)")
run("K4  LZ4    64 KB frames (qzd_lz4_compress_frames)", lambda: ctx.lz4_compress_frames(d_src, n, d_c, 65536)[0])
for hw in (131072, 524288):
    for mm in (3, 4):
        run("K4s LZ4s  %3d KB chunks, mini_match %d" % (hw >> 10, mm), lambda: ctx.lz4s_compress_blocks(d_src, n, d_c, hw, mm, 1)[0])
ctx.close()
