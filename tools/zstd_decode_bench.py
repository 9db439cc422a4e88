#!/usr/bin/env python3
"""Developer tool: the zstd decoder (qzd_zstd_decompress_frames) on device-resident frames of this project's writer, its two
stages alone, and libzstd's ZSTD_decompress on 16 threads of the same box where libzstd loads.

The data is bench.py's: 128 MiB of datagen's `silesia`, tiled with a period that is no multiple of a chunk, compressed in
the same process by qzd_zstd_compress_frames (mini_match 3) at 64 KB and 128 KB chunks.  Per configuration one warm-up call,
then --calls timed ones; GB/s is OUTPUT bytes over the call's kernels, first to last, by HIP events (qzd_last_timing), the
best call.  Stage E alone is a call with QATZIP_AMD_ZSTDD_STAGES=1, E and X one with =3 (qzd_zstdd.hip): the launches are
serial on one stream, so stage X is the difference.  The decoded bytes of the full call are compared with the input.
usage: zstd_decode_bench.py [--mib 1024] [--calls 3]

--one-frame MIB measures the block route instead (qzd_zstd_decompress_frames_ex, qzk_zstdd_blocks.h;
profiles/zstd_decode_blocks.txt): ONE frame of MIB MiB of the same data - libzstd's, level 3, with and without a content
checksum, where libzstd loads; otherwise the blocks of this writer's 128 KB frames behind one frame header - under route
`blocks` and route `frame` in the same process, the stages by QATZIP_AMD_ZSTDD_STAGES as above (=1: Plan to Finish, or stage
E).  Route `frame` takes --frame-mib MiB of the same frame's data (default 16: its bit streams run at a few MB/s a frame, the
tool says which size it timed).  Then the sweep that sets QZD_ZD_BLOCKS_MIN - 512 frames a call of 1, 2, 4, 8 and 16 blocks
of 128 KB, both routes - and the route's bit-stream stage beside stage E on the same bytes cut into 64 KB frames of this
writer."""
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
ap.add_argument("--one-frame", type=int, default=0, metavar="MIB")
ap.add_argument("--frame-mib", type=int, default=16)
args = ap.parse_args()


def one_frame():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_zstd_dec_blocks as G
    import zstdd_blocks_sim as B
    n = args.one_frame << 20
    base = datagen.gen("silesia", min(128 << 20, n), 20250523)
    tile = len(base) - TILE_SKEW if n > len(base) else len(base)
    src = np.empty(n, np.uint8)
    for off in range(0, n, tile):
        m = min(tile, n - off)
        src[off:off + m] = base[:m]
    ctx = qatzip_amd.Context(0)
    d_out = ctx.alloc(n + 64)
    print("one frame: %d MiB of silesia, tiled; ms of the call's kernels by HIP events, best of %d calls after a warm-up" % (args.one_frame, args.calls))

    def writer_frames(data, hw):
        d_s = ctx.alloc(len(data)); d_s.upload(data)
        d_d = ctx.alloc(zstd_bound(len(data), hw) + 64)
        zn, lens = ctx.zstd_compress_frames(d_s, len(data), d_d, hw, 3, 1)
        out = d_d.download(zn).tobytes()
        d_s.free(); d_d.free()
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.int64)
        return [out[offs[i]:offs[i + 1]] for i in range(len(lens))]

    def make(data, checksum):
        """-> (frame, what)"""
        if zstd_ref.available():
            return G.libzstd_frame(data.tobytes(), 3, checksum, window_log=21), "libzstd %d level 3, windowLog 21" % zstd_ref.version()
        return G.stitched(writer_frames(data, 131072)), "this writer's 128 KB blocks behind one frame header"

    def timed(d_c, segs, counts, route, stages, want=None, d_out=d_out):
        if stages:
            os.environ["QATZIP_AMD_ZSTDD_STAGES"] = stages
        else:
            os.environ.pop("QATZIP_AMD_ZSTDD_STAGES", None)
        ms = []
        for k in range(args.calls + 1):
            res = ctx.zstd_decompress_frames(d_c, d_out, segs, nblocks=counts, route=route)
            if k:
                ms.append(ctx.timing()[3])
        os.environ.pop("QATZIP_AMD_ZSTDD_STAGES", None)
        if not stages:
            assert all(int(r["status"]) == 0 and int(r["out_len"]) == s[3] and int(r["in_used"]) == s[2] for r, s in zip(res, segs)), res[:4]
            if want is not None:
                assert d_out.download(len(want)).tobytes() == want.tobytes(), "the output is not the input"
        return min(ms)

    def legs(name, frame, data, route):
        nb = B.walk_count(frame)
        d_c = ctx.alloc(len(frame) + 64); d_c.upload(frame)
        segs = [(0, 0, len(frame), len(data))]
        full = timed(d_c, segs, [nb], route, None, data)
        e = timed(d_c, segs, [nb], route, "1")
        ex = timed(d_c, segs, [nb], route, "3")
        d_c.free()
        gb = len(data) / 1e9
        print("%-34s %4d MiB %5d blocks, route %-6s %9.1f ms = %7.3f GB/s | bit streams %9.1f ms (%4.1f %%)  X %9.1f ms (%4.1f %%)  XXH64 %8.1f ms (%4.1f %%)" %
              (name, len(data) >> 20, nb, route, full, gb / (full * 1e-3), e, 100 * e / full, ex - e, 100 * (ex - e) / full, full - ex, 100 * (full - ex) / full),
              flush=True)
        return full

    fm = min(args.frame_mib << 20, n)
    for checksum in (0, 1):
        frame, what = make(src, checksum)
        name = "%s%s" % ("checksum" if checksum else "no checksum", "" if zstd_ref.available() else " (none: this writer)")
        if not checksum:
            print("the frame: %s, %d bytes (ratio %.4f)" % (what, len(frame), len(frame) / n))
        b = legs(name, frame, src, "blocks")
        if fm != n:
            small, _ = make(src[:fm], checksum)
            print("    route frame is timed on the first %d MiB of the same data as a frame of its own:" % (fm >> 20))
            bs = legs("    " + name, small, src[:fm], "blocks")
            f = legs("    " + name, small, src[:fm], "frame")
            print("    route blocks is %.1fx route frame on that frame" % (f / bs))
        else:
            f = legs(name, frame, src, "frame")
            print("    route blocks is %.1fx route frame" % (f / b))
        if not zstd_ref.available():
            break
    # ---- the sweep: 512 frames a call of 1 .. 16 blocks of 128 KB
    print("sweep for QZD_ZD_BLOCKS_MIN: 512 frames a call, k blocks of 128 KB a frame, ms of the whole call (bit streams alone)")
    for k in (1, 2, 4, 8, 16):
        per = k * 131072
        nf, distinct = 512, min(512, n // per)                     # (the data's frames over again where it holds fewer than 512)
        frames = [make(src[i * per:(i + 1) * per], 0)[0] for i in range(distinct)]
        comp = b"".join(frames)
        d_c = ctx.alloc(len(comp) + 64); d_c.upload(comp)
        d_o = ctx.alloc(nf * per + 64)
        offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
        segs = [(int(offs[i % distinct]), i * per, len(frames[i % distinct]), per) for i in range(nf)]
        counts = [B.walk_count(frames[i % distinct]) for i in range(nf)]
        row = []
        for route in ("frame", "blocks"):
            row.append((timed(d_c, segs, counts, route, None, src[:per], d_o), timed(d_c, segs, counts, route, "1", None, d_o)))
        d_c.free(); d_o.free()
        print("    k = %2d  %3d frames (%d..%d blocks)  frame %8.2f ms (%8.2f)   blocks %8.2f ms (%8.2f)   blocks / frame %.2f" %
              (k, nf, min(counts), max(counts), row[0][0], row[0][1], row[1][0], row[1][1], row[1][0] / row[0][0]), flush=True)
    # ---- the same bytes as many small frames of this writer: stage E beside the route's bit-stream stage
    fr64 = writer_frames(src, 65536)
    comp = b"".join(fr64)
    d_c = ctx.alloc(len(comp) + 64); d_c.upload(comp)
    offs = np.concatenate([[0], np.cumsum([len(f) for f in fr64])])
    segs = [(int(offs[i]), i * 65536, len(fr64[i]), min(65536, n - i * 65536)) for i in range(len(fr64))]
    full = timed(d_c, segs, None, "frame", None, src)
    e = timed(d_c, segs, None, "frame", "1")
    d_c.free()
    print("the same %d MiB as %d frames of 64 KB of this writer: the call %.1f ms, stage E alone %.1f ms = %.2f GB/s (not gated; the writer's frames "
          "are not libzstd's)" % (args.one_frame, len(fr64), full, e, n / (e * 1e-3) / 1e9))
    ctx.close()


if args.one_frame:
    one_frame()
    sys.exit(0)
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
