#!/usr/bin/env python3
"""Developer tool: decode of device-resident LZ4 frames of INDEPENDENT blocks through qzd_lz4_decompress_frames, timed by the
HIP events the device layer records around the call's GPU work (qzd_last_timing): one warm-up call, then three timed calls,
all three printed, and the host clock around each beside them.
Shapes (--shape, several allowed):
  1024x64k   ONE frame of 64 MiB in 1024 blocks of 64 KB - the block bodies of the library's own 64 KB software frames
             (ctx.lz4_compress_frames), re-framed by tests/lz4_frame_writer.py, as tests/test_gpu_lz4_blocks.py builds its
             16 MiB frame
  16x4m      ONE frame of 64 MiB in 16 blocks of 4 MiB, written by liblz4 (needs that library; else "not measured")
  2blk       ONE frame of two 64 KB blocks
  4096x2blk  one call of 4096 frames of two 64 KB blocks each
Each shape runs with and without a content checksum (--cc both|0|1).  --route auto|wave|blocks sets the route (libraries
that have the switch); QATZIP_AMD_SO=<library> measures another build, e.g. the parent commit's.  The output is checked
against the input on every call.
usage: lz4_frame_decode_bench.py [--shape 1024x64k] [--cc both] [--route auto] [--calls 3] [--label TEXT]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import datagen  # noqa: E402
import lz4_frame_writer as W  # noqa: E402
import qatzip_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", action="append")
ap.add_argument("--cc", default="both")
ap.add_argument("--route", default="auto")
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()
shapes = args.shape or ["1024x64k"]
ccs = {"both": (0, 1), "0": (0,), "1": (1,)}[args.cc]
ctx = qatzip_amd.Context(0)
if args.route != "auto":
    ctx.lz4_decode_route(args.route)


def source(n):
    base = datagen.gen("silesia", min(64 << 20, n), 20250523)
    reps = (n + base.size - 1) // base.size
    return (np.concatenate([np.roll(base, 4099 * i) for i in range(reps)])[:n] if reps > 1 else base).tobytes()


def bodies_64k(src):
    """[(body, stored)] of the 64 KB blocks of src, parsed by the library's own compressor"""
    n = len(src)
    d_s = ctx.alloc(n); d_s.upload(src)
    d_d = ctx.alloc(n + (n >> 16) * 64 + 4096)
    total, lens = ctx.lz4_compress_frames(d_s, n, d_d, 65536)
    comp = d_d.download(total).tobytes()
    d_s.free(); d_d.free()
    out, pos = [], 0
    for ln in lens:
        fr = comp[pos:pos + int(ln)]; pos += int(ln)
        (w, o, l), = W.blocks_of(fr)[0]
        out.append((fr[o:o + l], bool(w >> 31)))
    return out


def frames_of(shape, cc):
    """-> ([frames], [decoded parts]) or None"""
    if shape == "16x4m":
        import refcalls
        if not refcalls.lz4_pinned():
            return None
        import gen_lz4_blocks
        src = source(64 << 20)
        return [gen_lz4_blocks.compress_independent(src, 7, 0, cc, 1)], [src]
    per, count = {"1024x64k": (1024, 1), "2blk": (2, 1), "4096x2blk": (2, 4096)}[shape]
    src = source(per * count * 65536)
    bodies = bodies_64k(src)
    frames, parts = [], []
    for i in range(count):
        part = src[i * per * 65536:(i + 1) * per * 65536]
        frames.append(W.frame(bodies[i * per:(i + 1) * per], part, block_id=4, content_checksum=bool(cc), content_size=len(part)))
        parts.append(part)
    return frames, parts


for shape in shapes:
    for cc in ccs:
        made = frames_of(shape, cc)
        if made is None:
            print("%s %s cc=%d: not measured (liblz4 1.9.3 is not installed here)" % (args.label, shape, cc), flush=True)
            continue
        frames, parts = made
        comp = b"".join(frames)
        want = np.frombuffer(b"".join(parts), np.uint8)
        d_c = ctx.alloc(len(comp)); d_c.upload(comp)
        d_o = ctx.alloc(want.size)
        segs, io, oo = [], 0, 0
        for fr, p in zip(frames, parts):
            segs.append((io, oo, len(fr), len(p))); io += len(fr); oo += len(p)
        ev, host = [], []
        for k in range(args.calls + 1):
            t0 = time.perf_counter()
            res = ctx.lz4_decompress_frames(d_c, d_o, segs)
            dt = time.perf_counter() - t0
            assert (res["status"] == 0).all() and (res["out_len"] == [len(p) for p in parts]).all(), res[:4]
            assert np.array_equal(d_o.download(want.size), want)
            if k:
                ev.append(ctx.timing()[3]); host.append(dt * 1e3)
        print("%s %-10s cc=%d route=%s: %d frame(s), %d -> %d bytes: events %s ms, host clock %s ms  (%.2f GB/s by the median of the events)"
              % (args.label, shape, cc, args.route, len(frames), len(comp), want.size, " / ".join("%.3f" % t for t in ev),
                 " / ".join("%.3f" % t for t in host), want.size / (sorted(ev)[len(ev) // 2] * 1e-3) / 1e9), flush=True)
        d_c.free(); d_o.free()
ctx.close()
