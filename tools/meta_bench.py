#!/usr/bin/env python3
"""Developer tool: what block-addressable compression costs on top of the paths it stands on, device-resident, by the host
clock around device-layer calls that end in a synchronise (one warm-up call, then --calls timed ones, all printed).

  (a) qzd_blocks_compress against qzd_deflate_slots alone on the same input: the difference is hash + four CRCs + plan + pack
  (b) qzd_crcn_ranges with the gzip config against qzd_crc32_ranges (qzk_block_crc32, the routine of the chunk CRCs of the
      deflate path) on the same ranges, and CRC-64/ECMA-182 alone
  (c) qzd_blocks_decompress against qzd_inflate_segments alone on the same blocks

usage: meta_bench.py [--mib 1024] [--block 65536] [--level 1] [--calls 3] [--label TEXT]
For the launch count per call: rocprofv3 --kernel-trace --stats -- python tools/meta_bench.py --mib 1 --calls 1 and again
with --mib 1024 (16 and 16384 blocks): the count of kernel launches per blocks_compress / blocks_decompress call must be
the same.  The output of every call is checked (round trip, CRCs of sampled blocks against zlib)."""
import argparse
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
import qatzip_amd  # noqa: E402
from qatzip_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=1024)
ap.add_argument("--block", type=int, default=65536)
ap.add_argument("--level", type=int, default=1)
ap.add_argument("--calls", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()
n, B = args.mib << 20, args.block
nb = (n + B - 1) // B
ctx = qatzip_amd.Context(0)
L = ctx.L
L.qzd_deflate_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64,
                                C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]

base = datagen.gen("silesia", min(64 << 20, n), 20250523)
reps = (n + base.size - 1) // base.size
src = np.concatenate([np.roll(base, 4099 * i) for i in range(reps)])[:n] if reps > 1 else base
d_src = ctx.alloc(nb * B); d_src.upload(src)
cap = _lib.max_deflate_len(n, B)
d_dst = ctx.alloc(cap)
d_out = ctx.alloc(nb * B)


def timed(what, fn, nbytes):
    ts = []
    for k in range(args.calls + 1):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        if k:
            ts.append(dt * 1e3)
    med = sorted(ts)[len(ts) // 2]
    print("%s %-44s %s ms  (%.1f GB/s of %d bytes by the median)" % (args.label, what, " / ".join("%.3f" % t for t in ts),
                                                                    nbytes / (med * 1e-3) / 1e9, nbytes), flush=True)
    return r


cdesc = np.array([min(B, n - k * B) | 0x80000000 for k in range(nb)], np.uint32)
slot_len = np.zeros(nb, np.uint32); ol = C.c_uint64(0)


def slots():
    ctx._chk(L.qzd_deflate_slots(ctx.h, d_src.ptr, nb, B, args.level, cdesc.ctypes.data, d_dst.ptr, cap, C.byref(ol),
                                 slot_len.ctypes.data, None))
    return ol.value


print("%s %d MiB in %d blocks of %d bytes, level %d" % (args.label, args.mib, nb, B, args.level), flush=True)
timed("(a) qzd_deflate_slots alone", slots, n)
recs = np.zeros(nb, _lib.BLOCKREC_DT)
rc = timed("(a) qzd_blocks_compress (thr = block size)", lambda: L.qzd_blocks_compress(ctx.h, d_src.ptr, n, B, args.level, B, None, None, d_dst.ptr,
                                                                                        d_dst.nbytes, recs.ctypes.data, C.byref(ol)), n)
total = ol.value
assert rc == 0 and (recs["size"][recs["flags"] == 1] == slot_len[recs["flags"] == 1]).all()
for k in (0, nb // 2, nb - 1):
    piece = src[k * B:(k + 1) * B].tobytes()
    assert int(recs["in_crc32"][k]) == zlib.crc32(piece), k
    got = d_dst.download(int(recs["size"][k]), int(recs["offset"][k])).tobytes()
    assert int(recs["out_crc32"][k]) == zlib.crc32(got) and (zlib.decompress(got, -15) if recs["flags"][k] else got) == piece, k

ranges = [(k * B, min(B, n - k * B)) for k in range(nb)]
ra = np.array([(o, z, 0) for o, z in ranges], dtype=_lib.RANGE_DT)
c32 = np.zeros(nb, np.uint32)
timed("(b) qzd_crc32_ranges (qzk_block_crc32)", lambda: ctx._chk(L.qzd_crc32_ranges(ctx.h, d_src.ptr, ra.ctypes.data, nb, c32.ctypes.data)), n)
g32, g64 = np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)
gz, ecma = _lib.CrcCfg(0x04C11DB7, 0xFFFFFFFF, 1, 1, 0xFFFFFFFF), _lib.CrcCfg(0x42F0E1EBA9EA3693, 0, 0, 0, 0)
timed("(b) qzd_crcn_ranges, gzip CRC-32", lambda: ctx._chk(L.qzd_crcn_ranges(ctx.h, d_src.ptr, ra.ctypes.data, nb, 32, C.byref(gz), None, g32.ctypes.data)), n)
assert (g32.astype(np.uint32) == c32).all()
timed("(b) qzd_crcn_ranges, CRC-64/ECMA-182", lambda: ctx._chk(L.qzd_crcn_ranges(ctx.h, d_src.ptr, ra.ctypes.data, nb, 64, C.byref(ecma), None, g64.ctypes.data)), n)
assert (g64 == recs["in_crc64"]).all()

comp_segs = [(int(r["offset"]), k * B, int(r["size"]), min(B, n - k * B), 0, int(r["size"])) for k, r in enumerate(recs) if r["flags"]]
if comp_segs:
    sa = np.array(comp_segs, dtype=_lib.SEG_DT); res = np.zeros(len(comp_segs), _lib.RES_DT)
    timed("(c) qzd_inflate_segments alone (%d compressed blocks)" % len(comp_segs),
          lambda: ctx._chk(L.qzd_inflate_segments(ctx.h, d_dst.ptr, d_out.ptr, sa.ctypes.data, len(sa), res.ctypes.data)), n)
    assert (res["status"] == 0).all()
status = np.zeros(nb, np.int32); produced = C.c_uint64(0)
rc = timed("(c) qzd_blocks_decompress", lambda: L.qzd_blocks_decompress(ctx.h, d_dst.ptr, total, recs.ctypes.data, nb, B, d_out.ptr, d_out.nbytes,
                                                                       status.ctypes.data, C.byref(produced)), n)
assert rc == 0 and produced.value == n and np.array_equal(d_out.download(n), src)
for b in (d_src, d_dst, d_out):
    b.free()
ctx.close()
